"""GibbsEngine -- host-side orchestration of one macau() run on one MI355X (one process per GPU).

Everything numeric is a call into libbdf_hip.so (include/bdf.h).  torch is used for what the task calls plumbing: device
allocations (tensors) and, with several ranks, the channel over which rank 0 hands the RCCL unique id to the others.

* The whole iteration (the relations' models, rows of every entity, exchange between the GPUs, hyperpriors, beta, test
  prediction update) is ONE native call, bdf_gibbs_sweep (csrc/bdf_gibbs.hip).  BDF_NO_NATIVE: the same object's pieces -- relation
  step, row launches, hyperprior draws and steps, beta -- are driven one by one from here (bdf_gibbs_step_relations, _rows, _draws,
  _hyper, _beta), on three streams with plain stream order; only the prediction update goes through the entry points of bdf.h.
* Several ranks (shard=(rank, world)): every entity's rows are shared out by bdf_layout_build -- dealt over the ranks in
  falling order of degree as the reference deals rows i:P:N to its workers (src/sampling.jl:154) -- and stored at INTERNAL
  positions, so that a rank's rows of a chunk are one contiguous block and the exchange is an in-place all-gather
  (bdf_allgather_rows: RCCL over xGMI).  A rank holds the observations of its own rows only
  (bdf_relation_create_sharded) and a replica of every factor matrix.  Random streams are keyed by the original row id.

Layout: an entity's sample is the reference's D x N column-major matrix == a contiguous torch tensor of shape (N, D)
(N = chunks * world * cmax rows with a layout; EntityState.host() returns the reference's orientation and order).
"""
import ctypes as C
import math
import os
import sys
import weakref

import numpy as np
import torch

from . import _lib
from . import features as feat
from ._lib import ArgumentError, GibbsEntity, Term, check, lib
from .indexed_df import IndexedDF
from .relation_data import background_mean, check_model, dense_matrix, noise_kind


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _alpha_args(alpha, host=0.0):
    """alpha as the two arguments the entry points take: the host double, or -- a device scalar (tensor of one double) that only
    the device reads -- `host` and its address"""
    return (host, _ptr(alpha)) if torch.is_tensor(alpha) else (float(alpha), None)


class _DeviceObject:
    """an object of the library created on a context (self.ctx, self.handle): destroyed once, by the function `_destroy` names"""

    def close(self):
        if self.handle:
            if self.ctx.handle:                 # a closed context has already destroyed its objects
                getattr(lib(), self._destroy)(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _facs(factors):
    """the factor matrices of a relation's modes as the array of device pointers the entry points take"""
    fp = (C.c_void_p * len(factors))(*[f.data_ptr() for f in factors])
    return fp


class Layout:
    """internal row positions of an entity (bdf_layout_build); world == 1: the identity"""

    def __init__(self, N, degree=None, world=1, chunks=1):
        self.N, self.world, self.chunks = int(N), int(world), int(chunks)
        if world == 1 and chunks == 1:
            self.pos, self.cmax, self.nint = None, self.N, self.N
            return
        degree = np.ascontiguousarray(degree, dtype=np.int64)
        self.pos = np.zeros(self.N, dtype=np.int32)
        cmax = C.c_int64(0)
        check(lib().bdf_layout_build(self.N, degree.ctypes.data_as(_lib.c_i64p), world, chunks,
                                     self.pos.ctypes.data_as(_lib.c_i32p), C.byref(cmax)))
        self.cmax = cmax.value
        self.nint = self.chunks * self.world * self.cmax

    def to_internal(self, ids1):
        """1-based original ids -> 1-based internal positions"""
        ids1 = np.asarray(ids1)
        return ids1 if self.pos is None else self.pos[ids1 - 1].astype(np.int64) + 1

    def block(self, rank, chunk):
        """[begin, end) of the rows of (rank, chunk) in the factor matrix"""
        b = (chunk * self.world + rank) * self.cmax
        return b, b + self.cmax


class KernelTimer:
    """a pair of HIP events that bdf_ctx_time_next_rows attaches to the next row-kernel dispatch (the kernel's own begin and
    end on its stream; events recorded around the launch would add their marker packets to the interval)"""

    def __init__(self):
        self.start, self.stop = C.c_void_p(), C.c_void_p()
        check(lib().bdf_event_create(C.byref(self.start)))
        check(lib().bdf_event_create(C.byref(self.stop)))

    def elapsed_us(self):
        us = C.c_double(0.0)
        check(lib().bdf_event_elapsed_us(self.start, self.stop, C.byref(us)))
        return us.value

    def __del__(self):
        try:
            lib().bdf_event_destroy(self.start)
            lib().bdf_event_destroy(self.stop)
        except Exception:
            pass


class Context:
    """bdf_ctx bound to a torch device and torch's current stream."""

    def __init__(self, device=None, seed=0, stream=None):
        if not torch.cuda.is_available():
            raise _lib.NoGpuError("no GPU visible: bayesiandatafusion.jl_amd has no CPU path (the reference is the CPU path)")
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
        torch.cuda.set_device(self.device)
        self.stream = stream if stream is not None else torch.cuda.current_stream(self.device)
        self.handle = C.c_void_p()
        check(lib().bdf_ctx_create(self.device.index, C.c_void_p(self.stream.cuda_stream), C.c_uint64(int(seed) & (2 ** 64 - 1)),
                                   C.byref(self.handle)))
        self.seed = int(seed)
        # device objects created on this context; they are destroyed before it whatever order the garbage collector
        # finalises things in (a relation / feature handle points back into the context)
        self._children = weakref.WeakSet()

    @classmethod
    def wrap(cls, handle, device, seed, owned=False):
        """a context created by the library (bdf_ctx_create_rows, bdf_gibbs_contexts): the stream is the library's"""
        self = cls.__new__(cls)
        self.device = device
        self.handle = C.c_void_p(handle) if not isinstance(handle, C.c_void_p) else handle
        st = C.c_void_p()
        check(lib().bdf_ctx_stream(self.handle, C.byref(st)))
        self.stream = torch.cuda.ExternalStream(st.value or 0, device=device)
        self.seed = int(seed)
        self._children = weakref.WeakSet()
        self._owned = owned
        return self

    @classmethod
    def rows(cls, device, seed, reserve_cus=0):
        """a row context on a library-owned stream that keeps `reserve_cus` CUs free for a side context (bdf_ctx_create_rows)"""
        if not torch.cuda.is_available():
            raise _lib.NoGpuError("no GPU visible: bayesiandatafusion.jl_amd has no CPU path (the reference is the CPU path)")
        dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
        torch.cuda.set_device(dev)
        h = C.c_void_p()
        check(lib().bdf_ctx_create_rows(dev.index, C.c_uint64(int(seed) & (2 ** 64 - 1)), int(reserve_cus), C.byref(h)))
        return cls.wrap(h, dev, seed, owned=True)

    def adopt(self, child):
        self._children.add(child)

    def item_size(self):
        """the most observations one work item of the wave-per-row kernel takes on this context (bdf_ctx_item_size)"""
        out = C.c_int(0)
        check(lib().bdf_ctx_item_size(self.handle, C.byref(out)))
        return out.value

    def set_item_size(self, observations):
        check(lib().bdf_ctx_set_item_size(self.handle, int(observations)))

    def set_nonneg_chunk(self, rows):
        """rows per chunk of the non-negative prior's launches (bdf_ctx_set_nonneg_chunk); 0: the default"""
        check(lib().bdf_ctx_set_nonneg_chunk(self.handle, int(rows)))

    def rows_unfinished(self):
        """parity hook: split rows left unfinished by the row-kernel launches so far (must be 0)"""
        n = C.c_int64(0)
        check(lib().bdf_rows_unfinished(self.handle, C.byref(n)))
        return n.value

    def set_small_rows(self, max_observations, min_rows):
        """D <= 16: rows of at most max_observations observations four to a wave when the entity has min_rows rows or more
        (bdf_ctx_set_small_rows; 0 observations: off)"""
        check(lib().bdf_ctx_set_small_rows(self.handle, int(max_observations), int(min_rows)))

    def set_lowrank(self, max_observations=-1, min_rows=8192):
        """D > 16: rows of at most max_observations observations (-1: D / 2 up to 16, up to 32 at D > 32; 0: off) by the low-rank sampler when a
        launch has min_rows such rows or more (bdf_ctx_set_lowrank) -- the same conditional distribution as the reference's
        map, other sampled values"""
        check(lib().bdf_ctx_set_lowrank(self.handle, int(max_observations), int(min_rows)))

    def set_col_rows(self, max_piece=-1):
        """16 < D <= 32, one two-mode relation: the rows four to a wave in the column layout, cut into pieces of at most max_piece
        observations (bdf_ctx_set_col_rows; 0: off -- the wave-per-row kernel; -1: the default, 128 unless the caller chose an item size)"""
        check(lib().bdf_ctx_set_col_rows(self.handle, int(max_piece)))

    def rows_dispatch(self, entity_tag):
        """how the latest row launch under entity_tag was dispatched on this context (bdf_ctx_rows_dispatch): a dict of rows by
        the low-rank sampler, k_rows_small, K1c and k_rows, k_rows' work items and K1c's waves; None before the first launch"""
        out = (C.c_int64 * 6)()
        if lib().bdf_ctx_rows_dispatch(self.handle, int(entity_tag), out) != 0:
            return None
        return dict(zip(("lowrank", "small", "col", "k1", "k1_items", "col_waves"), (int(x) for x in out)))

    def set_gather_image(self, on=1):
        """K1c at D = 32 gathers from the opposite sample's gather image (bdf_ctx_set_gather_image): 1 on (the default: the pair image),
        0 off -- the values are the same either way; 2: the full image, the tier that was measured against it and lost"""
        check(lib().bdf_ctx_set_gather_image(self.handle, int(on)))

    def gather_image_stats(self):
        """K1c launches of this context that gathered from an image, images packed from a sample, launches that left their entity's
        image (bdf_ctx_gather_image_stats)"""
        out = (C.c_int64 * 3)()
        check(lib().bdf_ctx_gather_image_stats(self.handle, out))
        return dict(zip(("launches", "packs", "left"), (int(x) for x in out)))

    def gather_image_read(self, sample, tier_doubles=32):
        """parity hook: the image the context holds of the device tensor `sample` (rows x 32), as a numpy array rows x 16 x
        (tier_doubles / 16) (bdf_ctx_gather_image_read)"""
        out = np.empty((sample.shape[0], 16, tier_doubles // 16), dtype=np.float64)
        check(lib().bdf_ctx_gather_image_read(self.handle, _ptr(sample), int(sample.shape[0]), out.ctypes.data_as(C.c_void_p)))
        return out

    def gather_image_pack(self, sample, tier_doubles=32):
        """parity hook: the pack kernel's image of the device tensor `sample` (rows x 32), as a device tensor (bdf_gather_image_pack)"""
        img = self.zeros(sample.shape[0], 16, tier_doubles // 16)
        check(lib().bdf_gather_image_pack(self.handle, _ptr(sample), int(sample.shape[0]), _ptr(img)))
        return img

    def set_piece_size(self, observations):
        check(lib().bdf_ctx_set_piece_size(self.handle, int(observations)))

    def set_gather(self, mode):
        """parity hook: 0 auto, 1 general gather path, 2 lean path with 64-bit row offsets (num_latent > 32)"""
        check(lib().bdf_ctx_set_gather(self.handle, int(mode)))

    def set_sweep(self, i):
        check(lib().bdf_ctx_set_sweep(self.handle, C.c_uint32(int(i))))

    def advance_sweep(self):
        check(lib().bdf_ctx_advance_sweep(self.handle))

    def sync(self):
        check(lib().bdf_ctx_sync(self.handle))
        bits = C.c_uint32(0)
        check(lib().bdf_ctx_warnings(self.handle, C.byref(bits)))
        if bits.value & 64:          # BDF_WARN_CG_MAXITER: the reference returns such a column silently (parallel_cg.jl:73-93)
            import warnings
            warnings.warn("beta update: a conjugate-gradient column was still above its tolerance after maxiter iterations",
                          RuntimeWarning, stacklevel=2)

    def zeros(self, *shape, dtype=torch.float64):
        with torch.cuda.stream(self.stream):          # filled on the stream that will use it
            return torch.zeros(*shape, dtype=dtype, device=self.device)

    def tensor(self, a, dtype=torch.float64):
        with torch.cuda.stream(self.stream):
            return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(self.device)

    def close(self):
        if self.handle:
            for ch in list(self._children):
                ch.close()
            if getattr(self, "_owned", True):      # (contexts of a bdf_gibbs object are destroyed with it)
                lib().bdf_ctx_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceRelation(_DeviceObject):
    """bdf_rel: Relation.data (IndexedDF) as per-mode CSR in HBM."""
    _destroy = "bdf_relation_destroy"

    def __init__(self, ctx, idf, layouts=None, rank=0, values=None):
        """layouts: one Layout per mode (several ranks): the device then holds this rank's rows only, at internal positions;
        values: what the row kernels read in place of idf.values (a background relation with unit weights, _background_values)"""
        self.ctx = ctx
        self.handle = C.c_void_p()
        dims = np.asarray(idf.dims, dtype=np.int64)
        vals = np.ascontiguousarray(idf.values if values is None else values, dtype=np.float64)
        ids = idf.ids
        if layouts is None or all(l.pos is None for l in layouts):
            check(lib().bdf_relation_create(ctx.handle, len(idf.dims), dims.ctypes.data_as(_lib.c_i64p), idf.nnz(),
                                            ids.ctypes.data_as(C.c_void_p), ids.dtype.itemsize, vals.ctypes.data_as(_lib.c_dp),
                                            C.byref(self.handle)))
        else:
            pos = (_lib.c_i32p * len(layouts))(*[l.pos.ctypes.data_as(_lib.c_i32p) for l in layouts])
            cmax = np.asarray([l.cmax for l in layouts], dtype=np.int64)
            check(lib().bdf_relation_create_sharded(ctx.handle, len(idf.dims), dims.ctypes.data_as(_lib.c_i64p), idf.nnz(),
                                                    ids.ctypes.data_as(C.c_void_p), ids.dtype.itemsize, vals.ctypes.data_as(_lib.c_dp),
                                                    pos, cmax.ctypes.data_as(_lib.c_i64p), rank, layouts[0].world,
                                                    layouts[0].chunks, C.byref(self.handle)))
        self.dims = list(idf.dims)
        self.nnz = idf.nnz()
        # the relation's model on the device (GibbsEngine._build_model fills it; a bare relation has none)
        self.kind, self.alpha_sample, self.alpha_dev = "gauss", False, None
        self.F = self.beta = self.F_test = self.test_baseline = None     # relation-level side information
        self.train = None            # the training table as DevicePairs
        self.linear = None           # linear_values of the row kernels: mean + F beta, or what the model's latent draw leaves
        self.censor = self.interval = self.ordinal = self.ord_codes = None
        self.omega = None          # obs_precision of the row kernels
        self.robust_nu, self.pg_model, self.pg_r = 0.0, 0, 0.0
        # a noise precision per row of one entity (setEntityNoise): {"mode", "shape", "rate"}; tau per row of that mode
        self.noise = self.tau = None
        # biases (setBias): {mode0: {"shape", "rate"}}; per biased mode its bias vector (dims[mode0]); the modes' lambda, one double
        # each in rising mode order; the draw's residual scratch
        self.bias_spec = self.bias = self.bias_lambda = self.bias_resid = None
        # background cells (setBackground): {"weight", "value"}; the caller's weights (omega is then what the rows read, omega_k - c0)
        self.bg = self.bg_weights = None
        # a dense relation (setDense): {"R": N x M, the values without their mean; "C": per mode, its rows of R V / R' U; "sum_r2":
        # the sum of r^2}.  The handle is then a relation WITHOUT cells
        self.dense = None
        # either of the two is folded into its entities' priors: per mode, D + D^2 doubles of bdf_hyper_sums (the rows' sum and Gram matrix)
        self.fold_sums = None
        ctx.adopt(self)

    @property
    def has_model(self):
        """a model of its own -- alpha sampled, relation-level side information, a noise model other than fixed-precision
        Gaussian noise: registered with the library's iteration, which steps it before the rows of every iteration"""
        return (self.alpha_sample or self.F is not None or self.kind != "gauss" or self.bg is not None or self.dense is not None
                or self.bias is not None)

    def index(self, mode0):
        rp, ri = _lib.c_i64p(), _lib.c_i64p()
        check(lib().bdf_relation_index(self.handle, mode0, C.byref(rp), C.byref(ri)))
        return (np.ctypeslib.as_array(rp, shape=(self.dims[mode0] + 1,)).copy(),
                np.ctypeslib.as_array(ri, shape=(max(self.nnz, 1),))[:self.nnz].copy())

    def value_mean(self):
        m = C.c_double()
        check(lib().bdf_relation_value_mean(self.handle, C.byref(m)))
        return m.value

    def order(self, mode0):
        out = np.zeros(self.dims[mode0], dtype=np.int32)
        check(lib().bdf_relation_order(self.handle, mode0, out.ctypes.data_as(_lib.c_i32p)))
        return out



class DevicePairs(_DeviceObject):
    """bdf_pairs: test_vec (or the training table) with its running prediction state."""
    _destroy = "bdf_pairs_destroy"

    def __init__(self, ctx, ids, values):
        self.ctx = ctx
        self.handle = C.c_void_p()
        ids = np.asfortranarray(np.asarray(ids, dtype=np.int64))
        values = np.ascontiguousarray(values, dtype=np.float64)
        self.n, self.n_modes = ids.shape
        check(lib().bdf_pairs_create(ctx.handle, self.n_modes, self.n, ids.ctypes.data_as(C.c_void_p), 8,
                                     values.ctypes.data_as(_lib.c_dp), C.byref(self.handle)))
        # the reporting step's device scalars, read back together: bdf_predict_update's 4 stats, then roc_avg (auc), then
        # bdf_pairs_lpd_update's 4 (lpd_update)
        self.report = ctx.zeros(9)
        self.stats = self.report[:4]
        self.lpd_stats = self.report[5:]
        self.waic_stats = None         # bdf_pairs_waic_update's 4, a tensor of its own at first use (waic_update)
        self._order = None
        ctx.adopt(self)

    def sort(self, mode0=0):
        """store the pairs sorted by their id in mode `mode0` (neighbouring pairs share that factor row); results keep the
        caller's order"""
        check(lib().bdf_pairs_sort(self.handle, int(mode0)))
        self._order = np.zeros(self.n, dtype=np.int64)
        check(lib().bdf_pairs_order(self.handle, self._order.ctypes.data_as(_lib.c_i64p)))
        return self

    def set_link(self, link):
        """0: predictions are udot + base (the default); 1: the probit link, probabilities Phi(udot + base) (bdf_pairs_set_link)"""
        check(lib().bdf_pairs_set_link(self.handle, int(link)))
        return self

    def set_precision_scale(self, tau, mode0=0):
        """lpd_update scores pair k with alpha tau[its id in mode mode0] (bdf_pairs_set_precision_scale): tau, a device tensor with one
        double per row of that mode, is read at every update (the per-row noise model's draw); None clears it"""
        check(lib().bdf_pairs_set_precision_scale(self.handle, _ptr(tau), int(mode0)))
        self._scale = tau                # (borrowed by the library: keep it alive)
        return self

    def set_pg_link(self, model, r=0.0):
        """the links of the Polya-Gamma models: model 1, the logistic probability 1 / (1 + exp(-(udot + base))) (bdf_pairs_set_logistic_link);
        model 2, the counts' mean r exp(udot + base) (bdf_pairs_set_count_link)"""
        if int(model) == 1:
            check(lib().bdf_pairs_set_logistic_link(self.handle))
        else:
            check(lib().bdf_pairs_set_count_link(self.handle, float(r)))
        return self

    def _on_own_stream(self):
        """the pairs' stream ordered after the caller's current stream (where the factors were produced), as a context
        manager under which torch allocates and fills on the pairs' stream"""
        cur = torch.cuda.current_stream(self.ctx.device)
        if cur != self.ctx.stream:
            self.ctx.stream.wait_stream(cur)
        return cur, torch.cuda.stream(self.ctx.stream)

    def _hand_back(self, cur, *tensors):
        """results written on the pairs' stream become visible to the caller's stream (a later .cpu() / kernel there)"""
        if cur != self.ctx.stream:
            cur.wait_stream(self.ctx.stream)
            for t in tensors:
                t.record_stream(cur)

    def predict(self, D, factors, mean_value):
        # the pairs of an engine live on its prediction stream (engine.test_pairs): `out` is allocated, zero-filled and
        # written there, and the caller's stream waits for it -- a plain ctx.zeros() here raced the side-stream kernel
        # against a null-stream fill and read-back (round-1 smoke)
        cur, own = self._on_own_stream()
        with own:
            out = torch.zeros(self.n, dtype=torch.float64, device=self.ctx.device)
            check(lib().bdf_predict(self.ctx.handle, self.handle, D, _facs(factors), mean_value, _ptr(out)))
        self._hand_back(cur, out)
        return out

    def sse(self, D, factors, mean_value, linear=None):
        """device scalar (stats[1]): sum of (value - pred)^2, pred = udot + (linear | mean_value)"""
        check(lib().bdf_predict_sse(self.ctx.handle, self.handle, D, _facs(factors), mean_value,
                                    _ptr(linear) if linear is not None else None, _ptr(self.stats)))
        return self.stats

    def update(self, D, factors, mean_value, phase, clamp, class_cut):
        lo, hi = (clamp[0], clamp[1]) if len(clamp) else (1.0, -1.0)
        check(lib().bdf_predict_update(self.ctx.handle, self.handle, D, _facs(factors), mean_value, phase, lo, hi,
                                       class_cut, _ptr(self.stats)))
        return self.stats

    def auc(self, class_cut, ctx=None, counts=None):
        """roc_avg of macau.jl:200, AUC_ROC(values .< class_cut, -avg) over the running average in the caller's order
        (bdf_pairs_auc), as a device scalar (report[4]).  ctx: the context whose stream ran the prediction update (default: the
        pairs' own); counts: nullable int64 device tensor of 3 that receives {C, P, Nn}"""
        ctx = ctx or self.ctx
        check(lib().bdf_pairs_auc(ctx.handle, self.handle, float(class_cut), C.c_void_p(self.report.data_ptr() + 32),
                                  _ptr(counts)))
        return self.report[4]

    def lpd_update(self, D, factors, mean_value, alpha, phase, bounds=None):
        """one scoring step of the held-out log predictive density (bdf_pairs_lpd_update) on the pairs' own stream: every pair's
        log-likelihood under `factors` -- probit pairs (set_link(1)) as 0/1 values, pairs whose `bounds` (device (n, 2) tensor in
        the caller's order, or None) differ by their interval's mass, the others by the Gaussian density at their value -- folded
        into the running log-sum-exp (phase 0: burn-in, nothing kept; 1: first posterior draw; 2: later ones).  alpha: a float,
        or a device scalar (tensor of one double) read on the device.  Returns the device statistics: [0] the sum of this
        draw's log-likelihoods, [1] the sum of the pairs' lpd after it, [2] = [3] = 0."""
        check(lib().bdf_pairs_lpd_update(self.ctx.handle, self.handle, _ptr(bounds) if bounds is not None else None, D, _facs(factors),
                                         mean_value, *_alpha_args(alpha), int(phase), _ptr(self.lpd_stats)))
        return self.lpd_stats

    def lpd(self):
        """the pairs' lpd over the posterior draws scored so far, as a host array in the caller's order (bdf_pairs_lpd maps the
        state, kept in storage order like state()'s, through the pairs' order on the device)"""
        cur, own = self._on_own_stream()
        with own:
            out = torch.zeros(self.n, dtype=torch.float64, device=self.ctx.device)
            check(lib().bdf_pairs_lpd(self.ctx.handle, self.handle, _ptr(out)))
        self._hand_back(cur, out)
        return out.cpu().numpy()

    def waic_update(self, D, factors, mean_value, alpha, phase, bounds=None):
        """one scoring step of WAIC (bdf_pairs_waic_update) on the pairs' own stream: every pair's log-likelihood as lpd_update
        forms it (with `bounds` the pairs' baseline is not read: m = udot + mean_value), folded into the running log-sum-exp and
        Welford's mean and M2 of it.  Returns the device statistics (waic_stats): [0] the sum of this draw's log-likelihoods, [1]
        the sum of the pairs' lppd after it, [2] the sum of their V (the variance of the log-likelihood over the draws), [3] the
        number of pairs with V > 0.4."""
        if self.waic_stats is None:
            self.waic_stats = self.ctx.zeros(4)
        check(lib().bdf_pairs_waic_update(self.ctx.handle, self.handle, _ptr(bounds) if bounds is not None else None, D, _facs(factors),
                                          mean_value, *_alpha_args(alpha), int(phase), _ptr(self.waic_stats)))
        return self.waic_stats

    def waic(self, pointwise=False):
        """the end of the run (bdf_pairs_waic): the host array {sum lppd, sum V, sum (elpd - mean elpd)^2, the count of V > 0.4}
        and, with `pointwise`, the (n, 2) host array of every pair's (lppd, V) in the caller's order (otherwise None)"""
        cur, own = self._on_own_stream()
        with own:
            stats = torch.zeros(4, dtype=torch.float64, device=self.ctx.device)
            out = torch.zeros((self.n, 2), dtype=torch.float64, device=self.ctx.device) if pointwise else None
            check(lib().bdf_pairs_waic(self.ctx.handle, self.handle, _ptr(out) if (pointwise and self.n) else None, _ptr(stats)))
        self._hand_back(cur, *([stats] + ([out] if pointwise else [])))
        return stats.cpu().numpy(), (out.cpu().numpy() if pointwise else None)

    def state(self):
        """(avg, sq) as host arrays"""
        a, s, n = C.c_void_p(), C.c_void_p(), C.c_int64()
        check(lib().bdf_pairs_state(self.handle, C.byref(a), C.byref(s), C.byref(n)))
        avg, sq = np.zeros(n.value), np.zeros(n.value)
        if n.value:
            check(lib().bdf_d2h(self.ctx.handle, avg.ctypes.data_as(C.c_void_p), a, n.value * 8))
            check(lib().bdf_d2h(self.ctx.handle, sq.ctypes.data_as(C.c_void_p), s, n.value * 8))
        if self._order is not None:             # storage order -> the caller's order
            a2, s2 = np.empty_like(avg), np.empty_like(sq)
            a2[self._order], s2[self._order] = avg, sq
            avg, sq = a2, s2
        return avg, sq



_AUC_CONTEXTS = {}          # (device, stream) -> Context of device_auc_roc


class _DrawRing(_DeviceObject):
    """what DeviceScores and DeviceAcquire share: planes of n_rows x M doubles over the scored rows of a two-mode relation's first
    entity against all M rows of its second, and a ring of posterior draws that are not in the planes yet.  `_lib_name`: the
    prefix of the object's entry points.  Everything runs on ctx's stream."""

    def _create(self, ctx, n_rows, M, D, batch, rows0, *model):
        """rows0: None, the rows 0 .. n_rows - 1 of U; else the 0-based row of U of every scored row"""
        self.ctx, self.handle, self._destroy = ctx, C.c_void_p(), self._lib_name + "_destroy"
        self.n_rows, self.M, self.D, self.batch = int(n_rows), int(M), int(D), int(batch)
        rows = ctx.tensor(np.asarray(rows0, dtype=np.int32), dtype=torch.int32) if rows0 is not None else None
        check(self._call("create")(ctx.handle, self.n_rows, self.M, self.D, self.batch, _ptr(rows), *model, C.byref(self.handle)))
        ctx.adopt(self)

    def _call(self, name):
        return getattr(lib(), f"{self._lib_name}_{name}")

    def flush(self):
        check(self._call("flush")(self.handle))

    def read(self, first=0, count=None, *plane):
        """parity hook: `count` doubles of the sum (a plane) from cell `first` (behind the n_rows M cells: 64 guard doubles), flushed first"""
        count = self.n_rows * self.M - first if count is None else int(count)
        out = self.ctx.zeros(count)
        check(self._call("copy")(self.handle, *plane, _ptr(out), int(first), count, 0))
        return out

    def write(self, values, draws, *plane):
        """parity hook: the sum's (a plane's) cells from a device tensor and, unless None, the count of draws the planes then stand for"""
        check(self._call("copy")(self.handle, *plane, _ptr(values), 0, int(values.numel()), 1))
        if draws is not None:
            check(self._call("set_draws")(self.handle, float(draws)))


class DeviceScores(_DrawRing):
    """bdf_scores: the sum of u.v over the posterior draws (n_rows x M doubles on the device), a ring of draws that are not in the
    sum yet, and the top-K lists and ranking metrics from it (setRecommend; csrc/k_recommend.hip)."""
    _lib_name = "bdf_scores"

    def __init__(self, ctx, n_rows, M, D, batch, rows0=None):
        self._create(ctx, n_rows, M, D, batch, rows0)

    def push(self, U, V):
        """this draw's factors (N x D and M x D tensors) into the ring; a full ring is added into the sum (bdf_scores_push)"""
        check(lib().bdf_scores_push(self.handle, _ptr(U), _ptr(V)))

    def topk(self, K, mean_value, rel=None):
        """(items int32 n_rows x K, 1-based and 0 behind the last candidate; scores float64, NaN there) on the device; rel: the
        DeviceRelation whose listed cells are left out of every row's list"""
        K = int(K)
        items = self.ctx.zeros(self.n_rows, K, dtype=torch.int32)
        scores = self.ctx.zeros(self.n_rows, K)
        check(lib().bdf_scores_topk(self.handle, rel.handle if rel is not None else None, K, float(mean_value), _ptr(items), _ptr(scores)))
        return items, scores

    def metrics(self, items, K, pairs, class_cut):
        """the device tensor {recall@K, NDCG@K, hit rate, rows scored} of the lists `items` on the test cells `pairs`"""
        out = self.ctx.zeros(4)
        check(lib().bdf_scores_metrics(self.handle, _ptr(items), int(K), pairs.handle, float(class_cut), _ptr(out)))
        return out


ACQUIRE_RULES = {"ucb": 0, "sd": 1, "prob_above": 2}        # BDF_ACQ_UCB, _SD, _PROB (csrc/acquire.h)
ACQUIRE_PLANES = {"mean": 0, "M2": 1, "psum": 2, "score": 3}


class DeviceAcquire(_DrawRing):
    """bdf_acquire: the running mean and sum of squared deviations of u.v over the posterior draws and, with a threshold, the sum of
    the draws' exceedance probabilities (n_rows x M doubles each on the device), a ring of draws that are not in the planes yet, and
    the top-K lists by an acquisition score from them (setAcquire; csrc/k_acquire.hip)."""
    _lib_name = "bdf_acquire"

    def __init__(self, ctx, n_rows, M, D, batch, rows0=None, mean_value=0.0, threshold=None):
        """threshold: None keeps no psum plane"""
        self.want_prob = threshold is not None
        self._create(ctx, n_rows, M, D, batch, rows0, int(self.want_prob), float(mean_value), float(threshold) if self.want_prob else 0.0)

    def push(self, U, V, alpha):
        """this draw's factors (N x D and M x D tensors) and its precision into the ring; alpha: a float, or a device tensor of
        one double that only the device reads.  A full ring is folded into the planes (bdf_acquire_push)"""
        check(lib().bdf_acquire_push(self.handle, _ptr(U), _ptr(V), *_alpha_args(alpha, 1.0)))

    def topk(self, K, rule, kappa=0.0, rel=None):
        """{"items" (int32 n_rows x K, 1-based and 0 behind the last candidate), "scores", "mean", "sd" and, with a psum plane,
        "prob" (float64, NaN there)} on the device; rel: the DeviceRelation whose listed cells are left out of every row's list"""
        K = int(K)
        out = {"items": self.ctx.zeros(self.n_rows, K, dtype=torch.int32)}
        for k in ("scores", "mean", "sd") + (("prob",) if self.want_prob else ()):
            out[k] = self.ctx.zeros(self.n_rows, K)
        check(lib().bdf_acquire_topk(self.handle, rel.handle if rel is not None else None, K, ACQUIRE_RULES[rule], float(kappa), _ptr(out["items"]),
                                     _ptr(out["scores"]), _ptr(out["mean"]), _ptr(out["sd"]), _ptr(out.get("prob"))))
        return out

    def read(self, plane, first=0, count=None):
        """parity hook: `count` doubles of plane "mean", "M2", "psum" or "score" from cell `first`"""
        return super().read(first, count, ACQUIRE_PLANES[plane])

    def write(self, planes, draws):
        """parity hook: the cells of the planes {name: device tensor}, and the count of draws they stand for"""
        for name, values in planes.items():
            super().write(values, None, ACQUIRE_PLANES[name])
        check(lib().bdf_acquire_set_draws(self.handle, float(draws)))


DIAG_STATS = ("max_rhat", "min_ess", "n_rhat_high", "n_ess_low", "n_constant", "n_draws")      # stats_out of bdf_diag_compute, then 3 per scalar


class DeviceDiag(_DeviceObject):
    """bdf_diag: every pushed draw of the predictions of a set of pairs, and of n_scalars scalars beside them (the draw's sum of squared
    errors, its alpha), in one plane of capacity x (n_cells + n_scalars) doubles on the device, draw-major with the cells in the
    pairs' storage order; and the split R-hat, effective sample size and Monte Carlo standard error of every series down its columns
    (setDiagnostics; csrc/k_diag.hip).  Everything runs on ctx's stream."""
    _destroy = "bdf_diag_destroy"

    def __init__(self, ctx, n_cells, n_scalars, capacity):
        self.ctx, self.handle = ctx, C.c_void_p()
        self.n_cells, self.n_scalars, self.capacity = int(n_cells), int(n_scalars), int(capacity)
        check(lib().bdf_diag_create(ctx.handle, self.n_cells, self.n_scalars, self.capacity, C.byref(self.handle)))
        ctx.adopt(self)

    def push(self, pairs, D, factors, mean_value, alpha=1.0):
        """this draw into the next row: the pairs' predictions as pairs.predict forms them, the sum of their squared errors and, with
        two scalars, alpha -- a float, or a device tensor of one double that only the device reads (bdf_diag_push)"""
        check(lib().bdf_diag_push(self.ctx.handle, self.handle, pairs.handle, int(D), _facs(factors), float(mean_value), *_alpha_args(alpha, 1.0)))

    def write(self, draw, values):
        """parity hook: row `draw` of the plane from a device tensor of n_cells + n_scalars doubles"""
        check(lib().bdf_diag_write(self.handle, int(draw), _ptr(values)))

    def plane(self):
        """parity hook: the draws held, as a host array (draws, n_cells + n_scalars) with the cells in the pairs' storage order"""
        p, n = C.c_void_p(), C.c_int64()
        check(lib().bdf_diag_plane(self.handle, C.byref(p), C.byref(n)))
        out = np.zeros((n.value, self.n_cells + self.n_scalars))
        if n.value:
            check(lib().bdf_d2h(self.ctx.handle, out.ctypes.data_as(C.c_void_p), p, out.nbytes))
        return out

    def compute(self, rhat_cut, ess_cut, pointwise=False, order=None):
        """(stats, out) on the device (bdf_diag_compute): stats = DIAG_STATS, then (rhat, ess, mcse) per scalar; out, with `pointwise`,
        the (n_cells, 3) tensor of every cell's (rhat, ess, mcse) at the caller's index order[storage position] (a host array, or None
        for the storage order itself), else None"""
        stats = self.ctx.zeros(len(DIAG_STATS) + 3 * self.n_scalars)
        out = self.ctx.zeros(self.n_cells, 3) if pointwise else None
        orig = self.ctx.tensor(np.asarray(order, dtype=np.int32), dtype=torch.int32) if (pointwise and order is not None) else None
        check(lib().bdf_diag_compute(self.ctx.handle, self.handle, _ptr(orig), float(rhat_cut), float(ess_cut), _ptr(out), _ptr(stats)))
        return stats, out


class DeviceNewRows:
    """Cells of rows that were not in training (setNewRows / setNewTest; csrc/k_newrows.hip): the operator of
    the new rows' features, their cells as pairs whose first mode indexes the new rows, and the buffers of the three launches that
    follow every iteration on the row stream -- uhat of the new rows (bdf_uhat), q per row of the other entity (bdf_newrows_quad),
    the update of the cells' running state (bdf_newrows_update).  With known cells of the new rows (setNewObserved; csrc/k_foldin.hip,
    DESIGN.md section 29) it also holds their relation, n* x M, and the (m, q) planes, and the launches are bdf_uhat for an entity with
    features, bdf_foldin_cells -- the systems by the row sampler's accumulation into the context's scratch, then a workgroup of four
    waves per new row -- and bdf_newrows_update_cells.  Nothing of a draw comes to the host."""

    def __init__(self, eng, r):
        spec = r.model.new_test
        mode0 = spec["mode"] - 1
        self.eng, self.rel, self.mode0 = eng, r, mode0
        ctx = self.ctx = eng.ctx
        self.st = eng.ent[eng._entity_index(r.entities[mode0])]          # the entity with new rows
        self.so = eng.ent[eng._entity_index(r.entities[1 - mode0])]      # the other one: V
        D = self.D = eng.D
        known = r.model.new_observed
        self.foldin = known is not None
        F_new = r.entities[mode0].new_rows
        self.F = FeatOperator(ctx, F_new) if F_new is not None else None
        self.n_rows = self.F.m if self.F is not None else int(known["n_rows"])
        ids, vals = spec["ids"], spec["values"]
        # (the new row's id first, whichever of the relation's columns holds it; stored sorted by the existing row: neighbours share
        # v_j and q_j -- or, with known cells, by the new row: a row's cells are one workgroup's, bdf_foldin_cells)
        self.pairs = DevicePairs(ctx, np.stack([ids[:, mode0], ids[:, 1 - mode0]], axis=1).reshape(-1, 2), vals)
        if self.pairs.n:
            self.pairs.sort(0 if self.foldin else 1)
        if r.model.probit:
            self.pairs.set_link(1)
        self.known = self.term = self.m = self.qc = self.n_known = None
        if self.foldin:
            # the known cells as a relation of their own, n* x M, whose first mode the row sampler's accumulation takes for (P_i, b_i);
            # the systems live in the context's scratch, a chunk at a time; (m, q) per cell between the two launches
            kid = known["ids"]
            self.known = DeviceRelation(ctx, IndexedDF((np.stack([kid[:, mode0], kid[:, 1 - mode0]], axis=1).reshape(-1, 2), known["values"]),
                                                       dims=[self.n_rows, self.so.N]))
            self.term = Term()
            self.term.rel, self.term.mode, self.term.mean_value = self.known.handle, 0, float(r.model.mean_value)
            self.m, self.qc = ctx.zeros(max(self.pairs.n, 1)), ctx.zeros(max(self.pairs.n, 1))
            self.n_known = np.bincount(kid[:, mode0] - 1, minlength=self.n_rows).astype(np.int64)
        self.uhat = ctx.zeros(self.n_rows, D)
        self.factors = ctx.zeros(self.n_rows, D)           # mu + uhat: what the cells are predicted from
        self.q = ctx.zeros(max(self.so.N, 1)) if not self.foldin else None       # q_j per row of V: the cold path's
        self.report = ctx.zeros(10)                        # bdf_newrows_update's 8, then the ROC of the running mean
        self.draws = 0
        # the cells with a value, in the caller's order: what the ROC ranks
        has = ~np.isnan(vals)
        self.n_scored = int(has.sum())
        self._has = ctx.tensor(np.nonzero(has)[0], dtype=torch.int64)
        self._labels = ctx.tensor((vals[has] < r.class_cut).astype(np.uint8), dtype=torch.uint8)
        self._auc_ws = torch.empty(max(1, lib().bdf_auc_workspace_bytes(self.n_scored)), dtype=torch.uint8, device=ctx.device)
        self._out = ctx.zeros(max(self.pairs.n, 1), 3)

    def step(self, phase, clamp, class_cut, alpha, lpd):
        """the three launches behind iteration's last launch, on the row stream -> this draw's factors of the new rows.  They read beta
        and V (written on the row stream) and (mu, Lambda) of this iteration (the hyperprior stream: the row stream is already behind
        that draw, which beta's update waited for; the wait below says so again).  Everything that overwrites one of them in the next
        iteration is either on the row stream or waits for the next iteration's rows of this entity, which are enqueued on the row
        stream behind these launches."""
        eng, ctx, D, L = self.eng, self.ctx, self.D, lib()
        if eng.ctx_h is not ctx:
            ctx.stream.wait_stream(eng.ctx_h.stream)
        lo, hi = (clamp[0], clamp[1]) if len(clamp) else (1.0, -1.0)
        alpha_host, alpha_dev = _alpha_args(alpha)
        if self.F is not None:
            check(L.bdf_uhat(ctx.handle, self.F.handle, D, _ptr(self.st.beta), _ptr(self.st.mu), _ptr(self.uhat), _ptr(self.factors)))
        if self.foldin:
            # with known cells: the systems' launch reads V, Lambda, mu_i and alpha under the same stream order,
            # bdf_foldin_cells leaves uhat_i in `uhat` (over F_new beta, which `factors` = mu_i has taken in) and (m, q) per cell, and
            # the fold is bdf_newrows_update's on those planes
            t = self.term
            t.alpha, t.alpha_dev = _alpha_args(alpha, 1.0)
            t.factors[1] = self.so.sample.data_ptr()
            mu = self.factors if self.F is not None else self.st.mu
            check(L.bdf_foldin_cells(ctx.handle, D, self.n_rows, C.byref(t), _ptr(mu), int(self.F is not None), _ptr(self.st.Lambda),
                                     self.pairs.handle, float(self.rel.model.mean_value), _ptr(self.m), _ptr(self.qc), _ptr(self.uhat)))
            check(L.bdf_newrows_update_cells(ctx.handle, self.pairs.handle, _ptr(self.m), _ptr(self.qc), alpha_host, alpha_dev, int(phase),
                                             lo, hi, float(class_cut), int(bool(lpd)), _ptr(self.report)))
        else:
            check(L.bdf_newrows_quad(ctx.handle, D, self.so.N, _ptr(self.st.Lambda), _ptr(self.so.sample), _ptr(self.q)))
            check(L.bdf_newrows_update(ctx.handle, self.pairs.handle, D, _ptr(self.factors), _ptr(self.so.sample), _ptr(self.q),
                                       float(self.rel.model.mean_value), alpha_host, alpha_dev, int(phase),
                                       lo, hi, float(class_cut), int(bool(lpd)), _ptr(self.report)))
        if phase >= 1:                  # (the cells' running state holds one draw more)
            self.draws = 1 if phase == 1 else self.draws + 1
        return self.uhat if self.foldin else self.factors

    def auc(self):
        """AUC_ROC(values .< class_cut, -pred) over the cells with a value (bdf_auc_roc on the running mean, in the caller's order)
        into report[8], behind the update on the row stream; NaN before the first posterior draw"""
        ctx = self.ctx
        with torch.cuda.stream(ctx.stream):
            if self.draws < 1 or self.n_scored == 0:
                self.report[8] = float("nan")
                return
            check(lib().bdf_newrows_result(ctx.handle, self.pairs.handle, _ptr(self._out)))
            scores = (-self._out[:, 0]).index_select(0, self._has).contiguous()
            check(lib().bdf_auc_roc(ctx.handle, self.n_scored, _ptr(self._labels), _ptr(scores), _ptr(self._auc_ws),
                                    C.c_void_p(self.report.data_ptr() + 64), None))
            scores.record_stream(ctx.stream)

    def result(self):
        """(n, 3) host array of (pred, stdev, lpd) in the caller's order"""
        ctx = self.ctx
        with torch.cuda.stream(ctx.stream):
            if self.draws < 1:
                return np.full((self.pairs.n, 3), np.nan)
            if self.pairs.n:
                check(lib().bdf_newrows_result(ctx.handle, self.pairs.handle, _ptr(self._out)))
            return self._out[:self.pairs.n].cpu().numpy()

    def state(self):
        """parity hook: the running state as a (5, n) host array in STORAGE order -- mean, M2, sum q, M, A -- and the draws it holds"""
        st, draws = C.c_void_p(), C.c_double()
        check(lib().bdf_newrows_state(self.pairs.handle, C.byref(st), C.byref(draws)))
        out = np.zeros((5, self.pairs.n))
        if st.value and self.pairs.n:
            check(lib().bdf_d2h(self.ctx.handle, out.ctypes.data_as(C.c_void_p), st, out.size * 8))
        return out, draws.value

    def close(self):
        self.pairs.close()
        if self.F is not None:
            self.F.close()
        if self.known is not None:
            self.known.close()


def device_auc_roc(labels, scores):
    """AUC_ROC(labels, scores) (src/ROC.jl:1-11) of GPU tensors through bdf_auc_roc, on torch's current stream ->
    (auc, C, P, Nn): C the exact number of (negative, positive) pairs ranked in that order, P / Nn the class sizes"""
    if not (torch.is_tensor(scores) and scores.device.type == "cuda"):
        raise ArgumentError("device_auc_roc: scores must be a GPU tensor")
    dev = scores.device
    labels = torch.as_tensor(labels, device=dev)
    if scores.dtype != torch.float64:
        raise ArgumentError(f"AUC_ROC: scores must be float64 on the device, not {scores.dtype}")
    if labels.dtype not in (torch.bool, torch.uint8):
        raise ArgumentError(f"AUC_ROC: labels must be bool or uint8 on the device, not {labels.dtype}")
    if labels.device != dev or labels.numel() != scores.numel():
        raise _lib.DimensionMismatch(f"AUC_ROC: {labels.numel()} labels on {labels.device} for {scores.numel()} scores on {dev}")
    stream = torch.cuda.current_stream(dev)
    ctx = _AUC_CONTEXTS.get((dev.index, stream.cuda_stream))
    if ctx is None:
        with torch.cuda.device(dev):
            ctx = _AUC_CONTEXTS[(dev.index, stream.cuda_stream)] = Context(dev.index, stream=stream)
    labels = labels.reshape(-1).contiguous()
    labels = labels.view(torch.uint8) if labels.dtype == torch.bool else labels
    scores = scores.reshape(-1).contiguous()
    n = scores.numel()
    ws = torch.empty(max(1, lib().bdf_auc_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    res = torch.empty(4, dtype=torch.int64, device=dev)          # the auc's bits, then C, P, Nn: one read-back
    check(lib().bdf_auc_roc(ctx.handle, n, _ptr(labels), _ptr(scores), _ptr(ws), _ptr(res), C.c_void_p(res.data_ptr() + 8)))
    h = res.cpu().numpy()
    return float(h[:1].view(np.float64)[0]), int(h[1]), int(h[2]), int(h[3])


class FeatOperator(_DeviceObject):
    """bdf_feat: the Entity.F operator on the device (dense / CSR / binary)."""
    _destroy = "bdf_feat_destroy"

    def __init__(self, ctx, F, layout=None):
        """layout (several ranks): the rows of F move to the entity's internal positions (rows nobody owns are zero), and the
        original ids key the rows' noise streams (bdf_feat_set_row_ids)"""
        self.ctx = ctx
        self.handle = C.c_void_p()
        L = lib()
        self.m_orig = feat.feature_shape(F)[0]
        if layout is not None and layout.pos is not None:
            F = _rows_to_internal(F, layout)
        if isinstance(F, feat.SparseMatrixCSR):
            self.kind = "csr"
            check(L.bdf_feat_create_csr(ctx.handle, F.m, F.n, len(F.rows), F.rows.ctypes.data_as(_lib.c_i32p),
                                        F.cols.ctypes.data_as(_lib.c_i32p), F.vals.ctypes.data_as(_lib.c_dp), C.byref(self.handle)))
            self.m, self.n = F.m, F.n
        elif isinstance(F, feat.SparseBinMatrix):
            self.kind = "bin"
            check(L.bdf_feat_create_bin(ctx.handle, F.m, F.n, len(F.rows), F.rows.ctypes.data_as(_lib.c_i32p),
                                        F.cols.ctypes.data_as(_lib.c_i32p), C.byref(self.handle)))
            self.m, self.n = F.m, F.n
        elif hasattr(F, "tocoo"):
            coo = F.tocoo()
            rows = np.ascontiguousarray(coo.row + 1, dtype=np.int32)
            cols = np.ascontiguousarray(coo.col + 1, dtype=np.int32)
            vals = np.ascontiguousarray(coo.data, dtype=np.float64)
            self.kind = "csr"
            check(L.bdf_feat_create_csr(ctx.handle, coo.shape[0], coo.shape[1], len(rows), rows.ctypes.data_as(_lib.c_i32p),
                                        cols.ctypes.data_as(_lib.c_i32p), vals.ctypes.data_as(_lib.c_dp), C.byref(self.handle)))
            self.m, self.n = int(coo.shape[0]), int(coo.shape[1])
        else:
            A = np.asfortranarray(np.asarray(F, dtype=np.float64))
            if A.ndim != 2:
                raise ArgumentError("feature matrix must be two-dimensional")
            self.kind = "dense"
            check(L.bdf_feat_create_dense(ctx.handle, A.shape[0], A.shape[1], A.ctypes.data_as(_lib.c_dp), C.byref(self.handle)))
            self.m, self.n = int(A.shape[0]), int(A.shape[1])
        if layout is not None and layout.pos is not None:
            ids = np.full(layout.nint, -1, dtype=np.int32)
            ids[layout.pos] = np.arange(layout.N, dtype=np.int32)
            check(L.bdf_feat_set_row_ids(self.handle, ids.ctypes.data_as(_lib.c_i32p)))
        ctx.adopt(self)

    # B, out: torch tensors holding column-major matrices, i.e. shape (ncol, rows)
    def mul(self, B, transpose=False):
        ncol = B.shape[0]
        out = self.ctx.zeros(ncol, self.n if transpose else self.m)
        check(lib().bdf_feat_mul(self.ctx.handle, self.handle, _ptr(B), ncol, _ptr(out), int(transpose)))
        return out

    def AtA_mul(self, X, lam):
        out = self.ctx.zeros(X.shape[0], self.n)
        check(lib().bdf_feat_AtA_mul(self.ctx.handle, self.handle, _ptr(X), X.shape[0], float(lam), _ptr(out)))
        return out



def _dense_mean(r):
    """mean_value of a dense relation: the listed values added one after the other, as bdf_relation_create adds the explicit listing's"""
    v = np.asarray(r.data.values, dtype=np.float64)
    return float(np.cumsum(v)[-1]) / len(v) if len(v) else 0.0


def _background_values(r):
    """What the row kernels read as the values of a background relation (setBackground) whose listed cells all have weight 1:
    y' = mean + (r - c0 rb) / (1 - c0), with r = y - mean and rb = value - mean.  Beside the precision alpha (1 - c0) a listed cell
    then adds alpha (1 - c0) v v' and alpha (r - c0 rb) v, its own term less the background term the Gram matrix counts for it, on
    the unweighted kernels -- and y' takes as many distinct values as y, so a relation of ratings keeps its 8-bit value codes.
    None: no background, or one with setWeights (the weighted kernel reads obs_precision and linear_values instead)."""
    bg = r.model.background
    if bg is None or r.model.weights is not None:
        return None
    mean, c0 = background_mean(r), bg["weight"]
    y = np.asarray(r.data.values, dtype=np.float64)
    return mean + ((y - mean) - c0 * (bg["value"] - mean)) / (1.0 - c0)


def _rows_to_internal(F, layout):
    """F with row i moved to row layout.pos[i] of a layout.nint-row matrix of the same kind"""
    pos = layout.pos.astype(np.int64)
    if isinstance(F, feat.SparseMatrixCSR):
        return feat.SparseMatrixCSR(pos[F.rows - 1] + 1, F.cols, F.vals, layout.nint, F.n)
    if isinstance(F, feat.SparseBinMatrix):
        return feat.SparseBinMatrix(layout.nint, F.n, pos[F.rows - 1] + 1, F.cols)
    if hasattr(F, "tocoo"):
        import scipy.sparse as sp
        coo = F.tocoo()
        return sp.csr_matrix((coo.data, (pos[coo.row], coo.col)), shape=(layout.nint, coo.shape[1]))
    A = np.asarray(F, dtype=np.float64)
    out = np.zeros((layout.nint, A.shape[1]))
    out[pos] = A
    return out


def _take_rows(F, rows0):
    """the rows rows0 (0-based, in that order) of F as a matrix of the same kind"""
    rows0 = np.asarray(rows0, dtype=np.int64)
    m = feat.feature_shape(F)[0]
    if isinstance(F, (feat.SparseMatrixCSR, feat.SparseBinMatrix)):
        new = np.full(m, -1, dtype=np.int64)
        new[rows0] = np.arange(len(rows0))                    # (rows0 holds no row twice: blocks and test subsets)
        to = new[np.asarray(F.rows, dtype=np.int64) - 1]
        keep = to >= 0
        rr = (to[keep] + 1).astype(np.int32)
        if isinstance(F, feat.SparseMatrixCSR):
            return feat.SparseMatrixCSR(rr, F.cols[keep], F.vals[keep], len(rows0), F.n)
        return feat.SparseBinMatrix(len(rows0), F.n, rr, F.cols[keep])
    if hasattr(F, "tocsr"):
        return F.tocsr()[rows0]
    return np.asarray(F, dtype=np.float64)[rows0]


class EntityState:
    """Device-resident EntityModel (RelationData.jl:14-40, initModel! :66-90)."""

    def __init__(self, ctx, en, D, tag, layout):
        self.ctx, self.D, self.tag, self.layout = ctx, D, tag, layout
        self.n_real = en.count
        self.N = layout.nint                     # rows of the factor matrix (rows nobody owns stay zero)
        # the rows of the next sweep are written to another buffer, then the three rotate: a launch overwrites the rows of
        # three sweeps ago, so readers of the previous two sweeps' rows on other streams are never overwritten under their feet
        self.bufs = [ctx.zeros(self.N, D) for _ in range(3)]
        self.cur = 0
        self.mu = ctx.zeros(D)
        self.Lambda = ctx.tensor(5.0 * np.eye(D))
        self.mu0 = ctx.zeros(D)
        self.b0 = 2.0
        self.WI = ctx.tensor(np.eye(D))
        self.nu0 = float(D)
        self.sumU = ctx.zeros(D)
        self.UUt = ctx.zeros(D, D)
        self.params = ctx.zeros(D + D * D)
        # what K1 needs of (mu, Lambda), written by the hyperprior draw (bdf_hyper_sample) so that K1 needs no pre-launch
        self.prior_pack = ctx.zeros(lib().bdf_prior_pack_doubles(D))
        self.prior_pack_valid = False
        # the random part of the hyperprior draw (Bartlett matrix + mean normals), drawn ahead of the rows (bdf_hyper_draws)
        self.draws = ctx.zeros(D * D + D)
        self.draws_sweep = None
        # a relation of the entity has background cells (setBackground): the prior its rows are sampled with, made before every
        # row launch (row_prior() of csrc/bdf_gibbs.hip); allocated by background_buffers()
        self.bg_Lambda = self.bg_mu = self.bg_pack = self.bg_alpha_rows = None
        # the spike-and-slab prior (setSpikeAndSlab): pi, tau, logit pi, log tau (D each; pi = 1/2, tau = 1 at the start)
        self.spike = en.spike
        self.spike_state = ctx.tensor(np.concatenate([np.full(D, 0.5), np.ones(D), np.zeros(D), np.zeros(D)])) if en.spike is not None else None
        # the non-negative prior (setNonNegative): tau (D; 1 at the start)
        self.nonneg = en.nonneg
        self.nonneg_tau = ctx.tensor(np.ones(D)) if en.nonneg is not None else None
        self.F = None
        self.numF = 0
        self.beta = ctx.zeros(D, 0)
        self.uhat = None
        self.mu_matrix = None
        self.Tinv = None
        self.lambda_beta = None
        self.cg_iters = None
        if not feat.isempty(en.F):
            if feat.feature_shape(en.F)[0] != en.count:
                raise ArgumentError(f"Entity {en.name} has {en.count} instances but its feature matrix has {feat.feature_shape(en.F)[0]} rows")
            self.F = FeatOperator(ctx, en.F, layout)
            self.numF = self.F.n
            self.beta = ctx.zeros(D, self.numF)          # numF x D column-major
            self.uhat = ctx.zeros(self.N, D)
            self.mu_matrix = ctx.zeros(self.N, D)
            self.Tinv = ctx.zeros(D, D)
            self.lambda_beta = ctx.tensor([en.lambda_beta])
            self.cg_iters = ctx.zeros(D, dtype=torch.int32)

    def background_buffers(self, dense=False):
        """(Lambda_eff, mu_eff -- one per row with side information --, their prior pack, alpha (1 - c0) per term) of bdf_background_prior;
        dense: of bdf_dense_prior, whose mu_eff is always one per row"""
        if dense and (self.bg_mu is None or self.bg_mu.dim() == 1):
            self.bg_mu = self.ctx.zeros(self.N, self.D)
        if self.bg_Lambda is None:
            ctx, D = self.ctx, self.D
            self.bg_Lambda = ctx.zeros(D, D)
            if self.bg_mu is None:
                self.bg_mu = ctx.zeros(self.N, D) if self.F is not None else ctx.zeros(D)
            self.bg_pack = ctx.zeros(lib().bdf_prior_pack_doubles(D))
            self.bg_alpha_rows = ctx.zeros(_lib.BDF_MAX_TERMS)

    def spike_active(self):
        """how many components have a nonzero loading in the current draw, over the entity's n_real rows: a count, read on the row
        stream, where the rows are written (the read waits for that stream alone)"""
        with torch.cuda.stream(self.ctx.stream):
            return int((self.sample[:self.n_real] != 0).any(dim=0).sum().item())

    @property
    def sample(self):
        return self.bufs[self.cur]

    @property
    def sample_next(self):
        return self.bufs[(self.cur + 1) % 3]

    def rotate(self):
        self.cur = (self.cur + 1) % 3

    def norm(self, name):
        """vecnorm of a device array (bdf_norm2: the squares summed in a fixed order) as a float, with no host copy of the array.
        On the row context's stream, where the samples and beta are written."""
        t = getattr(self, name)
        if t is None or t.numel() == 0:
            return 0.0
        with torch.cuda.stream(self.ctx.stream):
            out = torch.empty(1, dtype=torch.float64, device=self.ctx.device)
            check(lib().bdf_norm2(self.ctx.handle, t.numel(), _ptr(t), _ptr(out)))
            return float(out.item())

    def host(self, name):
        t = getattr(self, name)
        if t is None:
            return np.zeros((0, 0))
        torch.cuda.synchronize(t.device)      # the state is written on several streams (rows, hyperprior): wait for all of them
        a = t.detach().cpu().numpy()
        if name in ("sample", "uhat", "mu_matrix") and self.layout.pos is not None:
            a = a[self.layout.pos]            # internal positions -> the reference's row order
        return a.T.copy() if a.ndim == 2 else a.copy()


class DeviceOrdinal(_DeviceObject):
    """bdf_ordinal: the sampled edges of an ordinal relation with their Metropolis step's state and trace, on the device."""
    _destroy = "bdf_ordinal_destroy"

    def __init__(self, ctx, K, step=0.1, trace_capacity=0):
        self.ctx, self.K, self.capacity = ctx, int(K), int(trace_capacity)
        self.handle = C.c_void_p()
        check(lib().bdf_ordinal_create(ctx.handle, self.K, float(step), self.capacity, C.byref(self.handle)))
        ctx.adopt(self)

    def set_adapt(self, steps):
        """the first `steps` steps taken with adapt = -1 adapt the step size (the burn-in's length)"""
        check(lib().bdf_ordinal_set_adapt(self.handle, int(steps)))

    def step(self, ctx, train, codes, D, factors, mean_value, alpha, rel_tag, adapt, bounds):
        """one Metropolis step on ctx's stream (bdf_ordinal_step); alpha: a float, or a device scalar read on the device; codes: int8
        device tensor, the levels in the caller's order; bounds: (n, 2) device tensor, rewritten when the proposal is accepted"""
        check(lib().bdf_ordinal_step(ctx.handle, self.handle, train.handle, _ptr(codes), int(D), _facs(factors), float(mean_value),
                                     *_alpha_args(alpha), int(rel_tag), int(adapt), _ptr(bounds)))

    def bounds(self, ctx, codes, out):
        """out[k] = the bin of level codes[k] under the current edges, on ctx's stream (bdf_ordinal_bounds)"""
        check(lib().bdf_ordinal_bounds(ctx.handle, self.handle, _ptr(codes), int(codes.numel()), _ptr(out)))

    def read(self, trace_rows=0):
        """waits for the last step; {"edges", "sigma", "proposals", "accepts", "S", "trace"}"""
        edges, sigma, S = np.zeros(self.K - 1), C.c_double(), C.c_double()
        npr, nac = C.c_int64(), C.c_int64()
        trace = np.zeros((int(trace_rows), self.K - 1))
        check(lib().bdf_ordinal_read(self.handle, edges.ctypes.data_as(_lib.c_dp), C.byref(sigma), C.byref(npr), C.byref(nac), C.byref(S),
                                     trace.ctypes.data_as(_lib.c_dp), int(trace_rows)))
        return {"edges": edges, "sigma": sigma.value, "proposals": npr.value, "accepts": nac.value, "S": S.value, "trace": trace}

    def proposal(self):
        """(parity checks) the last step's {"edges" proposed, "jacobian", "accepted", "log_u"}"""
        edges, jac, lu, acc = np.zeros(self.K - 1), C.c_double(), C.c_double(), C.c_int()
        check(lib().bdf_ordinal_proposal(self.handle, edges.ctypes.data_as(_lib.c_dp), C.byref(jac), C.byref(acc), C.byref(lu)))
        return {"edges": edges, "jacobian": jac.value, "accepted": bool(acc.value), "log_u": lu.value}



def _bias_terms(dr):
    """DeviceRelation dr's biased modes as bdf_bias_term records, rising"""
    terms = (_lib.BiasTerm * len(dr.bias_spec))()
    for t, (m0, sp) in enumerate(dr.bias_spec.items()):
        terms[t].mode, terms[t].shape, terms[t].rate = m0, sp["shape"], sp["rate"]
        terms[t].bias, terms[t].lambda_ = dr.bias[m0].data_ptr(), dr.bias_lambda.data_ptr() + 8 * t
    return terms


def bias_baseline(dr, mean_value, pairs, out):
    """out (device, one double per pair, the caller's order) = mean_value + the current biases of every pair over the entities of
    DeviceRelation dr (bdf_bias_baseline), on the pairs' stream behind the relation's stream, where the biases are drawn"""
    if pairs.ctx is not dr.ctx:
        pairs.ctx.stream.wait_stream(dr.ctx.stream)
    check(lib().bdf_bias_baseline(pairs.ctx.handle, pairs.handle, len(dr.bias_spec), _bias_terms(dr), float(mean_value), _ptr(out)))
    return out


class GibbsEngine:
    """Device state of a RelationData and the per-iteration steps of macau.jl:80-140."""

    def __init__(self, data, num_latent, seed=0, device=None, lambda_beta=float("nan"), compute_ff_size=6500,
                 full_lambda_u=True, tol=float("nan"), shard=None, chunks=None):
        if not (1 <= num_latent <= _lib.BDF_MAX_D):
            raise ArgumentError(f"num_latent={num_latent} must be in 1..{_lib.BDF_MAX_D}")
        for r in data.relations:
            check_model(r, 1 if shard is None else shard[1])
        self.data, self.D = data, int(num_latent)
        # The row context runs on a stream of its own that leaves a few CUs (one or two per XCD) free for the hyperprior's
        # small kernels, which otherwise wait for slots beside the chip-filling row kernel -- when the entities are small
        # enough for those kernels to be small (the reductions of a 10M-row entity want the whole chip)
        big = max((en.count for en in data.entities), default=0) * int(num_latent) * 8 > (32 << 20)
        # (the test rig that runs several ranks on ONE GPU, BDF_DIST_BACKEND=gloo, reserves none: two processes' kernels on the
        # same eight masked CUs stalled each other for seconds once in ten runs -- k_hyper_chain's last workgroup ran into its spin
        # bound; one process per GPU, the deployment, has the reserved CUs to itself)
        rig = shard is not None and shard[1] > 1 and os.environ.get("BDF_DIST_BACKEND") == "gloo"
        reserve = int(os.environ.get("BDF_RESERVE_CUS", "0" if (big or rig) else "8"))
        self.ctx = Context.rows(device, seed, reserve)
        self.rank, self.world = (0, 1) if shard is None else shard
        self.full_lambda_u = bool(full_lambda_u)
        self.tol = float(tol)
        self.compute_ff_size = compute_ff_size
        # the whole iteration in one native call: entity side information, the relation models (alpha sampled, relation-level
        # side information: bdf_gibbs_set_relations) and the exchange between ranks included.  BDF_NO_NATIVE: enqueued step by
        # step from here instead (the same entry points, the same values)
        self.native = not os.environ.get("BDF_NO_NATIVE")
        # ---- row layouts (several ranks): degree of a row = its observations over all the entity's relations
        if chunks is None:
            chunks = int(os.environ.get("BDF_CHUNKS", "0"))
        # one chunk count for the whole model (a relation's modes share it): the chunked exchange -- the row kernel of chunk
        # c + 1 beside the all-gather of chunk c -- pays once an entity's share of rows is large
        if chunks <= 0:
            share = max(-(-en.count // self.world) for en in data.entities) if self.world > 1 else 0
            chunks = 8 if share >= 1_000_000 else (4 if share >= 200_000 else 1)      # the last chunk's exchange is what stays exposed
        self.layouts = []
        for en in data.entities:
            if self.world == 1:
                self.layouts.append(Layout(en.count))
                continue
            deg = np.zeros(en.count, dtype=np.int64)
            for r in en.relations:
                m = [e is en for e in r.entities].index(True)
                deg += np.bincount(np.asarray(r.data.ids[:, m], dtype=np.int64) - 1, minlength=en.count)
            self.layouts.append(Layout(en.count, deg, self.world, chunks))
        # ---- reset! (RelationData.jl:331-355)
        self.ent = []
        for en in data.entities:
            if en.spike is not None:
                from .relation_data import check_spike
                check_spike(en, 1 if shard is None else shard[1])
            if en.nonneg is not None:
                from .relation_data import check_nonneg
                check_nonneg(en, 1 if shard is None else shard[1])
        for j, en in enumerate(data.entities):
            if not np.isnan(lambda_beta):
                en.lambda_beta = float(lambda_beta)
            st = EntityState(self.ctx, en, self.D, j + 1, self.layouts[j])
            en.modes = [[e is en for e in r.entities].index(True) + 1 for r in en.relations]
            en.modes_other = [[k + 1 for k, e in enumerate(r.entities) if e is not en] for r in en.relations]
            if st.F is not None:
                en.use_FF = st.numF <= compute_ff_size
            from .relation_data import EntityModel
            en.model = EntityModel()
            en.model._dev = st
            self.ent.append(st)
        self.rel = []
        for r in data.relations:
            if len(r.entities) != len(r.data.dims):
                raise ArgumentError(f"Relation {r.name} has {len(r.entities)} entities but its data implies {r.data.size()}.")
            lays = [self.layouts[self._entity_index(e)] for e in r.entities]
            # (a dense relation lists no cell to the row kernels: its matrix reaches the rows through the prior, row_prior() of csrc/bdf_gibbs.hip)
            idf = r.data if not r.model.dense else type(r.data)((r.data.ids[:0], r.data.values[:0]), list(r.data.dims), names=r.data.names)
            dr = DeviceRelation(self.ctx, idf, lays if self.world > 1 else None, self.rank, values=_background_values(r))
            r._dev = dr
            self.rel.append(dr)
            self._build_model(r, dr, noise_kind(r))
            if dr.bg is not None or dr.dense is not None:
                for e in r.entities:
                    self.ent[self._entity_index(e)].background_buffers(dense=dr.dense is not None)
        self._test_pairs = None
        self._train_pairs = None
        self._new_rows = None
        self._test_opts = None
        self.k1_spans = None      # bench.py: (tensor n x 2 of uint64 ticks as int64, [entity per used slot]) -- device-side launch spans (k1_span_begin)
        self.k1_events = None     # bench.py: list of (entity, KernelTimer) of the timed K1 launches
        self.k1_event_every = 1   # ... of every n-th sweep
        self._k1_sweep = 0
        # ---- streams: rows (main) | hyperpriors | prediction updates
        self.comm = None
        self._ev_pred = None
        self._ev_rows, self._ev_hyper = {}, {}
        self._create_gibbs()
        # (callers take `gibbs` for the native path's handle: None step by step)
        self.gibbs = self._gibbs if self.native else None
        if not self.native:
            # BDF_NO_OVERLAP: everything on the row context (the object, created above, read it too: its hyperprior pieces go
            # there); a relation with features: the prediction updates stay there (their baseline is refreshed on the row stream)
            if os.environ.get("BDF_NO_OVERLAP"):
                self.ctx_h = self.ctx_p = self.ctx
            elif not all(feat.isempty(r.F) and not r.model.bias for r in data.relations):
                self.ctx_p = self.ctx            # (biases: the same -- their draw refreshes the test pairs' base on the row stream)
        torch.cuda.synchronize(self.ctx.device)      # everything set up above (on torch's streams too) is in place

    def _build_model(self, r, dr, kind):
        """relation r's model on the device (the fields DeviceRelation names): what _register_relations hands the library, which
        steps it before the rows.  kind: noise_kind(r), after check_model(r)"""
        ctx, m, nn = self.ctx, r.model, r.data.nnz()
        dr.kind, dr.alpha_sample = kind, bool(m.alpha_sample)
        # (probit: the latent is not centred; logit / counts: psi = u'v + the offset the setter was given)
        # (background cells: the mean over ALL cells, the unlisted ones at the background value -- valueMean of the dense listing)
        # (every entity non-negative, setNonNegative: u.v >= 0 models the values themselves -- not centred)
        all_nonneg = all(en.nonneg is not None for en in r.entities)
        m.mean_value = 0.0 if kind == "probit" else (m.pg["offset"] if kind in ("logit", "counts") else
                                                     (background_mean(r) if m.background is not None else
                                                      (_dense_mean(r) if m.dense else (0.0 if all_nonneg else dr.value_mean()))))
        # several ranks: the relation's observations (COO order) in world blocks of obs_block; this rank's block is
        # [obs_lo, obs_hi): its rows of the relation's feature matrix, its observations as pairs (the squared-error sum
        # of sample_alpha and F'v of sample_beta_rel are summed over the ranks in rank order, bdf_sum_ranks)
        dr.obs_block = -(-nn // self.world)
        dr.obs_lo = min(nn, self.rank * dr.obs_block)
        dr.obs_hi = min(nn, dr.obs_lo + dr.obs_block)
        if self.world > 1 and (not feat.isempty(r.F) or m.alpha_sample) and dr.obs_hi - dr.obs_lo < 1:
            raise ArgumentError(f"Relation {r.name} has fewer observations ({nn}) than a block per rank needs")
        # relation-level side information (RelationData.jl:348-353): FF path only, as in the reference
        if not feat.isempty(r.F):
            if feat.feature_shape(r.F)[0] != nn:
                raise ArgumentError(f"Relation {r.name} has {nn} observations but its feature matrix has {feat.feature_shape(r.F)[0]} rows")
            dr.F = FeatOperator(ctx, r.F if self.world == 1 else _take_rows(r.F, np.arange(dr.obs_lo, dr.obs_hi)))
            if dr.F.n > self.compute_ff_size:
                raise ArgumentError("conjugate gradient unimplemented for sampling relation beta")      # sampling.jl:335
            dr.beta = ctx.zeros(dr.F.n)
            m.beta = np.zeros(dr.F.n)
        # the training table as pairs: this rank's block for sample_alpha and sample_beta_rel; a noise model takes every row (one
        # rank), sorted -- its per-observation arrays stay in the caller's order, whichever way the pairs are stored
        ids, values = np.asarray(r.data.ids), np.asarray(r.data.values)
        if dr.F is not None or (m.alpha_sample and not m.dense):
            dr.train = self._pairs(ctx, r, ids[dr.obs_lo:dr.obs_hi], values[dr.obs_lo:dr.obs_hi])
        if kind != "gauss":
            dr.train = self._sorted_pairs(ctx, r, ids, values, dr.train)
        # linear_values of the row kernels (K1 reads [0, nnz)) start at mean_value: features add F beta (pred(r) = udot +
        # linear_values, sampling.jl:16-18); a latent z per observation drawn before the rows of every iteration leaves y - z
        # (probit, alpha = 1), mean + y - z (censored, interval, ordinal, the relation's alpha) or the Polya-Gamma
        # pseudo-observation offset + y - kappa / omega (logit, counts, alpha = 1)
        if dr.F is not None or kind in ("probit", "censored", "interval", "ordinal", "logit", "counts"):
            dr.linear = ctx.tensor(np.full(max(dr.obs_block * self.world, 1), m.mean_value))
        # ... and is the training pairs' baseline where sample_alpha's squared error is that of udot + linear_values: with features,
        # and of z for the censored models (the first alpha is drawn from the values as they are)
        if dr.F is not None or kind in ("censored", "interval", "ordinal"):
            check(lib().bdf_pairs_set_baseline(dr.train.handle, C.c_void_p(dr.linear.data_ptr() + 8 * dr.obs_lo)))
        if kind == "probit":                      # bdf_probit_draw; the training pairs predict probabilities (rmse_train)
            dr.train.set_link(1)
        elif kind == "censored":                  # bdf_censored_draw after alpha: z of every flagged observation
            dr.censor = ctx.tensor(m.censor if nn else np.zeros(1, dtype=np.int8), dtype=torch.int8)
        elif kind in ("interval", "ordinal"):     # bdf_interval_draw at the same place: a (lower, upper) pair per row in place of the flag
            dr.interval = ctx.tensor(m.interval if nn else np.zeros((1, 2)))
            if kind == "ordinal" and m.ordinal["sample_edges"]:
                # the bounds follow the sampled edges: one Metropolis step on them after alpha and before the latent draw
                # (bdf_ordinal_step), which rewrites dr.interval.  Without sampled edges the relation IS an interval relation.
                # (ordinal_begin gives the object its trace and burn-in)
                dr.ord_codes = ctx.tensor(m.ordinal_codes if nn else np.zeros(1, dtype=np.int8), dtype=torch.int8)
                dr.ordinal = DeviceOrdinal(ctx, m.ordinal["K"], m.ordinal["step"], 0)
        elif kind in ("weights", "robust"):
            # a precision weight per training row, which the row kernels read beside the relation's alpha (bdf_term.obs_precision):
            # the caller's weights, or the omega of the Student-t model -- drawn before alpha and the rows of every iteration
            # (bdf_robust_draw), which also leaves sum omega e^2 for sample_alpha
            dr.omega = ctx.tensor(m.weights if (kind == "weights" and nn) else np.ones(max(nn, 1)))
            dr.robust_nu = float(m.robust["nu"]) if kind == "robust" else 0.0
        elif kind == "entity_noise":
            # a noise precision tau_j per row of one entity, drawn where the robust model draws omega
            # (bdf_entity_noise_draw): tau per row of that mode, and -- what the row kernels of EVERY entity read as obs_precision --
            # tau of its row per training cell; the draw also leaves sum tau_j S_j for sample_alpha
            dr.noise = dict(m.entity_noise)
            dr.omega = ctx.tensor(np.ones(max(nn, 1)))
            dr.tau = ctx.tensor(np.ones(max(int(r.data.dims[dr.noise["mode"] - 1]), 1)))
        elif kind in ("logit", "counts"):
            # bdf_pg_draw: omega of every training row, the rows' obs_precision beside linear_values; the training pairs predict
            # through the model's link (rmse_train)
            dr.pg_model, dr.pg_r = (1, 0.0) if kind == "logit" else (2, float(m.pg["r"]))
            dr.omega = ctx.tensor(np.ones(max(nn, 1)))
            dr.train.set_pg_link(dr.pg_model, dr.pg_r)
        if m.bias:
            # biases (setBias): a bias per row of every listed mode and a precision per mode, drawn before alpha
            # and the rows of every iteration (bdf_bias_draw), which leaves mean + the cell's biases in linear_values: what the rows
            # of every entity read as their base, and the training pairs' baseline -- for alpha's sum of squares, rmse_train and WAIC
            dr.bias_spec = {int(mode) - 1: dict(spec) for mode, spec in sorted(m.bias.items())}
            dr.train = self._sorted_pairs(ctx, r, ids, values, dr.train)
            dr.linear = ctx.tensor(np.full(max(nn, 1), m.mean_value))
            check(lib().bdf_pairs_set_baseline(dr.train.handle, _ptr(dr.linear)))
            dr.bias = {m0: ctx.zeros(max(int(r.data.dims[m0]), 1)) for m0 in dr.bias_spec}
            dr.bias_lambda = ctx.tensor([sp["shape"] / sp["rate"] for sp in dr.bias_spec.values()])
            dr.bias_resid = ctx.zeros(max(nn, 1))
        if m.background is not None:
            # background cells (setBackground): every unlisted cell observes `value` with precision alpha c0.  The
            # rows of both entities are sampled with the prior row_prior() makes from the other entity's sum and Gram matrix (fold_sums:
            # per mode, D + D^2 doubles).  Unit weights: the relation was created from _background_values and its terms read alpha
            # (1 - c0) -- nothing per observation.  setWeights: the rows read omega_k - c0 and, through linear_values, the
            # pseudo-residual (omega_k r_k - c0 rb) / (omega_k - c0), both constant over the run; alpha's sum of squares reads omega_k
            c0, rb = m.background["weight"], m.background["value"] - m.mean_value
            dr.bg = dict(m.background)
            dr.fold_sums = ctx.zeros(2, self.D + self.D * self.D)
            if kind == "weights":
                w, y = np.asarray(m.weights, dtype=np.float64), np.asarray(values, dtype=np.float64)
                dr.bg_weights = dr.omega
                dr.omega = ctx.tensor((w - c0) if nn else np.ones(1))
                dr.linear = ctx.tensor((y - (w * (y - m.mean_value) - c0 * rb) / (w - c0)) if nn else np.full(1, m.mean_value))
        if m.dense:
            # a dense relation (setDense): R = Y - mean as one N x M matrix, a hole at 0 until the first
            # imputation.  The rows of both entities are sampled with the prior row_prior() makes from the other entity's Gram matrix
            # and the product R V (R' U), kept per mode in C; alpha's sum of squares is the closed form over the same pieces.
            Y, holes = dense_matrix(r)
            N, M = Y.shape
            listed = ~np.isnan(Y)
            R0 = np.where(listed, Y - m.mean_value, 0.0)
            Cs = ctx.zeros(N + M, self.D)              # (one buffer: the native iteration is handed its start)
            dr.dense = {"R": ctx.tensor(R0), "C": [Cs[:N], Cs[N:]], "sum_r2": math.fsum((R0 * R0).ravel().tolist()), "holes": None, "stats": None}
            dr.fold_sums = ctx.zeros(2, self.D + self.D * self.D)
            if len(holes):
                # the holes as pairs (the values are not read) and where their draw leaves the sum of their squares
                dr.dense["holes"] = self._pairs(ctx, r, holes + 1, np.zeros(len(holes)))
                dr.dense["stats"] = ctx.zeros(4)
        dr.alpha_dev = ctx.tensor([float(m.alpha)])

    # ---- the iteration object (bdf_gibbs) -----------------------------------------------------------------------------
    def _create_gibbs(self):
        """the library's description of the iteration, on both paths: the native one runs it whole (bdf_gibbs_sweep), the
        step-by-step one drives its pieces one by one (bdf_gibbs_step_relations, _rows, _draws, _hyper, _beta) on a schedule of its
        own, with the object's two side contexts"""
        ents = (GibbsEntity * len(self.ent))()
        for j, (en, st) in enumerate(zip(self.data.entities, self.ent)):
            g = ents[j]
            g.N, g.n_real, g.tag, g.n_terms = st.N, st.n_real, st.tag, len(en.relations)
            if not en.relations:
                raise ArgumentError(f"Entity {en.name} takes part in no relation")
            for t, r in enumerate(en.relations):
                g.terms[t].rel = self.rel[self._relation_index(r)].handle
                g.terms[t].mode = en.modes[t] - 1
                for k, e2 in enumerate(r.entities):
                    g.terms[t].entity_of_mode[k] = self._entity_index(e2)
                g.terms[t].alpha = r.model.alpha
                g.terms[t].mean_value = r.model.mean_value
            for b in range(3):
                g.sample[b] = st.bufs[b].data_ptr()
            for name in ("mu", "Lambda", "mu0", "WI", "sumU", "UUt", "params", "prior_pack", "draws"):
                setattr(g, name, getattr(st, name).data_ptr())
            g.b0, g.nu0 = st.b0, st.nu0
            if st.bg_Lambda is not None:
                for name in ("bg_Lambda", "bg_mu", "bg_pack", "bg_alpha_rows"):
                    setattr(g, name, getattr(st, name).data_ptr())
            if st.spike is not None:
                g.spike, g.spike_state = 1, st.spike_state.data_ptr()
                g.spike_a, g.spike_b, g.spike_shape, g.spike_rate = (st.spike[k] for k in ("incl_a", "incl_b", "shape", "rate"))
            if st.nonneg is not None:
                g.nonneg, g.nonneg_tau = 1, st.nonneg_tau.data_ptr()
                g.nonneg_shape, g.nonneg_rate = st.nonneg["shape"], st.nonneg["rate"]
            if st.F is not None:
                g.feat = st.F.handle
                for name in ("beta", "uhat", "mu_matrix", "Tinv", "lambda_beta", "cg_iters"):
                    setattr(g, name, getattr(st, name).data_ptr())
                g.use_ff, g.sample_lambda_beta, g.full_lambda_u = int(en.use_FF), int(en.lambda_beta_sample), int(self.full_lambda_u)
                g.tol, g.lb_nu, g.lb_mu = self.tol, en.nu, en.mu
        self._gibbs = C.c_void_p()
        check(lib().bdf_gibbs_create(self.ctx.handle, self.D, len(self.ent), ents, C.byref(self._gibbs)))
        h, p = C.c_void_p(), C.c_void_p()
        check(lib().bdf_gibbs_contexts(self._gibbs, C.byref(h), C.byref(p)))
        self.ctx_h = Context.wrap(h, self.ctx.device, self.ctx.seed)
        self.ctx_p = Context.wrap(p, self.ctx.device, self.ctx.seed)
        if self.world > 1 or os.environ.get("BDF_FORCE_COMM"):
            # (BDF_FORCE_COMM: a ONE-rank communicator all the same -- the exchange's kernels then run between the row launches
            # of a single-GPU run: the soak of the schedule with RCCL on the device, tools/soak_determinism.py rccl)
            self.comm = make_comm(self.ctx, self.rank, self.world)
            check(lib().bdf_gibbs_set_comm(self._gibbs, self.comm.handle))
        self._register_relations()

    def _register_relations(self):
        """the relations with a model of their own -- alpha sampled, relation-level side information, a noise model: the library
        steps them before the rows of every iteration (macau.jl:83-92) and makes their row terms"""
        from ._lib import GibbsRelation
        rows = [(ri, r, dr) for ri, (r, dr) in enumerate(zip(self.data.relations, self.rel)) if dr.has_model]
        arr = (GibbsRelation * max(len(rows), 1))()
        for k, (ri, r, dr) in enumerate(rows):
            g = arr[k]
            g.rel = dr.handle
            for m, e2 in enumerate(r.entities):
                g.entity_of_mode[m] = self._entity_index(e2)
            g.mean_value = r.model.mean_value
            g.alpha_dev = dr.alpha_dev.data_ptr()
            g.alpha_sample, g.rel_tag = int(bool(r.model.alpha_sample)), ri + 1
            g.alpha_lambda0, g.alpha_nu0, g.nnz = r.model.alpha_lambda0, r.model.alpha_nu0, r.data.nnz()
            g.train = dr.train.handle if dr.train is not None else None      # (a background with a fixed alpha and unit weights has none)
            g.first_obs, g.obs_block = dr.obs_lo, dr.obs_block
            g.probit, g.robust_nu, g.pg_model, g.pg_r = int(dr.kind == "probit"), dr.robust_nu, dr.pg_model, dr.pg_r
            if dr.bg is not None:
                g.bg_weight, g.bg_value = dr.bg["weight"], dr.bg["value"]
            if dr.dense is not None:
                dn = dr.dense
                g.dense_R, g.dense_C, g.dense_sum_r2 = dn["R"].data_ptr(), dn["C"][0].data_ptr(), dn["sum_r2"]
                if dn["holes"] is not None:
                    g.dense_holes, g.dense_stats = dn["holes"].handle, dn["stats"].data_ptr()
            if dr.bias is not None:
                g.n_bias, g.bias_resid = len(dr.bias_spec), dr.bias_resid.data_ptr()
                for t, bt in enumerate(_bias_terms(dr)):
                    g.bias[t] = bt
                if ri == 0 and dr.test_baseline is not None:
                    g.bias_test, g.test_baseline = self._test_pairs.handle, dr.test_baseline.data_ptr()
            if dr.noise is not None:
                g.noise_mode, g.noise_shape, g.noise_rate, g.noise_tau = dr.noise["mode"], dr.noise["shape"], dr.noise["rate"], dr.tau.data_ptr()
            for name, t in (("linear", dr.linear), ("censor", dr.censor), ("interval", dr.interval), ("ordinal_codes", dr.ord_codes),
                            ("obs_precision", dr.omega), ("beta", dr.beta), ("bg_weights", dr.bg_weights)):
                if t is not None:
                    setattr(g, name, t.data_ptr())
            if dr.fold_sums is not None:           # (the C struct keeps a field per family: the buffer goes to the one the relation uses)
                setattr(g, "dense_sums" if dr.dense is not None else "bg_sums", dr.fold_sums.data_ptr())
            if dr.ordinal is not None:
                g.ordinal = dr.ordinal.handle
            if dr.F is not None:
                g.feat, g.lambda_beta = dr.F.handle, r.model.lambda_beta
                if ri == 0 and dr.F_test is not None:
                    g.feat_test, g.test_baseline = dr.F_test.handle, dr.test_baseline.data_ptr()
        self._gibbs_relations = arr            # (the library copies the records; the tensors they point at live in self.rel)
        check(lib().bdf_gibbs_set_relations(self._gibbs, len(rows), C.cast(arr, C.c_void_p)))

    def bias_baseline(self, ri, pairs, out):
        """bias_baseline() of relation ri"""
        return bias_baseline(self.rel[ri], self.data.relations[ri].model.mean_value, pairs, out)

    def ordinal_begin(self, burnin, psamples, ri=0):
        """a run of burnin + psamples iterations starts on ordinal relation ri (sampled edges): its object gets a trace of that many
        rows and adapts its step size for the first `burnin` steps.  The chain must be at its start (a fresh engine)."""
        r, dr = self.data.relations[ri], self.rel[ri]
        if dr.ordinal is None:
            return None
        if dr.ordinal.read()["proposals"] != 0:
            raise ArgumentError(f"Relation {r.name} is ordinal: its edges' trace and burn-in cover one run; build a new engine (reset_model = true)")
        dr.ordinal.close()
        dr.ordinal = DeviceOrdinal(self.ctx, r.model.ordinal["K"], r.model.ordinal["step"], int(burnin) + int(psamples))
        dr.ordinal.set_adapt(burnin)
        self._register_relations()
        return dr.ordinal

    def warm_device(self, milliseconds=50.0):
        """set-up (native iteration): bring the device to its working state before the first iteration
        (bdf_gibbs_warm_device).  Full iterations -- rows of every entity, hyperprior chains, beta, the prediction kernel on
        the registered test pairs without running state -- with iteration numbers no real iteration uses, for `milliseconds`
        (several ranks: a fixed count, the same on every rank), then the chain's state is put back bit for bit.  Nothing of
        the chain advances.  (Row launches alone do not do it: a 20-iteration region behind 60 ms of them runs at 96-98 us
        per iteration, behind full iterations at 92-93: tools/region_idle_probe.py)  A no-op on the
        step-by-step path."""
        if self.gibbs and milliseconds > 0:
            check(lib().bdf_gibbs_warm_device(self.gibbs, float(milliseconds)))
            for j, st in enumerate(self.ent):          # the library's buffer rotation went on: follow it
                cur = C.c_int(0)
                check(lib().bdf_gibbs_current(self.gibbs, j, C.byref(cur)))
                st.cur = cur.value

    def k1_algorithmic_bytes(self, j):
        """bytes one K1 launch over all rows of entity j must move, summed over its relations:
        nnz*((4 + 8D)*(n_modes-1) + 8) + N*(8D + 8) [+ N*8D per-row prior mean] + 8D^2 + 8D"""
        en, st, D = self.data.entities[j], self.ent[j], self.D
        b = st.n_real * (8 * D + 8) + 8 * D * D + 8 * D + (st.n_real * 8 * D if st.F is not None else 0)
        for r in en.relations:
            b += r.data.nnz() * ((4 + 8 * D) * (len(r.entities) - 1) + 8)
        return b

    def k1_algorithmic_flops(self, j):
        """flops of one K1 launch over all rows of entity j by the reference's map (sampling.jl:200-212):
        nnz*(D(D+1) + 2D) [+ nnz*D*(n_modes-2) Hadamard] + N*(D^3/3 + 3D^2)"""
        en, st, D = self.data.entities[j], self.ent[j], self.D
        f = st.n_real * (D ** 3 / 3.0 + 3 * D * D)
        for r in en.relations:
            f += r.data.nnz() * (D * (D + 1) + 2 * D + D * max(len(r.entities) - 2, 0))
        return f

    def sample_written(self, j):
        """the caller has written entity j's sample itself, after sync(): K1c's gather image of it is stale and the next launch
        that gathers it packs a new one (bdf_gibbs_sample_written).  Without this call the rows of the opposite entity would
        still be sampled from the sample as it was."""
        check(lib().bdf_gibbs_sample_written(self._gibbs, int(j)))

    def rows_dispatch(self, j):
        """how the library dispatched entity j's latest row launch (Context.rows_dispatch); None before the first iteration"""
        return self.ctx.rows_dispatch(self.ent[j].tag)

    def lowrank_rows(self, j):
        """rows of entity j the library draws with the low-rank sampler (k_rows_lr.hip) instead of the reference's map -- the
        library's own count for the latest launch (bdf_ctx_rows_dispatch); before the first iteration: the rule of
        route_key and collect_rows (rows_plan.hip) restated from the environment (D > 16, one two-mode relation, no side information on the relation,
        rows of at most min(16, D / 2) observations (D > 32: min(32, D / 2)), at least 8,192 of them and at least half as many as the opposite entity has rows)"""
        got = self.rows_dispatch(j)
        if got is not None:
            return got["lowrank"]
        en, st, D = self.data.entities[j], self.ent[j], self.D
        lr = int(os.environ.get("BDF_LOWRANK", "-1"))
        cap = 32 if D > 32 else 16
        lr = min(cap, D // 2) if lr < 0 else min(lr, cap)
        if D <= 16 or lr == 0 or len(en.relations) != 1 or len(en.relations[0].entities) != 2:
            return 0
        r = en.relations[0]
        dr = self.rel[self._relation_index(r)]
        if dr.F is not None or dr.omega is not None:         # (not has_model: a sampled alpha alone leaves the rows on the low-rank sampler)
            return 0
        m = [e is en for e in r.entities].index(True)
        deg = np.bincount(np.asarray(r.data.ids[:, m], dtype=np.int64) - 1, minlength=en.count)
        cnt = int((deg <= lr).sum())
        min_rows = int(os.environ.get("BDF_LOWRANK_MIN_ROWS", "8192"))
        return cnt if (cnt >= max(min_rows, 1) and 2 * cnt >= r.data.dims[1 - m]) else 0

    # ---- helpers ----------------------------------------------------------------------------------------
    def _entity_index(self, en):
        return [e is en for e in self.data.entities].index(True)

    def _relation_index(self, r):
        return [x is r for x in self.data.relations].index(True)

    def _terms(self, j):
        """entity j's row terms as the library makes them for its next row launch (bdf_gibbs_terms; fill_terms() of
        csrc/bdf_gibbs.hip), the factors at the current samples"""
        terms = (Term * len(self.data.entities[j].relations))()
        check(lib().bdf_gibbs_terms(self._gibbs, int(j), terms))
        return terms

    def _row_prior(self, j):
        """parity hook: the fold of entity j's background and dense terms into its prior, enqueued on the row stream
        (bdf_gibbs_row_prior; row_prior() of csrc/bdf_gibbs.hip) -> the device addresses (mu, is_matrix, Lambda, pack) its next
        row launch would take (pack None: none)"""
        mu, Lam, pack, is_matrix = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int(0)
        check(lib().bdf_gibbs_row_prior(self._gibbs, int(j), int(self.ent[j].prior_pack_valid), C.byref(mu), C.byref(is_matrix), C.byref(Lam),
                                        C.byref(pack)))
        return mu, is_matrix.value, Lam, (pack if pack.value else None)

    # ---- macau.jl:83-92: relation models (alpha, relation-level beta) -----------------------------------------------
    def update_relations(self):
        """(step by step) what the relations' models run before the latent rows of the sweep, on the main stream
        (bdf_gibbs_step_relations), then one device-to-host read per sweep: a sampled alpha as the host scalar that the reporting
        steps on other streams take (driver.py), as the reference's host loop has it"""
        check(lib().bdf_gibbs_step_relations(self._gibbs))
        if any(r.model.alpha_sample for r in self.data.relations):
            self.ctx.sync()
            for r, dr in zip(self.data.relations, self.rel):
                if r.model.alpha_sample:
                    r.model.alpha = float(dr.alpha_dev.item())

    # ---- macau.jl:96-117: latent rows of entity j --------------------------------------------------------------
    def sample_entity(self, j):
        """entity j's rows into its next buffer, which then becomes the current one (bdf_gibbs_step_rows: uhat, the prior, the row
        launch chunk by chunk and, several ranks, every chunk's exchange) -- the step-by-step path's row step, and a launch by
        itself for the probes, under the iteration number the caller has set (ctx.set_sweep)"""
        st = self.ent[j]
        timed = self.k1_events is not None and self._k1_sweep % self.k1_event_every == 0
        if timed:
            timer = KernelTimer()
            check(lib().bdf_ctx_time_next_rows(self.ctx.handle, timer.start, timer.stop))
            self.k1_events.append((j, timer))
        check(lib().bdf_gibbs_step_rows(self._gibbs, int(j), int(st.prior_pack_valid)))
        st.rotate()

    # ---- macau.jl:119-134: hyperprior of entity j ----------------------------------------------------------------
    def prepare_prior(self, j, sweep):
        """the data-independent part of update_prior(j) of this sweep (bdf_gibbs_step_draws); may be issued before the rows of j
        are sampled"""
        check(lib().bdf_gibbs_step_draws(self._gibbs, int(j)))
        self.ent[j].draws_sweep = sweep

    def update_prior(self, j, sweep=None):
        """entity j's hyperprior from its current rows (bdf_gibbs_step_hyper), with the draws prepare_prior made for this sweep"""
        st = self.ent[j]
        check(lib().bdf_gibbs_step_hyper(self._gibbs, int(j), int(sweep is not None and st.draws_sweep == sweep)))
        st.prior_pack_valid = True

    # ---- macau.jl:138-140: beta of entity j ----------------------------------------------------------------
    def update_beta(self, j):
        check(lib().bdf_gibbs_step_beta(self._gibbs, int(j)))

    def sync_host_scalars(self):
        for en, st in zip(self.data.entities, self.ent):
            if st.lambda_beta is not None:
                en.lambda_beta = float(st.lambda_beta.item())
        for r, dr in zip(self.data.relations, self.rel):
            if dr.F is not None:
                r.model.beta = dr.beta.cpu().numpy().copy()
            if r.model.alpha_sample and self.native:       # (step by step the host reads it every iteration)
                r.model.alpha = float(dr.alpha_dev.item())
            if dr.ordinal is not None:
                r.model.ordinal_edges = dr.ordinal.read()["edges"]

    # ---- one Gibbs iteration (the timed unit of bench.py) ------------------------------------------------------
    def step(self, i, phase, clamp=(), class_cut=0.0):
        """iteration i and the reporting step of macau.jl:142-184 on the test pairs (phase 0 burn-in, 1 first posterior
        sample, 2 later ones); returns the pairs' device stats"""
        test = self.test_pairs()
        if self.native:
            self.register_test(clamp, class_cut)
            self.sweep(i, phase)
            return test.stats
        self.sweep(i)
        r = self.data.relations[0]
        return test.update(self.D, self.factors_of(r), r.model.mean_value, phase, list(clamp), class_cut)

    def register_test(self, clamp=(), class_cut=0.0):
        """(native iteration) the test pairs and reporting options the library's prediction update runs with; step() does it,
        a caller that warms the device before its first step does it first so that the warm-up runs the prediction kernel too"""
        if not self.native:
            return
        test = self.test_pairs()
        opts = (tuple(clamp), float(class_cut))
        if self._test_opts != opts:
            lo, hi = (clamp[0], clamp[1]) if len(clamp) else (1.0, -1.0)
            r = self.data.relations[0]
            eom = (C.c_int32 * len(r.entities))(*[self._entity_index(e) for e in r.entities])
            check(lib().bdf_gibbs_set_test(self.gibbs, test.handle, eom, r.model.mean_value, lo, hi, class_cut, _ptr(test.stats)))
            self._test_opts = opts

    def k1_span_begin(self, n):
        """the next n row launches of the native iteration leave {first wave's start, last wave's end} (100 MHz ticks) in a device
        buffer (bdf_gibbs_span_rows: K1c launches only) -- their durations with no event packets around them"""
        t = torch.zeros(n, 64, 2, dtype=torch.int64, device=self.ctx.device)      # (64 shards per launch: wave w uses shard w % 64)
        t[:, :, 0] = -1                    # (uint64 all ones: the kernel takes an atomic min)
        torch.cuda.synchronize(self.ctx.device)
        self.k1_spans = (t, [])

    def k1_span_result(self):
        """-> [(entity, microseconds)] of the launches that recorded a span"""
        if self.k1_spans is None:
            return []
        self.sync()
        t, ents = self.k1_spans
        self.k1_spans = None
        h = t.cpu().numpy().view(np.uint64)
        out = []
        for k, j in enumerate(ents):
            used = h[k, :, 1] > 0
            if used.any():
                out.append((j, (int(h[k, used, 1].max()) - int(h[k, used, 0].min())) / 100.0))
        return out

    def sweep(self, i, predict_phase=None):
        """iteration i without reporting (native: with the prediction update of `predict_phase` on the registered test pairs)"""
        self._k1_sweep = i
        if self.native and self.k1_spans is not None:
            t, ents = self.k1_spans
            for j in range(len(self.ent)):
                if len(ents) < t.shape[0]:
                    check(lib().bdf_gibbs_span_rows(self.gibbs, j, C.c_void_p(t[len(ents)].data_ptr())))
                    ents.append(j)
        if self.native:
            timed = self.k1_events is not None and i % self.k1_event_every == 0
            if timed:
                for j in range(len(self.ent)):
                    timer = KernelTimer()
                    check(lib().bdf_gibbs_time_rows(self.gibbs, j, timer.start, timer.stop))
                    self.k1_events.append((j, timer))
            check(lib().bdf_gibbs_sweep(self.gibbs, C.c_uint32(int(i)), -1 if (predict_phase is None or self._test_opts is None) else int(predict_phase)))
            for st in self.ent:
                st.rotate()
                st.prior_pack_valid = True
            return
        main, side = self.ctx.stream, self.ctx_h.stream
        two = self.ctx_h is not self.ctx
        self.ctx.set_sweep(i)
        if two:
            self.ctx_h.set_sweep(i)
        three = self.ctx_p is not self.ctx
        if three:
            self.ctx_p.set_sweep(i)
            # The row kernels of the NEXT sweep overwrite the buffers that held the rows of sweep i-2.  The prediction
            # updates that read those were all enqueued before the previous sweep began.  The side stream waits for them
            # here, where it idles until this sweep's first row kernel ends; every row kernel of the next sweep waits for a
            # hyperprior event recorded on the side stream after this point.
            if self._ev_pred is not None:
                side.wait_event(self._ev_pred)
            self._ev_pred = torch.cuda.Event()
            self._ev_pred.record(self.ctx_p.stream)
        self.update_relations()
        for j in range(len(self.ent)):
            if two and j in self._ev_hyper:
                main.wait_event(self._ev_hyper[j])       # (mu, Lambda) of entity j from the previous iteration
            if two:
                self.prepare_prior(j, i)                 # side stream, beside the row sampling
            self.sample_entity(j)
            if two:
                ev = self._ev_rows.setdefault(j, torch.cuda.Event())
                ev.record(main)
                side.wait_event(ev)
            self.update_prior(j, i)
            if two:
                ev = self._ev_hyper.setdefault(j, torch.cuda.Event())
                ev.record(side)
        if three:                                         # prediction updates read this sweep's rows
            self.ctx_p.stream.wait_event(self._ev_rows[len(self.ent) - 1])
        for j in range(len(self.ent)):
            if self.ent[j].F is not None:
                if two:
                    main.wait_event(self._ev_hyper[j])
                self.update_beta(j)
                if two:                                  # the next hyperprior of j reads beta / lambda_beta
                    ev = self._ev_rows.setdefault(j, torch.cuda.Event())
                    ev.record(main)
                    side.wait_event(ev)

    def sync(self):
        if self.gibbs:
            check(lib().bdf_gibbs_sync(self.gibbs))
            return
        if self.ctx_p is not self.ctx:
            self.ctx_p.sync()
        if self.ctx_h is not self.ctx:
            self.ctx_h.sync()
        self.ctx.sync()

    # ---- predictions ------------------------------------------------------------------------------------------
    def factors_of(self, r):
        return [self.ent[self._entity_index(e)].sample for e in r.entities]

    def pred_all(self, r):
        """pred_all(r) (sampling.jl:91-97): udot over every cell + mean_value (bdf_predict_all: k_predict.hip)"""
        S = []
        for e in r.entities:
            st = self.ent[self._entity_index(e)]
            S.append(st.sample if st.layout.pos is None else st.sample[torch.as_tensor(st.layout.pos.astype(np.int64), device=st.sample.device)])
        dims = [int(x.shape[0]) for x in S]
        with torch.cuda.stream(self.ctx.stream):
            S = [x.contiguous() for x in S]
            out = torch.empty(dims, dtype=torch.float64, device=S[0].device)
        check(lib().bdf_predict_all(self.ctx.handle, len(S), (C.c_int64 * len(S))(*dims), self.D, _facs(S), float(r.model.mean_value),
                                    C.c_void_p(out.data_ptr())))
        dr = self.rel[self._relation_index(r)]
        if dr.bias is not None:              # the biases' outer sum, in rising mode order, on the row stream behind their draw
            with torch.cuda.stream(self.ctx.stream):
                for m0, b in dr.bias.items():
                    out += b[:dims[m0]].reshape([-1 if k == m0 else 1 for k in range(len(dims))])
        return out

    def _pairs(self, ctx, r, ids, values):
        """test_vec / the training table as device pairs, ids at the entities' internal positions"""
        ids = np.asarray(ids).reshape(len(values), len(r.entities))
        if self.world > 1:
            ids = np.stack([self.layouts[self._entity_index(e)].to_internal(ids[:, k]) for k, e in enumerate(r.entities)], axis=1)
        return DevicePairs(ctx, ids, values)

    def _sorted_pairs(self, ctx, r, ids, values, pairs=None):
        """`pairs`, or (ids, values) as new pairs on ctx; a two-mode relation's are stored sorted by the mode with the fewest rows
        (most pairs per row): the kernels keep that mode's factor row in registers over a run of pairs and gather only the other
        mode's (k_predict_runs); results and per-pair arrays stay in the caller's order"""
        if pairs is None:
            pairs = self._pairs(ctx, r, ids, values)
        if len(r.entities) == 2 and pairs.n:
            pairs.sort(int(np.argmin(r.data.dims)))
        return pairs

    def test_pairs(self, subset=None):
        """the relation's test_vec on the device (subset: the rows of test_vec this rank predicts)"""
        r = self.data.relations[0]
        if self._test_pairs is None:
            ids = r.test_vec.ids.reshape(len(r.test_vec), len(r.entities))
            vals = np.asarray(r.test_vec.values)
            if subset is not None:
                ids, vals = ids[subset], vals[subset]
            # native iteration: the pairs belong to the row context (the library updates them on its own prediction stream)
            self._test_pairs = self._sorted_pairs(self.ctx if self.native else self.ctx_p, r, ids, vals)
            if r.model.probit:               # predictions are probabilities Phi(udot)
                self._test_pairs.set_link(1)
            dr = self.rel[0]
            if dr.pg_model:                  # ... the logistic probabilities / the counts' mean r e^psi
                self._test_pairs.set_pg_link(dr.pg_model, dr.pg_r)
            if dr.noise is not None:         # lpd_update scores a cell with alpha tau of its row (nothing else reads the scale)
                self._test_pairs.set_precision_scale(dr.tau, dr.noise["mode"] - 1)
            if dr.F is not None:             # pred(r, probe_vec, F) = udot + F_test beta + mean_value (sampling.jl:9-14)
                if feat.isempty(r.test_F):
                    raise ArgumentError(f"Relation {r.name} has features but its test set has no feature rows (test_F)")
                dr.F_test = FeatOperator(self.ctx, r.test_F if subset is None else _take_rows(r.test_F, np.asarray(subset)))
                dr.test_baseline = self.ctx.zeros(self._test_pairs.n)
                check(lib().bdf_pairs_set_baseline(self._test_pairs.handle, _ptr(dr.test_baseline)))
                self._register_relations()          # (the library refreshes the baseline after every relation beta)
            if dr.bias is not None:          # pred = udot + mean + the cell's biases: the draw refreshes the base of the registered pairs
                dr.test_baseline = self.ctx.zeros(max(self._test_pairs.n, 1))
                self.bias_baseline(0, self._test_pairs, dr.test_baseline)
                check(lib().bdf_pairs_set_baseline(self._test_pairs.handle, _ptr(dr.test_baseline)))
                self._register_relations()
        return self._test_pairs

    def new_rows(self, fresh=False):
        """the first relation's cells of new rows (setNewTest) on the device, built at first use; fresh: built again, with no state"""
        if fresh and self._new_rows is not None:
            self._new_rows.close()
            self._new_rows = None
        if self._new_rows is None:
            self._new_rows = DeviceNewRows(self, self.data.relations[0])
        return self._new_rows

    def train_pairs(self):
        r = self.data.relations[0]
        if self._train_pairs is None and self.rel[0].train is not None:
            self._train_pairs = self.rel[0].train
        if self._train_pairs is None:
            self._train_pairs = self._pairs(self.ctx_p if not self.native else self.ctx, r, r.data.ids, r.data.values)
        return self._train_pairs

    def close(self):
        if not self.ctx.handle:
            return
        try:
            self.sync()
        except Exception:
            pass
        for p in (self._test_pairs, self._train_pairs, self._new_rows):
            if p is not None:
                p.close()
        for st in self.ent:
            if st.F is not None:
                st.F.close()
        for dr in self.rel:
            dr.close()
        for side in (self.ctx_p, self.ctx_h):            # (what lives on them; the contexts themselves are the bdf_gibbs object's)
            if side is not self.ctx:
                side.close()
        lib().bdf_gibbs_destroy(self._gibbs)
        self._gibbs = self.gibbs = None
        if self.comm is not None:
            self.comm.close()
            self.comm = None
        self.ctx.close()


# ---- the communicator of a multi-rank run ----------------------------------------------------------------------------
class Comm:
    """bdf_comm: RCCL (one GPU per rank; the unique id travels over torch.distributed's channel), or -- several ranks on one
    GPU, the test rig BDF_DIST_BACKEND=gloo -- the library's host transport with a gloo all-gather behind it"""

    def __init__(self, ctx, rank, world):
        import torch.distributed as dist
        self.handle = C.c_void_p()
        self._cb = None
        self.transport = "RCCL (ncclAllGather in place, librccl resolved by the library)"
        if dist.get_backend() == "nccl":
            # every rank must end up on the same transport.  First the LOCAL preconditions of the library's own communicator --
            # librccl resolvable (bdf_comm_unique_id loads it and asks it for an id) -- agreed on over torch's process group
            # BEFORE any rank enters ncclCommInitRank: a rank that failed here alone would otherwise skip the collective
            # initialisation the others then block in
            err = ""
            raw0 = (C.c_char * _lib.BDF_COMM_ID_BYTES)()
            try:
                if os.environ.get("BDF_COMM_FORCE_STAGED"):
                    raise _lib.HipError("BDF_COMM_FORCE_STAGED is set")
                check(lib().bdf_comm_unique_id(raw0))
            except Exception as e:          # noqa: BLE001 -- agreed on below, then reported
                err = f"{type(e).__name__}: {e}"
            ok = torch.tensor([0 if err else 1], dtype=torch.int32, device=ctx.device)
            dist.all_reduce(ok, op=dist.ReduceOp.MIN)
            pre_ok = int(ok.item()) == 1
            buf = torch.zeros(_lib.BDF_COMM_ID_BYTES, dtype=torch.uint8)
            if rank == 0 and pre_ok:
                buf = torch.frombuffer(bytearray(raw0.raw), dtype=torch.uint8).clone()
            dev = buf.to(ctx.device)
            dist.broadcast(dev, src=0)
            raw = bytes(dev.cpu().numpy().tobytes())
            # every rank must end up on the same transport: the outcome of the library's own communicator is agreed on over
            # torch's process group; if any rank could not create it, all of them exchange through torch.distributed instead
            # (the library's host transport: staged through host memory -- slower, and said so in `transport`)
            # ... then the collective initialisation itself (every rank enters it, or none does), its outcome agreed on again
            try:
                if pre_ok:
                    check(lib().bdf_comm_create(ctx.handle, rank, world, raw, C.byref(self.handle)))
                elif not err:
                    err = "another rank cannot load librccl"
            except Exception as e:          # noqa: BLE001 -- agreed on below, then reported
                err = f"{type(e).__name__}: {e}"
            ok = torch.tensor([0 if err else 1], dtype=torch.int32, device=ctx.device)
            dist.all_reduce(ok, op=dist.ReduceOp.MIN)
            if int(ok.item()) == 0:
                if self.handle:
                    lib().bdf_comm_destroy(self.handle)
                    self.handle = C.c_void_p()
                self.transport = ("torch.distributed all-gather behind the library's host transport (a rank could not create the "
                                  "library's RCCL communicator" + (f": {err}" if err else "") + ")")
                print(f"[bdf] rank {rank}: {self.transport}", file=sys.stderr, flush=True)
                self._host_transport(ctx, rank, world, on_device=True)
        else:
            self.transport = "host transport with a gloo all-gather behind it (test rig: several ranks on one GPU)"
            self._host_transport(ctx, rank, world, on_device=False)
        self._enable_peer(ctx, rank, world, on_device=dist.get_backend() == "nccl")

    def _enable_peer(self, ctx, rank, world, on_device):
        """large exchanges (>= BDF_COMM_PEER_MIN_BYTES per rank, default 4 MiB) by direct all-pairs copies over IPC mappings
        (bdf_comm_enable_peer; ordered on the device by interprocess events) -- after a collective self-test: every rank pulls a
        small block from every other one and checks it; if any rank fails (no peer access, IPC refused) all of them stay on the
        communicator's own transport.  Off unless BDF_COMM_PEER=1: unmeasured on a node with several GPUs."""
        import torch.distributed as dist
        self.peer_min_bytes = None
        # (opt-in until it has run on a node with several GPUs: BDF_COMM_PEER=1)
        if world <= 1 or os.environ.get("BDF_COMM_PEER", "0") != "1":
            return
        self._peer_cb = _lib.EXCHANGE_FN(self._make_exchange(ctx, world, on_device))
        min_bytes = int(os.environ.get("BDF_COMM_PEER_MIN_BYTES", str(4 << 20)))
        err = ""
        try:
            check(lib().bdf_comm_enable_peer(self.handle, self._peer_cb, None, 0))
            probe = torch.full((world, 64), -1.0, dtype=torch.float64, device=ctx.device)
            probe[rank] = float(rank + 1)
            torch.cuda.synchronize(ctx.device)
            check(lib().bdf_comm_peer_selftest(ctx.handle, self.handle, C.c_void_p(probe.data_ptr()), 64 * 8))
            torch.cuda.synchronize(ctx.device)
            want = torch.arange(1, world + 1, dtype=torch.float64, device=ctx.device)[:, None].expand(world, 64)
            if not torch.equal(probe, want):
                err = "the self-test's blocks did not arrive"
        except Exception as e:          # noqa: BLE001 -- agreed on below
            err = f"{type(e).__name__}: {e}"
        ok = torch.tensor([0 if err else 1], dtype=torch.int32, device=ctx.device if on_device else "cpu")
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        if int(ok.item()) == 0:
            lib().bdf_comm_disable_peer(self.handle)
            if err:
                print(f"[bdf] rank {rank}: direct peer copies are off ({err})", file=sys.stderr, flush=True)
            return
        check(lib().bdf_comm_enable_peer(self.handle, self._peer_cb, None, min_bytes))
        self.peer_min_bytes = min_bytes
        self.transport += (f"; row exchanges of >= {min_bytes} bytes per rank by direct all-pairs peer copies over IPC mappings, "
                           f"ordered on the device by interprocess events (bdf_comm_enable_peer: one copy per xGMI link at once instead of the ring)")

    def peer_stats(self):
        n, b = C.c_int64(0), C.c_int64(0)
        check(lib().bdf_comm_peer_stats(self.handle, C.byref(n), C.byref(b)))
        return n.value, b.value

    def _make_exchange(self, ctx, world, on_device):
        import torch.distributed as dist

        def exchange(user, send, recv, nbytes):
            try:
                s = torch.frombuffer((C.c_char * nbytes).from_address(send), dtype=torch.uint8)
                r = torch.frombuffer((C.c_char * (nbytes * world)).from_address(recv), dtype=torch.uint8)
                if on_device:               # torch's own RCCL process group: through device tensors
                    rd = torch.empty(nbytes * world, dtype=torch.uint8, device=ctx.device)
                    dist.all_gather_into_tensor(rd, s.to(ctx.device))
                    r.copy_(rd.cpu())
                else:
                    dist.all_gather_into_tensor(r, s)
                return 0
            except Exception:        # noqa: BLE001 -- reported through the library's error code
                return 1
        return exchange

    def _host_transport(self, ctx, rank, world, on_device):
        self._cb = _lib.EXCHANGE_FN(self._make_exchange(ctx, world, on_device))
        check(lib().bdf_comm_create_host(ctx.handle, rank, world, self._cb, None, C.byref(self.handle)))

    def close(self):
        if self.handle:
            lib().bdf_comm_destroy(self.handle)
            self.handle = C.c_void_p()


def make_comm(ctx, rank, world):
    return Comm(ctx, rank, world)
