"""Row and column biases on the GPU (setBias): bdf_bias_draw and bdf_bias_baseline against the restatement
(tests/bias_restatement.py) with rows planted on the group boundaries of both widths and with more workgroups than lambda's reduction has threads, the errors of the C ABI, whole macau()
iterations against the restated chain on both iteration paths, the Gaussian chain untouched by an engine with biases in the same
process, a relation without biases beside one with them, and planted biases."""
import ctypes as C
import math
import os
import textwrap

import numpy as np
import pytest

from both_paths import child
import bias_restatement as BR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1234
COUNTS = (0, 1, 7, 8, 9, 63, 64, 65, 300)          # cells of the planted rows 0 .. 8: the group boundaries of the widths 8 and 64
N_CELLS = 1003                                       # not a multiple of 8 or of 256


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _facs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _planted_ids(rng, dims, mode):
    """N_CELLS cells; row r < 9 of `mode` has exactly COUNTS[r] of them, the other rows share the rest; in random order
    (test_gpu_entity_noise.py's layout)"""
    rest = N_CELLS - sum(COUNTS)
    col = np.concatenate([np.repeat(np.arange(1, len(COUNTS) + 1), COUNTS), rng.integers(len(COUNTS) + 1, dims[mode] + 1, rest)])
    col = rng.permutation(col)
    ids = np.stack([col if k == mode else rng.integers(1, d + 1, N_CELLS) for k, d in enumerate(dims)], axis=1).astype(np.int64)
    assert tuple(np.bincount(ids[:, mode] - 1, minlength=dims[mode])[:len(COUNTS)]) == COUNTS
    return ids


def _width(n, N):
    """the rule of the header: 8 lanes per row when the mean degree is at most 32, else 64"""
    return 8 if n <= 32 * N else 64


def _terms(B, modes, spec, bias, lam):
    """bdf_bias_term records in the order `modes` lists them (the library takes them in rising mode order whatever the listing)"""
    from bdf_amd._lib import BiasTerm
    t = (BiasTerm * len(modes))()
    for k, m in enumerate(modes):
        t[k].mode, t[k].shape, t[k].rate = m, spec[m][0], spec[m][1]
        t[k].bias, t[k].lambda_ = bias[m].data_ptr(), lam[m].data_ptr()
    return t


# ---- (a) the draw ---------------------------------------------------------------------------------------------------------------
# (number of modes, the biased modes as they are listed, the mode whose rows are planted)
LAYOUTS = [(2, (0,), 0), (2, (1,), 1), (2, (0, 1), 0), (2, (1, 0), 1), (3, (1,), 1), (3, (2, 0, 1), 2), (3, (0, 1, 2), 0)]


@pytest.mark.parametrize("sort", [False, True])
@pytest.mark.parametrize("n_modes,biased,plant", LAYOUTS)
@pytest.mark.parametrize("D", [1, 7, 32, 64])
def test_bias_draw_matches_the_restatement(B, ctx, D, n_modes, biased, plant, sort):
    """Two relations per case: dims [37, 23, 11][:n_modes], and the same with the planted mode's size changed so that its mean degree
    falls on the other side of 32 -- every case runs the 8-wide and the 64-wide row pass over rows of exactly 0, 1, 7, 8, 9, 63, 64,
    65 and 300 cells (the width follows from the shape alone, so the rule itself says which ran).  One mode, both modes of a matrix
    and all three of a tensor are biased, listed in rising and in other orders; alpha as a scalar and through alpha_dev with a decoy
    scalar; the biases and precisions the step finds are random, so that what it subtracts matters.

    Residuals are the device's own: e = y - bdf_predict on the same pairs, which the first launch forms in that very order.  Per
    biased mode in rising order, r_k = e_k less the other biased modes' biases -- the DEVICE's new draw for a mode drawn earlier,
    the values the step found for a later one -- S_j and sum |r_k| by math.fsum, z_j from the restated stream:
      |b_j - b_ref| <= 1e-13 (alpha sum_k |r_k| / prec_j + |b_ref|)
    (any summation order of at most 300 terms is within 300 x 2^-53 = 3.3e-14 of sum |r|; the remaining operations are a few ulp).
    lambda within 1e-12 relative of G_ref / (rate + sum b_dev^2 / 2).  linear_out and bdf_bias_baseline on other pairs equal, bit
    for bit, mean + the device's biases added in rising mode order; a rerun from the same state gives the same bits."""
    from bdf_amd._lib import check, lib
    rng = np.random.default_rng(7000 + 100 * D + 10 * n_modes + 2 * plant + sort + 1000 * len(biased))
    base_dims = [37, 23, 11][:n_modes]
    other = list(base_dims)
    other[plant] = 20 if _width(N_CELLS, base_dims[plant]) == 8 else 40
    widths = set()
    sweep, worst_b, worst_l = 20, 0.0, 0.0
    rising = sorted(biased)
    for dims in (base_dims, other):
        widths.add(_width(N_CELLS, dims[plant]))
        ids = _planted_ids(rng, dims, plant)
        y = rng.standard_normal(N_CELLS)
        dr = B.DeviceRelation(ctx, B.IndexedDF((ids, y), dims))
        pairs = B.DevicePairs(ctx, ids, y)
        probe_ids = np.stack([rng.integers(1, d + 1, 77) for d in dims], axis=1)
        probe = B.DevicePairs(ctx, probe_ids, np.zeros(77))
        if sort:
            pairs.sort(n_modes - 1)
            probe.sort(0)
        St = [ctx.tensor(rng.standard_normal((d, D))) for d in dims]
        mean = 0.3
        e = y - pairs.predict(D, St, mean).cpu().numpy()
        for (alpha, through_dev) in ((1.7, False), (40.0, True)):
            sweep += 1
            tag = 1 + sweep % 3
            spec = {m: (0.5 + m, 2.0 - 0.5 * m) for m in biased}
            b0 = {m: rng.standard_normal(dims[m]) for m in biased}
            lam0 = {m: float(np.exp(rng.uniform(-1, 1))) for m in biased}
            a_arg, a_dev = (alpha, None) if not through_dev else (123.0, ctx.tensor([alpha]))      # the decoy loses
            ctx.set_sweep(sweep)

            def draw():
                bt = {m: ctx.tensor(b0[m]) for m in biased}
                lt = {m: ctx.tensor([lam0[m]]) for m in biased}
                resid, lin, pb = ctx.tensor(np.full(N_CELLS, np.nan)), ctx.tensor(np.full(N_CELLS, np.nan)), ctx.tensor(np.full(77, np.nan))
                terms = _terms(B, biased, spec, bt, lt)
                check(lib().bdf_bias_draw(ctx.handle, dr.handle, pairs.handle, D, _facs(St), mean, a_arg, _p(a_dev), tag, len(biased), terms,
                                          _p(resid), _p(lin)))
                check(lib().bdf_bias_baseline(ctx.handle, probe.handle, len(biased), terms, mean, _p(pb)))
                ctx.sync()
                return ({m: bt[m].cpu().numpy() for m in biased}, {m: float(lt[m].item()) for m in biased}, resid.cpu().numpy(),
                        lin.cpu().numpy(), pb.cpu().numpy())

            b, lam, resid, lin, pb = draw()
            assert np.array_equal(resid, e)                                          # the same bits as y - bdf_predict, in the caller's order
            cur = dict(b0)
            for m in rising:
                N = dims[m]
                rows0 = ids[:, m] - 1
                r = BR.others_off(e, ids, cur, m)
                n_j = np.bincount(rows0, minlength=N)
                S = np.array([math.fsum(r[rows0 == j].tolist()) for j in range(N)])
                A = np.array([math.fsum(np.abs(r[rows0 == j]).tolist()) for j in range(N)])
                z = BR.normals(SEED, sweep, tag, np.arange(N), m)
                ref = BR.draw_rows(S, n_j, alpha, lam0[m], z)
                prec = lam0[m] + alpha * n_j
                bound = 1e-13 * (alpha * A / prec + np.abs(ref))
                err = np.abs(b[m] - ref)
                worst_b = max(worst_b, float((err / bound).max()))
                assert np.all(np.isfinite(b[m])) and np.all(err <= bound), (dims, m, alpha, int(np.argmax(err / bound)), float((err / bound).max()))
                if m == plant:
                    assert n_j[0] == 0 and A[0] == 0.0 and ref[0] == z[0] / np.sqrt(lam0[m])      # a row without cells: its prior's draw
                G = float(BR.gamma_variates(SEED, sweep, tag, [m], spec[m][0] + 0.5 * N)[0])
                lref = BR.draw_lambda(G, spec[m][1], math.fsum((b[m] * b[m]).tolist()))
                worst_l = max(worst_l, abs(lam[m] / lref - 1.0))
                assert abs(lam[m] / lref - 1.0) <= 1e-12, (dims, m, lam[m], lref)
                cur[m] = b[m]                                                        # the next mode sees the device's draw
            assert np.array_equal(lin, BR.base(ids, b, mean)) and np.array_equal(pb, BR.base(probe_ids, b, mean))
            b2, lam2, resid2, lin2, pb2 = draw()
            assert all(np.array_equal(b[m], b2[m]) and lam[m] == lam2[m] for m in biased)
            assert np.array_equal(resid, resid2) and np.array_equal(lin, lin2) and np.array_equal(pb, pb2)
        probe.close()
        pairs.close()
        dr.close()
    assert widths == {8, 64}
    print(f"bias draw D={D} modes={n_modes} biased={biased} sort={sort}: worst |b - b_ref| / bound {worst_b:.3f}, "
          f"max rel. error of lambda {worst_l:.3e} over 4 draws")


def _fsum_by_row(rows0, N, x):
    """math.fsum of x over the cells of every row 0 .. N - 1"""
    order = np.argsort(rows0, kind="stable")
    cut = np.searchsorted(rows0[order], np.arange(N + 1))
    xs = x[order]
    return np.array([math.fsum(xs[cut[j]:cut[j + 1]].tolist()) for j in range(N)])


FINAL = 256                                          # threads of k_bias_lambda: the partial sums of b^2 it adds in one pass


def _many_rows_ids(rng, kind):
    """(width, dims, ids) of a two-mode relation whose mode 0 leaves 257 workgroups' sums of b^2: "8-empty": 32 x 256 + 1 rows, three
    cells per row on average, some rows empty; "8-full": the same with at least one cell in every row; "64": 4 x 256 + 1 rows of 32
    cells and 40 more somewhere -- the last workgroup holds one group"""
    if kind == "64":
        N = 4 * FINAL + 1
        rows = np.concatenate([np.repeat(np.arange(1, N + 1), 32), rng.integers(1, N + 1, 40)])
    else:
        N = 32 * FINAL + 1
        rows = rng.integers(1, N + 1, 3 * N) if kind == "8-empty" else np.concatenate([np.arange(1, N + 1), rng.integers(1, N + 1, 2 * N)])
    rows = rng.permutation(rows)
    return (64 if kind == "64" else 8), [N, 200], np.stack([rows, rng.integers(1, 201, len(rows))], axis=1).astype(np.int64)


@pytest.mark.parametrize("biased", [(0,), (0, 1)])
def test_bias_draw_with_more_than_256_partial_sums_of_b2(B, ctx, biased):
    """k_bias_lambda adds the workgroups' sums of b^2 with 256 threads: 257 workgroups are its second pass.  Three relations at D = 7,
    mode 0 biased alone and both modes biased: the 8-wide row pass over 8193 rows (32 rows a workgroup), some of them empty, and
    over 8193 rows that all have cells; the 64-wide one over 1025 rows (4 a workgroup) and 32 x 1025 + 40 cells.  Rows are taken by
    falling degree, so the row that is alone in workgroup 257 is an empty one in the first relation (its bias is its prior's draw)
    and has cells in the other two.  The checks and bounds are test_bias_draw_matches_the_restatement's (mode 1 has 200 rows, so
    that no row has more than the 300 cells its bound reckons with: asserted); the rows' normals are BR.normals_reduced's, whose
    cosine has the device's exact reduction of the angle -- with BR.normals an empty row of the first relation, u = 0.7501944, is
    2.3 bounds off, which is the rounded angle's error in the reference, not the device's.  That lambda's bound bites is asserted on the CPU:
    the reference from the first 256 workgroups' rows alone is more than 1e-9 away from the full one."""
    from bdf_amd._lib import check, lib
    D, mean, sweep = 7, 0.3, 40 + len(biased)
    rising = sorted(biased)
    for kind in ("8-empty", "8-full", "64"):
        rng = np.random.default_rng(8100 + 10 * len(biased) + len(kind))
        width, dims, ids = _many_rows_ids(rng, kind)
        n = len(ids)
        per_group = 256 // width
        assert _width(n, dims[0]) == width and -(-dims[0] // per_group) == FINAL + 1 and dims[0] % per_group == 1
        y = rng.standard_normal(n)
        dr = B.DeviceRelation(ctx, B.IndexedDF((ids, y), dims))
        pairs = B.DevicePairs(ctx, ids, y)
        probe_ids = np.stack([rng.integers(1, d + 1, 77) for d in dims], axis=1)
        probe = B.DevicePairs(ctx, probe_ids, np.zeros(77))
        St = [ctx.tensor(rng.standard_normal((d, D))) for d in dims]
        e = y - pairs.predict(D, St, mean).cpu().numpy()
        alpha, through_dev = (1.7, False) if len(biased) == 1 else (40.0, True)
        sweep += 1
        tag = 1 + sweep % 3
        spec = {m: (0.5 + m, 2.0 - 0.5 * m) for m in biased}
        b0 = {m: rng.standard_normal(dims[m]) for m in biased}
        lam0 = {m: float(np.exp(rng.uniform(-1, 1))) for m in biased}
        a_arg, a_dev = (alpha, None) if not through_dev else (123.0, ctx.tensor([alpha]))      # the decoy loses
        ctx.set_sweep(sweep)

        def draw():
            bt = {m: ctx.tensor(b0[m]) for m in biased}
            lt = {m: ctx.tensor([lam0[m]]) for m in biased}
            resid, lin, pb = ctx.tensor(np.full(n, np.nan)), ctx.tensor(np.full(n, np.nan)), ctx.tensor(np.full(77, np.nan))
            terms = _terms(B, biased, spec, bt, lt)
            check(lib().bdf_bias_draw(ctx.handle, dr.handle, pairs.handle, D, _facs(St), mean, a_arg, _p(a_dev), tag, len(biased), terms,
                                      _p(resid), _p(lin)))
            check(lib().bdf_bias_baseline(ctx.handle, probe.handle, len(biased), terms, mean, _p(pb)))
            ctx.sync()
            return ({m: bt[m].cpu().numpy() for m in biased}, {m: float(lt[m].item()) for m in biased}, resid.cpu().numpy(),
                    lin.cpu().numpy(), pb.cpu().numpy())

        b, lam, resid, lin, pb = draw()
        assert np.array_equal(resid, e)
        cur = dict(b0)
        for m in rising:
            N = dims[m]
            rows0 = ids[:, m] - 1
            r = BR.others_off(e, ids, cur, m)
            n_j = np.bincount(rows0, minlength=N)
            assert n_j.max() <= 300
            S, A = _fsum_by_row(rows0, N, r), _fsum_by_row(rows0, N, np.abs(r))
            # (among thousands of rows one without cells draws a normal near a zero of its cosine: BR.normals_reduced)
            z = BR.normals_reduced(SEED, sweep, tag, np.arange(N), m)
            assert np.abs(z - BR.normals(SEED, sweep, tag, np.arange(N), m)).max() <= 1e-14
            ref = BR.draw_rows(S, n_j, alpha, lam0[m], z)
            prec = lam0[m] + alpha * n_j
            bound = 1e-13 * (alpha * A / prec + np.abs(ref))
            err = np.abs(b[m] - ref)
            assert np.all(np.isfinite(b[m])) and np.all(err <= bound), (kind, m, int(np.argmax(err / bound)), float((err / bound).max()))
            G = float(BR.gamma_variates(SEED, sweep, tag, [m], spec[m][0] + 0.5 * N)[0])
            lref = BR.draw_lambda(G, spec[m][1], math.fsum((b[m] * b[m]).tolist()))
            if m == 0:
                order = dr.order(0)
                assert sorted(order) == list(range(N)) and np.all(np.diff(n_j[order]) <= 0)
                assert (n_j[order[-1]] == 0) == (kind == "8-empty") and (n_j.min() == 0) == (kind == "8-empty")
                head = b[0][order[:FINAL * per_group]]                               # what the first 256 workgroups hold
                short = BR.draw_lambda(G, spec[m][1], math.fsum((head * head).tolist()))
                assert abs(short / lref - 1.0) > 1e-9, (kind, short, lref)
            print(f"bias draw past 256 partial sums, {kind} biased={biased} mode {m}: worst |b - b_ref| / bound {float((err / bound).max()):.3f}, "
                  f"rel. error of lambda {abs(lam[m] / lref - 1.0):.3e}")
            assert abs(lam[m] / lref - 1.0) <= 1e-12, (kind, m, lam[m], lref)
            cur[m] = b[m]
        assert np.array_equal(lin, BR.base(ids, b, mean)) and np.array_equal(pb, BR.base(probe_ids, b, mean))
        b2, lam2, resid2, lin2, pb2 = draw()
        assert all(np.array_equal(b[m], b2[m]) and lam[m] == lam2[m] for m in biased)
        assert np.array_equal(resid, resid2) and np.array_equal(lin, lin2) and np.array_equal(pb, pb2)
        probe.close()
        pairs.close()
        dr.close()


# ---- (b) errors through the C ABI ---------------------------------------------------------------------------------------------
def test_bias_c_abi_errors(B, ctx):
    import torch
    from bdf_amd._lib import BiasTerm, GibbsRelation, check, lib
    ids, y, _, _, _, _ = BR.planted(seed=9, N1=60, N2=50, n_train=1500, n_test=0)
    rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "e", [B.Entity("u"), B.Entity("v")], dims=[60, 50])
    eng = B.GibbsEngine(B.RelationData(rel), 8, seed=3)
    assert eng.native
    n = len(y)
    train = B.DevicePairs(eng.ctx, ids, y)
    lin, alpha = eng.ctx.tensor(np.full(n, rel.model.mean_value)), eng.ctx.tensor([1.0])
    check(lib().bdf_pairs_set_baseline(train.handle, _p(lin)))
    resid, tb = eng.ctx.zeros(n), eng.ctx.zeros(n)
    bu, bv, lam = eng.ctx.zeros(60), eng.ctx.zeros(50), eng.ctx.tensor([1.0, 1.0])
    om = eng.ctx.tensor(np.ones(n))
    op = B.FeatOperator(eng.ctx, np.ones((n, 2)))
    beta = eng.ctx.zeros(2)
    flags = eng.ctx.tensor(np.zeros(n, dtype=np.int8), dtype=torch.int8)
    bounds = eng.ctx.tensor(np.stack([y, y], axis=1))
    sums = eng.ctx.zeros(2, 8 + 64)

    def terms(spec=((0, 1.0, 1.0), (1, 1.0, 1.0)), bias=None, lambdas=None):
        t = (BiasTerm * max(len(spec), 1))()
        for k, (m, sh, rt) in enumerate(spec):
            t[k].mode, t[k].shape, t[k].rate = m, sh, rt
            t[k].bias = (bias or [bu.data_ptr(), bv.data_ptr()])[k]
            t[k].lambda_ = (lambdas or [lam.data_ptr(), lam.data_ptr() + 8])[k]
        return t

    def record(spec=((0, 1.0, 1.0), (1, 1.0, 1.0)), bias=None, lambdas=None, **kw):
        arr = (GibbsRelation * 1)()
        g = arr[0]
        g.rel, g.mean_value, g.alpha_dev, g.rel_tag, g.nnz = eng.rel[0].handle, rel.model.mean_value, alpha.data_ptr(), 1, n
        g.entity_of_mode[0], g.entity_of_mode[1] = 0, 1
        g.train, g.first_obs, g.obs_block, g.linear, g.bias_resid = train.handle, 0, n, lin.data_ptr(), resid.data_ptr()
        g.n_bias = len(spec)
        for k, t in enumerate(terms(spec, bias, lambdas)[:len(spec)]):
            g.bias[k] = t
        for k, v in kw.items():
            setattr(g, k, v)
        return arr

    def register(arr):
        check(lib().bdf_gibbs_set_relations(eng.gibbs, 1, C.cast(arr, C.c_void_p)))

    # the tail: what else the record carries, its counts, modes, priors and buffers
    for bad in (dict(probit=1), dict(censor=flags.data_ptr()), dict(interval=bounds.data_ptr()), dict(feat=op.handle, beta=beta.data_ptr()),
                dict(robust_nu=4.0, obs_precision=om.data_ptr()), dict(obs_precision=om.data_ptr()), dict(pg_model=1, obs_precision=om.data_ptr()),
                dict(bg_weight=0.1, bg_sums=sums.data_ptr()), dict(noise_mode=1, noise_shape=2.0, noise_rate=2.0, noise_tau=bu.data_ptr(), obs_precision=om.data_ptr()),
                dict(n_bias=3), dict(n_bias=-1), dict(train=None), dict(linear=None), dict(bias_resid=None), dict(test_baseline=tb.data_ptr()),
                dict(bias_test=train.handle)):
        with pytest.raises(B.ArgumentError, match="bias|n_bias"):
            register(record(**bad))
    for spec in (((0, 1.0, 1.0), (0, 1.0, 1.0)), ((2, 1.0, 1.0),), ((-1, 1.0, 1.0),), ((0, 0.0, 1.0),), ((0, float("nan"), 1.0),), ((1, 1.0, -1.0),),
                 ((1, 1.0, float("inf")),)):
        with pytest.raises(B.ArgumentError, match="bias"):
            register(record(spec=spec))
    with pytest.raises(B.ArgumentError, match="bias"):
        register(record(bias=[None, bv.data_ptr()]))
    with pytest.raises(B.ArgumentError, match="bias"):
        register(record(lambdas=[lam.data_ptr(), None]))
    with pytest.raises(B.ArgumentError, match="n_bias"):
        register(record(spec=(), bias_resid=resid.data_ptr()))           # a scratch buffer but no term
    # the two entry points
    facs = _facs(eng.factors_of(rel))
    small = B.DevicePairs(eng.ctx, ids[:-1], y[:-1])
    three = B.DevicePairs(eng.ctx, np.concatenate([ids, ids[:, :1]], axis=1), y)

    def draw(rel_h=eng.rel[0].handle, train_h=train.handle, D=8, fp=facs, a=1.0, a_dev=None, n_bias=2, t=terms(), sc=resid, out=lin):
        check(lib().bdf_bias_draw(eng.ctx.handle, rel_h, train_h, D, fp, 0.0, a, _p(a_dev), 1, n_bias, t, _p(sc), _p(out)))

    for bad in (dict(rel_h=None), dict(train_h=None), dict(fp=None), dict(t=None), dict(sc=None), dict(out=None), dict(D=0), dict(D=65),
                dict(a=0.0), dict(a=-1.0), dict(a=float("nan")), dict(a=float("inf")), dict(n_bias=0), dict(n_bias=3), dict(train_h=small.handle),
                dict(train_h=three.handle), dict(t=terms(((0, 1.0, 1.0), (0, 1.0, 1.0)))), dict(t=terms(((0, 1.0, 1.0), (2, 1.0, 1.0)))),
                dict(t=terms(((-1, 1.0, 1.0),)), n_bias=1), dict(t=terms(((0, 0.0, 1.0),)), n_bias=1), dict(t=terms(((0, 1.0, float("nan")),)), n_bias=1),
                dict(t=terms(((0, float("inf"), 1.0),)), n_bias=1), dict(t=terms(((0, 1.0, -2.0),)), n_bias=1),
                dict(t=terms(bias=[None, bv.data_ptr()])), dict(t=terms(lambdas=[None, lam.data_ptr()]))):
        with pytest.raises(B.ArgumentError, match="bdf_bias_draw"):
            draw(**bad)

    def baseline(pairs_h=train.handle, n_bias=2, t=terms(), out=tb):
        check(lib().bdf_bias_baseline(eng.ctx.handle, pairs_h, n_bias, t, 0.0, _p(out)))

    for bad in (dict(pairs_h=None), dict(t=None), dict(out=None), dict(n_bias=0), dict(n_bias=3), dict(t=terms(((1, 1.0, 1.0), (1, 1.0, 1.0)))),
                dict(t=terms(((2, 1.0, 1.0),)), n_bias=1), dict(t=terms(bias=[bu.data_ptr(), None]))):
        with pytest.raises(B.ArgumentError, match="bdf_bias_baseline"):
            baseline(**bad)
    baseline(t=terms(((0, 0.0, float("nan")), (1, -1.0, 0.0)), lambdas=[None, None]))    # of a term only mode and bias are read
    # a relation created with a layout holds only its own rows' cells
    from bdf_amd.engine import Layout
    sharded = B.DeviceRelation(eng.ctx, B.IndexedDF((ids, y), [60, 50]), [Layout(60, np.bincount(ids[:, 0] - 1, minlength=60), 2, 1),
                                                                         Layout(50, np.bincount(ids[:, 1] - 1, minlength=50), 2, 1)], 0)
    with pytest.raises(B.ArgumentError, match="layout"):
        draw(rel_h=sharded.handle)
    sharded.close()
    draw(a=0.0, a_dev=alpha)                                 # alpha_dev wins over the scalar
    register(record(alpha_sample=1, alpha_lambda0=1.0, alpha_nu0=2.0, bias_test=train.handle, test_baseline=tb.data_ptr()))
    eng.sweep(1)                                             # and the well-formed record is accepted: one iteration runs
    eng.sync()
    assert np.all(np.isfinite(rel.entities[0].model.sample))
    u, v, base = bu.cpu().numpy(), bv.cpu().numpy(), lin.cpu().numpy()
    assert np.all(np.isfinite(u)) and u.std() > 0 and v.std() > 0 and float(alpha.item()) != 1.0 and np.all(lam.cpu().numpy() > 0)
    assert np.array_equal(base, (rel.model.mean_value + u[ids[:, 0] - 1]) + v[ids[:, 1] - 1]) and np.array_equal(tb.cpu().numpy(), base)
    small.close(); three.close()
    op.close()
    train.close()
    eng.close()


# ---- (c) whole iterations -------------------------------------------------------------------------------------------------------
# (modes, D, alpha sampled, dense features on the first entity, the biased modes, 0-based): a covering choice -- every value of
# every factor, and every pair of values of two factors, occurs
CASES = [(2, 4, 0, 0, (1,)), (2, 4, 1, 1, (0, 1)), (2, 4, 0, 1, (0, 1)), (2, 4, 1, 0, (0,)), (2, 32, 1, 0, (0, 1)), (2, 32, 0, 1, (1,)),
         (3, 4, 1, 1, (2,)), (3, 4, 0, 0, (0, 1, 2)), (3, 32, 0, 0, (0,)), (3, 32, 1, 1, (0, 1, 2)), (3, 32, 1, 0, (0, 1, 2)), (3, 32, 0, 1, (1,))]
PRIOR = {0: (1.0, 1.0), 1: (1.5, 2.5), 2: (0.5, 0.75)}

CHILD = textwrap.dedent('''
    import sys
    import numpy as np
    sys.path.insert(0, %r); sys.path.insert(0, %r)
    import bdf_amd as B
    import bias_restatement as BR
    out, d = sys.argv[1], {}
    for n_modes, D, alpha_sample, with_feat, biased in %r:
        ids, y, dims, feats, n_test, alpha, _ = BR.iteration_case(n_modes, with_feat, alpha_sample)
        names = ["a", "b", "c"][:n_modes]
        ents = [B.Entity(nm, F=feats[k]) for k, nm in enumerate(names)]
        table = {nm: ids[:, k] for k, nm in enumerate(names)}
        table["y"] = y
        rel = B.Relation(table, "biased", ents, alpha=alpha, dims=list(dims))
        rel.model.alpha_sample = bool(alpha_sample)
        B.assignToTest(rel, np.arange(1, n_test + 1))
        for m in biased[::-1]:                                  # (in falling order: the step takes them rising all the same)
            B.setBias(rel, [ents[m], names[m], m + 1][(m + D) %% 3], *%r[m])      # by object, name or mode
        B.setWaic(rel)
        rd = B.RelationData(rel)
        res = B.macau(rd, num_latent=D, burnin=3, psamples=4, verbose=False, seed=91, lpd=True, rmse_train=True, full_prediction=True)
        key = "%%d_%%d_%%d%%d_%%s_" %% (n_modes, D, alpha_sample, with_feat, "".join(map(str, biased)))
        d[key + "native"], d[key + "pred"] = np.array(int(rd._engine.native)), res["predictions"]["pred"].to_numpy()
        d[key + "stdev"], d[key + "lpd"], d[key + "LPD"] = res["predictions"]["stdev"].to_numpy(), res["predictions"]["lpd"].to_numpy(), np.array(res["LPD"])
        d[key + "mean"], d[key + "alpha"] = np.array(rel.model.mean_value), np.array(rel.model.alpha)
        d[key + "waic"] = np.array([res["WAIC"][k] for k in ("waic", "elpd", "lppd", "p_waic", "se")])
        d[key + "rmse_train"], d[key + "full"], d[key + "RMSE"] = np.array(res["RMSE_train"]), res["predictions_full"], np.array(res["RMSE"])
        assert sorted(res["bias"]) == ["biased"] and sorted(res["bias"]["biased"]) == sorted(names[m] for m in biased)
        for m in biased:
            d[key + "b%%d" %% m] = rel._dev.bias[m].cpu().numpy()[:dims[m]]
            d[key + "bmean%%d" %% m], d[key + "lmean%%d" %% m] = res["bias"]["biased"][names[m]]["mean"], np.array(res["bias"]["biased"][names[m]]["precision"])
        d[key + "lam"] = rel._dev.bias_lambda.cpu().numpy()
        d[key + "probe"] = B.pred(rel, ids[:7])
        d[key + "train"] = B.pred(rel)
        for k, en in enumerate(rd.entities):
            d[key + "S%%d" %% k], d[key + "mu%%d" %% k], d[key + "Lam%%d" %% k] = en.model.sample.T, en.model.mu, en.model.Lambda
            if feats[k] is not None:
                d[key + "beta%%d" %% k], d[key + "lb%%d" %% k] = en.model.beta, np.array(en.lambda_beta)
        rd._engine.close()
    np.savez(out, **d)
''') % (ROOT, os.path.join(ROOT, "tests"), CASES, PRIOR)


@pytest.fixture(scope="module")
def chains():
    """seven iterations of every case of CASES on the native and on the step-by-step path: one child process per path"""
    return child(CHILD, no_native=False), child(CHILD, no_native=True)


@pytest.mark.parametrize("n_modes,D,alpha_sample,with_feat,biased", CASES)
def test_whole_iterations_match_the_restated_chain_on_both_paths(chains, n_modes, D, alpha_sample, with_feat, biased):
    """macau(lpd=True, rmse_train=True, full_prediction=True) with setWaic, burnin 3 + 4 draws, matrix 37 x 23 and tensor 37 x 23 x
    11, 600 training and 200 test cells.  The factors, the hyperparameters, the biases and their precisions (the last draw and the
    posterior means of result["bias"]), alpha, predictions, stdev, lpd, WAIC, RMSE_train, the full prediction and pred() are held
    to 1e-9 relative / 1e-6, as the chain tests of the other models are (tests/test_gpu_dense.py, test_gpu_nonneg.py); the two
    iteration paths give the same bits."""
    ids, y, dims, feats, n_test, alpha, _ = BR.iteration_case(n_modes, with_feat, alpha_sample)
    key = "%d_%d_%d%d_%s_" % (n_modes, D, alpha_sample, with_feat, "".join(map(str, biased)))
    nat, step = ({k[len(key):]: v for k, v in ch.items() if k.startswith(key)} for ch in chains)
    assert nat["native"] == 1 and step["native"] == 0
    assert sorted(nat) == sorted(step) and len(nat) >= 14 + 3 * n_modes + 3 * len(biased)
    for k in nat:
        if k != "native":
            assert np.array_equal(nat[k], step[k]), k       # the two paths enqueue the same launches: the same bits
    spec = {m: PRIOR[m] for m in biased}
    tr, te = ids[n_test:], ids[:n_test]
    ref = BR.run_chain(tr, y[n_test:], dims, D, 91, 7, spec=spec, alpha=alpha, alpha_sample=alpha_sample, feats=feats, test_ids=te,
                       test_values=y[:n_test], burnin=3, waic=True, train_pred=True)
    tol = dict(rtol=1e-9, atol=1e-6)
    assert abs(nat["mean"] - ref["mean"]) <= 1e-12
    np.testing.assert_allclose(nat["alpha"], ref["alpha"], rtol=1e-9)
    assert (nat["alpha"] != alpha) == bool(alpha_sample)
    for k in range(n_modes):
        np.testing.assert_allclose(nat["S%d" % k], ref["S"][k], err_msg="sample of entity %d" % k, **tol)
        np.testing.assert_allclose(nat["mu%d" % k], ref["mu"][k], **tol)
        np.testing.assert_allclose(nat["Lam%d" % k], ref["Lam"][k], **tol)
        if feats[k] is not None:
            np.testing.assert_allclose(nat["beta%d" % k], ref["beta"][k], err_msg="beta of entity %d" % k, **tol)
            np.testing.assert_allclose(nat["lb%d" % k], ref["lb"][k], **tol)
    for t, m in enumerate(sorted(biased)):
        np.testing.assert_allclose(nat["b%d" % m], ref["bias"][m], err_msg="bias of mode %d" % m, **tol)
        np.testing.assert_allclose(nat["bmean%d" % m], ref["bias_mean"][m], **tol)
        np.testing.assert_allclose(nat["lam"][t], ref["lambda"][m], **tol)
        np.testing.assert_allclose(nat["lmean%d" % m], ref["lambda_mean"][m], **tol)
        assert np.abs(nat["b%d" % m]).max() > 0.1
    np.testing.assert_allclose(nat["pred"], ref["pred"], **tol)
    np.testing.assert_allclose(nat["stdev"], ref["stdev"], **tol)
    assert np.all(np.isfinite(nat["lpd"])) and len(nat["lpd"]) == n_test
    np.testing.assert_allclose(nat["lpd"], ref["lpd"], **tol)
    np.testing.assert_allclose(nat["LPD"], ref["LPD"], **tol)
    np.testing.assert_allclose(nat["RMSE"], np.sqrt(np.mean((ref["pred"] - y[:n_test]) ** 2)), **tol)
    w = ref["WAIC"]
    np.testing.assert_allclose(nat["waic"], [w["waic"], w["elpd"], w["lppd"], w["p_waic"], w["se"]], **tol)
    np.testing.assert_allclose(nat["rmse_train"], np.sqrt(np.mean((y[n_test:] - ref["train_pred"]) ** 2)), **tol)
    np.testing.assert_allclose(nat["full"], ref["full"], **tol)
    # pred(r) and pred(r, probe) carry the last draw's biases
    from probit_restatement import udot
    np.testing.assert_allclose(nat["train"], udot(tr, ref["S"]) + BR.base(tr, ref["bias"], ref["mean"]), **tol)
    np.testing.assert_allclose(nat["probe"], udot(ids[:7], ref["S"]) + BR.base(ids[:7], ref["bias"], ref["mean"]), **tol)
    # and the model matters: the Gaussian chain on the same data is somewhere else, in its rows and in its score
    gauss = BR.run_chain(tr, y[n_test:], dims, D, 91, 7, alpha=alpha, alpha_sample=alpha_sample, feats=feats, test_ids=te,
                         test_values=y[:n_test], burnin=3)
    assert np.abs(gauss["S"][0] - ref["S"][0]).max() > 1e-3 and abs(gauss["LPD"] - ref["LPD"]) > 1e-3


def test_verbose_line_a_second_relation_and_a_reused_engine(B, capsys):
    """the verbose line gains the rms of the current draw per biased entity of the first relation; two relations carry biases of
    their own; the relation WITHOUT biases beside a biased one keeps linear_values == NULL in its row terms; macau() on a reused
    engine restarts the running sums"""
    import re
    ids, y, dims, feats, n_test, alpha, _ = BR.iteration_case(2, 0, 0)

    def run(which, again=False):
        a, b, c = B.Entity("a"), B.Entity("b"), B.Entity("c")
        r1 = B.Relation({"a": ids[:, 0], "b": ids[:, 1], "y": y}, "one", [a, b], alpha=alpha, dims=list(dims))
        r2 = B.Relation({"a": ids[:, 0], "c": (ids[:, 1] - 1) % 12 + 1, "y": y[::-1].copy()}, "two", [a, c], alpha=alpha, dims=[dims[0], 12])
        B.assignToTest(r1, np.arange(1, n_test + 1))
        if 1 in which:
            B.setBias(r1, "a")
            B.setBias(r1, "b", 2.0, 0.5)
        if 2 in which:
            B.setBias(r2, "c")
        rd = B.RelationData(r1)
        B.addRelation(rd, r2)
        res = B.macau(rd, num_latent=4, burnin=1, psamples=2, verbose=True, seed=5)
        eng = rd._engine
        lin = [[t.linear_values for t in eng._terms(j)] for j in range(3)]
        if again:
            res2 = B.macau(rd, num_latent=4, burnin=0, psamples=1, verbose=False, seed=5, engine=eng, reset_model=False)
            cur = {nm: r1._dev.bias[m].cpu().numpy()[:dims[m]] for m, nm in ((0, "a"), (1, "b"))}
            for nm in ("a", "b"):                             # one draw since the restart: its mean is that draw
                assert np.array_equal(res2["bias"]["one"][nm]["mean"], cur[nm])
        S = rd.entities[0].model.sample.copy()
        eng.close()
        return res, S, lin

    res0, S0, lin0 = run(())
    assert " b:" not in capsys.readouterr().out and "bias" not in res0 and all(x is None for row in lin0 for x in row)
    res1, S1, lin1 = run((1,), again=True)
    lines = [t for t in capsys.readouterr().out.splitlines() if "RMSE=" in t]
    assert len(lines) == 3 and all(re.search(r" b:\d+\.\d{3} b:\d+\.\d{3} \| ", t) for t in lines), lines
    assert sorted(res1["bias"]) == ["one"] and len(res1["bias"]["one"]["a"]["mean"]) == dims[0] and res1["bias"]["one"]["b"]["precision"] > 0
    # entity a: terms (one, two); b: (one); c: (two) -- only the biased relation's terms carry a base per cell
    assert lin1[0][0] is not None and lin1[0][1] is None and lin1[1][0] is not None and lin1[2][0] is None
    res2, S2, lin2 = run((2,))
    assert not re.search(r" b:\d", capsys.readouterr().out)          # the line shows the rms of the first relation's (two[... b:c] names the entity)
    assert sorted(res2["bias"]) == ["two"] and sorted(res2["bias"]["two"]) == ["c"]
    assert lin2[0][0] is None and lin2[0][1] is not None and lin2[1][0] is None and lin2[2][0] is not None
    res3, S3, _ = run((1, 2))
    assert sorted(res3["bias"]) == ["one", "two"]
    assert np.abs(S2 - S0).max() > 1e-3 and np.abs(S1 - S0).max() > 1e-3 and np.abs(S3 - S1).max() > 1e-3


# ---- (d) nothing else moved -------------------------------------------------------------------------------------------------
GAUSS = textwrap.dedent('''
    import sys
    import numpy as np
    sys.path.insert(0, %r); sys.path.insert(0, %r)
    import bdf_amd as B
    import bias_restatement as BR
    ids, y, _, _, n_test, alpha = BR.planted(seed=5, N1=120, N2=90, n_train=3500, n_test=500)

    def gaussian():
        rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y + 0.25 * ids[:, 0] %% 3}, "g", [B.Entity("u"), B.Entity("v")], dims=[120, 90])
        B.assignToTest(rel, np.arange(4000 - n_test + 1, 4001))
        rd = B.RelationData(rel)
        res = B.macau(rd, num_latent=16, burnin=2, psamples=2, verbose=False, seed=17, lpd=True)
        assert "bias" not in res and rel._dev.bias is None and rel._dev.linear is None and rel._dev.train is None
        out = [en.model.sample.copy() for en in rd.entities] + [res["predictions"]["pred"].to_numpy().copy(), res["predictions"]["lpd"].to_numpy().copy()]
        rd._engine.close()
        return out

    if sys.argv[2] == "beside":
        rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "p", [B.Entity("u"), B.Entity("v")], dims=[120, 90])
        B.assignToTest(rel, np.arange(4000 - n_test + 1, 4001))
        B.setBias(rel, "u"); B.setBias(rel, "v")
        rdb = B.RelationData(rel)
        res = B.macau(rdb, num_latent=16, burnin=1, psamples=1, verbose=False, seed=17, lpd=True)
        assert len(res["bias"]["p"]["v"]["mean"]) == 90 and np.abs(res["bias"]["p"]["v"]["mean"]).max() > 0.1
    got = gaussian()                                          # (beside: the engine with biases is alive)
    np.savez(sys.argv[1], *got)
''') % (ROOT, os.path.join(ROOT, "tests"))


def test_gaussian_chain_is_untouched_by_an_engine_with_biases_in_the_process():
    """a Gaussian chain run after an engine with biases has run, in one process, equals the same chain from a fresh process byte
    for byte: factors, predictions and lpd"""
    alone, beside = child(GAUSS, "alone", no_native=False), child(GAUSS, "beside", no_native=False)
    assert sorted(alone) == sorted(beside) and len(alone) == 4
    for k in alone:
        assert alone[k].tobytes() == beside[k].tobytes(), k


# ---- (e) planted biases -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0])
def test_planted_biases(B, seed):
    """150 x 100, rank 3 with loadings of sd 0.5, a_i and b_j ~ N(0, 1), noise sd 0.3, 4,500 training and 1,500 held-out cells; D = 8,
    60 + 60 iterations, alpha = 1 / 0.3^2 fixed, both entities biased with the default prior.  The held-out RMSE is below the mean
    predictor's and the posterior-mean biases, centred per entity, are closer to the planted ones (centred) than zero is: their RMS
    error is below the planted sd, 1.  The restated chain on the CPU (BR.run_chain, planted seeds 0, 1, 2, chain seed 1) holds both: RMSE 0.334, 0.350, 0.354 against
    the mean predictor's 1.490, 1.518, 1.590, and RMS errors 0.103 / 0.077, 0.079 / 0.137, 0.109 / 0.167."""
    ids, y, a, b, n_test, alpha = BR.planted(seed)
    n = len(y)
    rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "planted", [B.Entity("u"), B.Entity("v")], alpha=alpha, dims=[150, 100])
    B.assignToTest(rel, np.arange(n - n_test + 1, n + 1))
    B.setBias(rel, "u")
    B.setBias(rel, "v")
    rd = B.RelationData(rel)
    res = B.macau(rd, num_latent=8, burnin=60, psamples=60, verbose=False, seed=1)
    rd._engine.close()
    held = y[-n_test:]
    rmse_mean = float(np.sqrt(np.mean((held - y[:-n_test].mean()) ** 2)))
    eu, ev = BR.centred_rms(res["bias"]["planted"]["u"]["mean"], a), BR.centred_rms(res["bias"]["planted"]["v"]["mean"], b)
    print(f"planted biases, seed {seed}: held-out RMSE {res['RMSE']:.4f} (mean predictor {rmse_mean:.4f}), centred RMS error of the biases "
          f"{eu:.4f} (rows), {ev:.4f} (columns), posterior mean precisions {res['bias']['planted']['u']['precision']:.3f}, "
          f"{res['bias']['planted']['v']['precision']:.3f}")
    assert res["RMSE"] < rmse_mean, (res["RMSE"], rmse_mean)
    assert eu < 1.0 and ev < 1.0, (eu, ev)
