"""Every handle of the library gives back the device and pinned host memory it took (csrc/dev_buf.h; bdf_dev_live).

Each case reads bdf_dev_live -- the blocks, and their bytes as requested, that the library's own objects hold in this process --
creates a context of its own (what the context caches is then inside the measurement), builds the handle, drives each of its
lazily allocating and replacing paths at the smallest shapes that reach them, destroys everything and reads bdf_dev_live again:
blocks and bytes must equal the first reading exactly.  For the replacing paths the second and third identical call leave the
block count where the first left it.  No case provokes an error on the device: the failure side is tests/test_dev_buf_host.py's.
"""
import contextlib
import ctypes as C
import gc

import numpy as np
import pytest

from test_gpu_features import _colmajor, _sample_beta
from test_gpu_foldin import _foldin, _known_relation, _spd
from test_gpu_rows import _dev_terms, _run_rows
from test_gpu_rows_col import _ragged

pytestmark = pytest.mark.gpu


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _live():
    from bdf_amd._lib import check, lib
    blocks, nbytes = C.c_int64(-1), C.c_int64(-1)
    check(lib().bdf_dev_live(C.byref(blocks), C.byref(nbytes)))
    return blocks.value, nbytes.value


@contextlib.contextmanager
def _returns_all():
    """the body's handles, its contexts included, give back exactly what they took (checked when the body ends without an error)"""
    gc.collect()                                  # (handles that earlier tests dropped go now, not in the middle of the measurement)
    base = _live()
    assert base[0] >= 0 and base[1] >= 0
    yield base
    gc.collect()
    assert _live() == base, (_live(), base)


@contextlib.contextmanager
def _fresh_context(B, seed=77):
    with _returns_all() as base:
        ctx = B.Context(seed=seed)
        try:
            assert _live() == (base[0] + 2, base[1] + 4 + 64)          # the iteration counter and the flag words
            yield ctx
        finally:
            ctx.close()


def _unchanged_after_the_first(call, times=3):
    """`call` three times: the second and the third leave the block count where the first left it"""
    call()
    blocks = _live()[0]
    for _ in range(times - 1):
        call()
        assert _live()[0] == blocks
    return blocks


# ---- ctx ------------------------------------------------------------------------------------------------------------------------------
def test_context_gives_back_its_lazily_allocated_buffers(B):
    from bdf_amd._lib import check, lib
    rng = np.random.default_rng(1)
    with _fresh_context(B) as ctx:
        # scratch and scratch2: F'(F X) + lambda X of a dense F (the product's intermediate; the split sums of F' B)
        Fd = rng.standard_normal((300, 40))
        op = B.FeatOperator(ctx, Fd)
        before = _live()[0]
        _unchanged_after_the_first(lambda: op.AtA_mul(_colmajor(ctx, rng.standard_normal((40, 5))), 0.1))
        ctx.sync()
        assert _live()[0] == before + 2
        # cg_status (and, the operator being F'F of 140 features, the one-launch solve's counter cg_bar); cg_part: 2,600 sparse columns
        before = _live()[0]
        opd = B.FeatOperator(ctx, rng.standard_normal((300, 140)))
        D = 8
        Lam = _spd(rng, D)
        _sample_beta(B, ctx, opd, D, rng.standard_normal((300, D)), np.zeros(D), Lam, 0.75, False, None)
        import scipy.sparse as sp
        S = sp.random(3000, 2600, density=9 / 2600, random_state=4, format="coo")
        ops = B.FeatOperator(ctx, S)
        _sample_beta(B, ctx, ops, 6, rng.standard_normal((3000, 6)), np.zeros(6), _spd(rng, 6), 0.75, False, None)
        assert _live()[0] >= before + 3
        for o in (op, opd, ops):
            o.close()
        # lr_T, lr_mrows and lr_vt: a low-rank row launch with a prior mean per row
        D, dims = 32, [211, 90]
        deg = rng.integers(0, 18, dims[0])
        rows = np.repeat(np.arange(1, dims[0] + 1), deg)
        ids = np.stack([rows, rng.integers(1, dims[1] + 1, len(rows))], axis=1).astype(np.int64)
        vals = rng.integers(1, 6, len(rows)).astype(np.float64)
        dr = B.DeviceRelation(ctx, B.IndexedDF((ids, vals), dims))
        V = ctx.tensor(rng.standard_normal((dims[1], D)) * 0.5)
        terms = _dev_terms(B, ctx, [(dr, 0, 1.7, float(vals.mean()), [None, V], None)])
        Lam_t, mu_rows = ctx.tensor(_spd(rng, D)), ctx.tensor(rng.standard_normal((dims[0], D)))
        out = ctx.zeros(dims[0], D)
        ctx.set_lowrank(-1, 0)
        ctx.set_sweep(3)
        before = _live()[0]
        _unchanged_after_the_first(lambda: _run_rows(B, ctx, D, dims[0], terms, mu_rows, Lam_t, 5, out))
        assert ctx.rows_dispatch(5)["lowrank"] > 0
        assert _live()[0] >= before + 3
        dr.close()
        # norm_part and newrows_W
        before = _live()[0]
        x, res = ctx.tensor(rng.standard_normal(5000)), ctx.zeros(1)
        _unchanged_after_the_first(lambda: check(lib().bdf_norm2(ctx.handle, 5000, _p(x), _p(res))))
        q = ctx.zeros(90)
        _unchanged_after_the_first(lambda: check(lib().bdf_newrows_quad(ctx.handle, D, 90, _p(Lam_t), _p(V), _p(q))))
        ctx.sync()
        assert abs(res.item() - np.linalg.norm(x.cpu().numpy())) <= 1e-9
        assert _live()[0] == before + 2


# ---- rel ------------------------------------------------------------------------------------------------------------------------------
def test_relations_give_back_their_index(B):
    rng = np.random.default_rng(2)
    with _fresh_context(B) as ctx:
        base = _live()[0]
        nnz = 900
        ids2 = np.stack([rng.integers(1, 41, nnz), rng.integers(1, 31, nnz)], axis=1).astype(np.int64)
        ids3 = np.concatenate([ids2, rng.integers(1, 8, (nnz, 1))], axis=1).astype(np.int64)
        # per mode rowptr, colidx, vals, perm, order; with at most 256 distinct values the packed plane too, and the table once
        for ids, dims, vals, blocks in ((ids2, [40, 30], rng.integers(1, 6, nnz).astype(np.float64), 13),
                                        (ids2, [40, 30], rng.standard_normal(nnz), 10),
                                        (ids3, [40, 30, 7], rng.standard_normal(nnz), 15)):
            dr = B.DeviceRelation(ctx, B.IndexedDF((ids, vals), dims))
            assert _live()[0] == base + blocks
            dr.close()
            assert _live()[0] == base


# ---- rows plans -----------------------------------------------------------------------------------------------------------------------
def test_row_plans_and_gather_images_go_with_their_relation_and_context(B):
    rng = np.random.default_rng(3)
    with _fresh_context(B) as ctx:
        dims = [203, 90]
        ids, vals, deg = _ragged(rng, dims, [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 150, 700, 2, 48, 49], 120, True)
        dr = B.DeviceRelation(ctx, B.IndexedDF((ids, vals), dims))
        with_relation = _live()[0]
        N = dims[0]

        def launch(D, tag, per_row=False):
            V = ctx.tensor(rng.standard_normal((dims[1], D)) * 0.5)
            terms = _dev_terms(B, ctx, [(dr, 0, 1.7, float(vals.mean()), [None, V], None)])
            Lam_t = ctx.tensor(_spd(rng, D))
            mu_t = ctx.tensor(rng.standard_normal((N, D)) if per_row else rng.standard_normal(D))
            out = ctx.zeros(N, D)
            sweeps = iter((4, 5, 6))                           # (the dispatch report adds up the launches of one iteration number)

            def once():
                ctx.set_sweep(next(sweeps))
                _run_rows(B, ctx, D, N, terms, mu_t, Lam_t, tag, out)
            _unchanged_after_the_first(once)
            assert ctx.rows_unfinished() == 0
            return ctx.rows_dispatch(tag)

        ctx.set_lowrank(0, 0)
        ctx.set_small_rows(0, 1)
        d = launch(10, 1)                                      # the wave-per-row kernel: every row, the long ones in items
        assert d["k1"] == N and d["k1_items"] > N and d["small"] == d["lowrank"] == d["col"] == 0
        ctx.set_small_rows(48, 1)
        d = launch(10, 2)                                      # short rows four to a wave
        assert d["small"] > 0 and d["k1"] > 0
        ctx.set_lowrank(-1, 0)
        ctx.set_col_rows(0)
        d = launch(40, 3, per_row=True)                        # the low-rank sampler
        assert d["lowrank"] > 0 and d["col"] == 0
        ctx.set_lowrank(0, 0)
        ctx.set_col_rows(16)
        d = launch(24, 4)                                      # the column layout, the 700-observation row spans waves
        assert d["col"] == N and d["col_waves"] > 0 and d["k1"] == 0
        # D = 32: the gather image, the pair tier, then the full one -- switching the tier makes the image anew
        for tier in (1, 2, 1):
            ctx.set_gather_image(tier)
            seen = ctx.gather_image_stats()["launches"]
            d = launch(32, 5)
            assert d["col"] == N and ctx.gather_image_stats()["launches"] == seen + 3
        assert _live()[0] > with_relation
        dr.close()                                             # the relation's plans go with it; the images with the context


# ---- pairs ----------------------------------------------------------------------------------------------------------------------------
def test_pairs_give_back_their_running_states(B):
    from bdf_amd._lib import check, lib
    rng = np.random.default_rng(4)
    with _fresh_context(B) as ctx:
        D, n_new, M, n = 16, 13, 60, 300
        ids = np.stack([rng.integers(1, n_new + 1, n), rng.integers(1, 51, n)], axis=1)
        y = rng.standard_normal(n)
        U, V = ctx.tensor(rng.standard_normal((n_new, D)) * 0.6), ctx.tensor(rng.standard_normal((M, D)) * 0.6)
        Lam = _spd(rng, D)
        base = _live()[0]
        pairs = B.DevicePairs(ctx, ids, y)
        assert _live()[0] == base + 4                          # ids, values, avg, sq
        pairs.sort(1)
        assert _live()[0] == base + 5                          # the order
        pairs.update(D, [U, V], 0.1, 1, (), 0.0)
        grown = _live()[0]
        _unchanged_after_the_first(lambda: pairs.auc(0.0))
        _unchanged_after_the_first(lambda: pairs.lpd_update(D, [U, V], 0.1, 2.0, 1))
        _unchanged_after_the_first(lambda: pairs.waic_update(D, [U, V], 0.1, 2.0, 1))
        qt, stats = ctx.tensor(np.einsum("md,dk,mk->m", V.cpu().numpy(), np.linalg.inv(Lam), V.cpu().numpy())), ctx.zeros(8)
        _unchanged_after_the_first(lambda: check(lib().bdf_newrows_update(ctx.handle, pairs.handle, D, _p(U), _p(V), _p(qt), 0.1, 2.0, None, 1,
                                                                          1.0, -1.0, 0.0, 1, _p(stats))))
        ctx.sync()
        assert _live()[0] >= grown + 4                         # the AUC workspace and the three running states (the context's scratch may grow too)
        assert np.isfinite(pairs.lpd()).all() and np.isfinite(pairs.waic()[0]).all()
        # the fold-in's row pointer: made for (rows, columns), made again for other columns
        cells = B.DevicePairs(ctx, ids, np.zeros(n))
        cells.sort(0)
        Lt, mu_t = ctx.tensor(Lam), ctx.tensor(rng.standard_normal(D) * 0.4)
        blocks = None
        for cols in (50, 60, 50):
            kid = np.stack([rng.integers(1, n_new + 1, 40), rng.integers(1, cols + 1, 40)], axis=1)
            rel = _known_relation(B, ctx, kid, rng.standard_normal(40), n_new, cols)
            Vt = ctx.tensor(rng.standard_normal((cols, D)) * 0.5)
            _unchanged_after_the_first(lambda: _foldin(B, ctx, D, n_new, rel, Vt, mu_t, False, Lt, cells, 0.3, 2.0))
            rel.close()
            assert blocks is None or _live()[0] == blocks      # the pointer was replaced, not added
            blocks = _live()[0]
        cells.close()
        pairs.close()


# ---- feat -----------------------------------------------------------------------------------------------------------------------------
def test_feature_operators_give_back_their_workspaces(B):
    from bdf_amd._lib import check, lib
    import scipy.sparse as sp
    from bdf_amd import _lib
    rng = np.random.default_rng(5)
    with _fresh_context(B) as ctx:
        base = _live()[0]
        # dense
        op = B.FeatOperator(ctx, rng.standard_normal((120, 37)))
        assert _live()[0] == base + 1
        # ... its row ids, set three times and cleared
        for k in range(3):
            ids = rng.permutation(120).astype(np.int32)
            check(lib().bdf_feat_set_row_ids(op.handle, ids.ctypes.data_as(_lib.c_i32p)))
            assert _live()[0] == base + 2
        check(lib().bdf_feat_set_row_ids(op.handle, None))
        assert _live()[0] == base + 1
        op.mul(_colmajor(ctx, rng.standard_normal((37, 5))))
        ctx.sync()
        op.close()
        # csr through F'F: densified once, F'F, and the blocked solve's workspace, which grows with the columns of the solve
        S = sp.random(700, 650, density=0.02, random_state=6, format="coo")
        op = B.FeatOperator(ctx, S)
        made, held = _live()[0], {}
        for D in (4, 8):
            blocks = _unchanged_after_the_first(lambda: _sample_beta(B, ctx, op, D, rng.standard_normal((700, D)), np.zeros(D), _spd(rng, D), 0.75, True, None))
            held[D] = _live()[1]
            assert blocks >= made + 3                          # dense, F'F, the workspace
        assert held[8] > held[4]                               # the workspace of eight columns took the place of that of four
        op.close()
        # the eigen path (64 < features <= 640) at two widths: Q, the eigenvalues, and the workspace that is replaced at the larger D
        op = B.FeatOperator(ctx, rng.standard_normal((200, 100)))
        made, held = _live()[0], {}
        for D in (4, 8):
            blocks = _unchanged_after_the_first(lambda: _sample_beta(B, ctx, op, D, rng.standard_normal((200, D)), np.zeros(D), _spd(rng, D), 0.75, True, None))
            held[D] = _live()[1]
            assert blocks >= made + 4                          # F'F, Q, the eigenvalues, the workspace
        assert held[8] > held[4]
        op.close()
        # a binary matrix wide enough for column panels (more than 12,288 columns), its rows' entries in column order
        m, n, per = 2000, 13000, 6
        rows = np.repeat(np.arange(m), per)
        cols = np.concatenate([np.sort(rng.choice(n, per, replace=False)) for _ in range(m)])
        before = _live()[0]
        op = B.FeatOperator(ctx, B.SparseBinMatrix(m, n, rows + 1, cols + 1))
        assert _live()[0] == before + 5                        # two pointers, two index planes, the forward panels
        got = op.mul(_colmajor(ctx, np.ones((n, 1)))).cpu().numpy()
        assert np.array_equal(got.ravel(), np.full(m, float(per)))
        op.close()


# ---- gibbs ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reserve", [0, 8])
def test_the_iteration_object_gives_back_its_contexts_events_and_counters(B, monkeypatch, reserve):
    """reserve 0: events everywhere; 8: the rows' hand-over by counter (done_dev) and the gate's context.  The relation samples its
    precision, so it is registered with the object (rel_sse); the small entities' hyperprior runs as the one-launch chain (hyper_count)"""
    monkeypatch.setenv("BDF_RESERVE_CUS", str(reserve))
    rng = np.random.default_rng(6)
    with _returns_all() as base:
        Nu, Nv, nnz, D = 300, 200, 4000, 16
        ids = np.stack([rng.integers(1, Nu + 1, nnz), rng.integers(1, Nv + 1, nnz)], axis=1)
        rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": rng.standard_normal(nnz)}, "r", [B.Entity("u"), B.Entity("v")], dims=[Nu, Nv])
        B.assignToTest(rel, np.arange(1, 301))
        rel.model.alpha_sample = True
        eng = B.GibbsEngine(B.RelationData(rel), D, seed=9)
        try:
            assert eng.native and _live()[0] > base[0]
            for i in (1, 2, 3):
                eng.sweep(i)
            eng.sync()
        finally:
            eng.close()


# ---- vb, hmc --------------------------------------------------------------------------------------------------------------------------
def _two_mode_data(B, rng, Nu=60, Nv=40, nnz=700, n_test=90):
    ids = np.stack([rng.integers(1, Nu + 1, nnz), rng.integers(1, Nv + 1, nnz)], axis=1)
    rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": rng.standard_normal(nnz)}, "r", [B.Entity("u"), B.Entity("v")], dims=[Nu, Nv])
    B.assignToTest(rel, np.arange(1, n_test + 1))
    B.setPrecision(rel, 2.0)
    return B.RelationData(rel), (Nu, Nv)


def test_the_vb_trainer_gives_back_its_model(B):
    from bdf_amd import _lib, _two_mode
    lib, check = _lib.lib(), _lib.check
    rng = np.random.default_rng(7)
    rd, (Nu, Nv) = _two_mode_data(B, rng)
    D = 8
    mu = [np.ascontiguousarray(rng.standard_normal((n, D)) * 0.1) for n in (Nu, Nv)]
    with _returns_all() as base:
        extra = (2.0, mu[0].ctypes.data_as(_lib.c_dp), mu[1].ctypes.data_as(_lib.c_dp))
        with _two_mode.trainer(rd, D, lib.bdf_vb_create, lib.bdf_vb_destroy, extra, seed=3, device=None) as (h, test):
            check(lib.bdf_vb_set_test(h, test, 1.0, -1.0))
            _unchanged_after_the_first(lambda: check(lib.bdf_vb_iterate(h, 1)))
            st = np.zeros(4)
            check(lib.bdf_vb_stats(h, st.ctypes.data_as(_lib.c_dp)))
            assert np.isfinite(st).all() and _live()[0] > base[0] + 20


def test_the_hmc_trainer_gives_back_its_model_and_what_it_regrows(B):
    from bdf_amd import _lib, _two_mode
    lib, check = _lib.lib(), _lib.check
    rng = np.random.default_rng(8)
    rd, _ = _two_mode_data(B, rng)
    with _returns_all() as base:
        with _two_mode.trainer(rd, 8, lib.bdf_hmc_create, lib.bdf_hmc_destroy, (2.0,), seed=3, device=None) as (h, test):
            made = _live()
            # the test pairs' running mean and partial sums: set three times, replaced each time
            _unchanged_after_the_first(lambda: check(lib.bdf_hmc_set_test(h, test, 1.0, -1.0)))
            assert _live()[0] == made[0] + 2
            # a larger L regrows the partial sums, the record and its pinned copy: the same blocks, more bytes
            seen = {}
            for L in (3, 12, 12, 30):
                check(lib.bdf_hmc_set_params(h, L, 1, 8, 0.01, 100))
                check(lib.bdf_hmc_iterate(h, 1))
                st = np.zeros(16)
                check(lib.bdf_hmc_stats(h, st.ctypes.data_as(_lib.c_dp), None, 0))
                assert np.isfinite(st[:14]).all()
                seen[L] = _live()
                assert seen[L][0] == seen[3][0]
            assert seen[3][1] < seen[12][1] < seen[30][1]


# ---- ordinal --------------------------------------------------------------------------------------------------------------------------
def test_the_ordinal_edges_give_back_their_state(B):
    import torch
    import ordinal_restatement as OR
    with _fresh_context(B) as ctx:
        D, K = 8, 5
        ids, S, mean, codes, dims = OR.step_case(D, 2, K)
        pairs = B.DevicePairs(ctx, ids, codes.astype(np.float64))
        St = [ctx.tensor(s) for s in S]
        cd, bd = ctx.tensor(codes, dtype=torch.int8), ctx.tensor(OR.bounds_of(codes, OR.start_edges(K)))
        before = _live()
        o = B.DeviceOrdinal(ctx, K, OR.STEP_START, 3)
        assert _live() == (before[0] + 1, before[1] + (48 + 3 * (K - 1)) * 8)
        ctx.set_sweep(OR.STEP_SWEEPS[0])
        o.step(ctx, pairs, cd, D, St, mean, OR.STEP_ALPHA, 1, 1, bd)
        assert np.isfinite(o.read(1)["S"])
        o.close()
        pairs.close()


# ---- scores, acquire ------------------------------------------------------------------------------------------------------------------
def _draws(ctx, rng, N, M, D, n):
    return [(ctx.tensor(rng.standard_normal((N, D)) * 0.5), ctx.tensor(rng.standard_normal((M, D)) * 0.5)) for _ in range(n)]


def test_scores_give_back_their_sum_ring_and_relevance_lists(B):
    from bdf_amd.engine import DeviceScores
    rng = np.random.default_rng(10)
    with _fresh_context(B) as ctx:
        N, M, D, K = 37, 90, 12, 5
        ids = np.stack([rng.integers(1, N + 1, 400), rng.integers(1, M + 1, 400)], axis=1).astype(np.int64)
        rel = B.DeviceRelation(ctx, B.IndexedDF((ids, rng.standard_normal(400)), [N, M]))
        test = B.DevicePairs(ctx, np.stack([rng.integers(1, N + 1, 200), rng.integers(1, M + 1, 200)], axis=1), rng.standard_normal(200))
        for rows0 in (None, np.array([3, 0, 11, 36], dtype=np.int32)):
            base = _live()[0]
            sc = DeviceScores(ctx, N if rows0 is None else len(rows0), M, D, 3, rows0)
            assert _live()[0] == base + (2 if rows0 is None else 3)           # the sum, the ring, the scored rows
            for U, V in _draws(ctx, rng, N, M, D, 4):
                sc.push(U, V)
            lists = []
            _unchanged_after_the_first(lambda: lists.append(sc.topk(K, 0.2, rel)))
            items = lists[0][0]
            assert all(np.array_equal(items.cpu().numpy(), l[0].cpu().numpy()) for l in lists)
            made = _unchanged_after_the_first(lambda: sc.metrics(items, K, test, 0.0))
            assert made >= base + (2 if rows0 is None else 3) + 3              # the lists' pointer and items, the rows' metrics
            sc.metrics(items, K, test, 0.5)                                    # another cut: the lists are replaced
            ctx.sync()
            assert _live()[0] == made
            sc.close()
        test.close()
        rel.close()


def test_acquire_gives_back_every_plane(B):
    from bdf_amd.engine import DeviceAcquire
    rng = np.random.default_rng(11)
    with _fresh_context(B) as ctx:
        N, M, D, K = 37, 90, 12, 5
        ids = np.stack([rng.integers(1, N + 1, 400), rng.integers(1, M + 1, 400)], axis=1).astype(np.int64)
        rel = B.DeviceRelation(ctx, B.IndexedDF((ids, rng.standard_normal(400)), [N, M]))
        for threshold, planes in ((None, 3), (0.3, 4)):
            base = _live()
            ac = DeviceAcquire(ctx, N, M, D, 3, None, 0.2, threshold)
            cells = (N * M + 64) * 8
            assert _live()[0] == base[0] + planes + 1 and _live()[1] >= base[1] + planes * cells
            for U, V in _draws(ctx, rng, N, M, D, 4):
                ac.push(U, V, 2.0)
            for rule in ("ucb", "sd") + (("prob_above",) if threshold is not None else ()):
                outs = []
                _unchanged_after_the_first(lambda: outs.append(ac.topk(K, rule, 1.0, rel)))
                assert np.isfinite(outs[0]["scores"].cpu().numpy()[:, 0]).all()
            ac.close()
        rel.close()
