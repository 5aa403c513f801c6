"""The fold-in of new rows from a few cells of their own on the GPU (setNewObserved): bdf_foldin_cells and
bdf_newrows_update_cells through the C ABI against the numpy restatement (tests/foldin_restatement.py) and against the cold path's
kernels -- rows long enough for all four waves and a third trip, a V that is not 16-byte aligned -- whole macau() runs against the restatement driven by the per-iteration device state on both iteration paths, the runs that
must not change, and the quality of the predictions against the CPU chains of the restatement's own sampler.

The tolerances are section 24's: 1e-12 relative for one draw's m, q, uhat and state, 1e-9 for a whole run.  Every P_i here has
cond(P_i) <= 2e3 (asserted), so that D eps cond stays three orders below the run's tolerance."""
import ctypes as C
import math
import os
import textwrap

import numpy as np
import pytest

from both_paths import child
import foldin_restatement as FR
import newrows_restatement as NR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUP = 256                        # cells a workgroup of either update takes
FINAL = 256                        # partial sums the scalars' final reduction takes in one pass (one per thread)
BATCH = 64                         # test cells of a row that k_foldin_cells takes at a time, one lane each


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _spd(rng, D):
    A = rng.standard_normal((D, D))
    L = A @ A.T / D + np.eye(D)
    return 0.5 * (L + L.T)


def _known_relation(B, ctx, kid, ky, n_new, M):
    from bdf_amd.engine import DeviceRelation
    return DeviceRelation(ctx, B.IndexedDF((np.asarray(kid, dtype=np.int64).reshape(-1, 2), np.asarray(ky, dtype=np.float64)), dims=[n_new, M]))


def _foldin(B, ctx, D, n_new, rel, Vt, mu_t, is_matrix, Lt, pairs, mean, alpha, alpha_dev=None):
    """bdf_foldin_cells -> (m, q) in the CALLER's order and uhat, as host arrays; 8 guard doubles behind each stay untouched"""
    from bdf_amd._lib import Term, check, lib
    t = Term()
    t.rel, t.mode, t.alpha, t.mean_value = rel.handle, 0, alpha, mean
    t.factors[1] = Vt.data_ptr()
    t.alpha_dev = alpha_dev.data_ptr() if alpha_dev is not None else None
    n = pairs.n
    m, q, uh = ctx.tensor(np.full(n + 8, -7.0)), ctx.tensor(np.full(n + 8, -7.0)), ctx.tensor(np.full(n_new * D + 8, -7.0))
    check(lib().bdf_foldin_cells(ctx.handle, D, n_new, C.byref(t), _p(mu_t), int(is_matrix), _p(Lt), pairs.handle, mean, _p(m), _p(q), _p(uh)))
    ctx.sync()
    m, q, uh = m.cpu().numpy(), q.cpu().numpy(), uh.cpu().numpy()
    assert np.array_equal(m[n:], np.full(8, -7.0)) and np.array_equal(q[n:], np.full(8, -7.0)) and np.array_equal(uh[n_new * D:], np.full(8, -7.0))
    return _caller_order(pairs, m[:n]), _caller_order(pairs, q[:n]), uh[:n_new * D].reshape(n_new, D)


def _caller_order(pairs, x):
    if pairs._order is None:
        return x
    out = np.empty_like(x)
    out[pairs._order] = x
    return out


def _storage_order(pairs, x):
    return x if pairs._order is None else x[pairs._order]


def _dispatch(ctx):
    """{rows by K1-lr, K1s, K1c, K1, K1's work items, K1c's waves} of the system dumps' launches (entity tag 0) in this iteration"""
    d = ctx.rows_dispatch(0)                                         # None before the first such launch
    return np.array([d[k] for k in ("lowrank", "small", "col", "k1", "k1_items", "col_waves")] if d else [0] * 6, dtype=np.int64)


def _check_cells(D, P, b, ids, V, mean, m, q, uh):
    """one draw against the restatement: 1e-12 relative -- m to the size of what its sum adds, q to itself, uhat to its row's largest
    entry; q > 0"""
    ruh, rm, rq = FR.solve(P, b, ids, V, mean)
    assert max(np.linalg.cond(Pi) for Pi in P) <= 2e3
    e_u = (np.abs(uh - ruh) / np.abs(ruh).max(axis=1, keepdims=True)).max()
    i, j = ids[:, 0] - 1, ids[:, 1] - 1
    scale = np.abs(ruh[i] * V[j]).sum(axis=1) + abs(mean)
    e_m = (np.abs(m - rm) / scale).max() if len(ids) else 0.0
    e_q = (np.abs(q - rq) / rq).max() if len(ids) else 0.0
    assert np.all(q > 0.0)
    return e_u, e_m, e_q


# ---- (a) bdf_foldin_cells ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 3, 16, 17, 32, 33, 64])
def test_cells_match_the_restatement(B, ctx, D):
    """Eight new rows in one call.  Test cells per row: 0, 1, 63, 64, 65, 129 (none; one lane; one short of, exactly, one more than a
    batch of 64 lanes; two batches and a lane), 5 with duplicate columns, 3.  Known cells per row: 1, 0, D + 3, 0, 1, item + 8 (more
    than one work item of the wave-per-row kernel takes -- item: the context's item_size, read through bdf_ctx_item_size; the
    dispatch report must show more items than rows), D + 3, 0.  Once with the shared prior mean and once with a mean per row
    (mu_is_matrix), alpha by value and through alpha_dev.  A second call gives the same bits; uhat is written for the row without a test cell; a cold row (no known cell) has
    P = Lambda and equals newrows_restatement's quad."""
    rng = np.random.default_rng(4100 + D)
    item = ctx.item_size()                                         # (192 as bdf_ctx_create sets it)
    assert 8 <= item <= 4096, item                                 # (a test that set larger items on the shared context did not restore it)
    n_new, M, mean, alpha = 8, item + 20, 0.3, 2.0
    n_test = [0, 1, BATCH - 1, BATCH, BATCH + 1, 2 * BATCH + 1, 5, 3]
    n_known = [1, 0, D + 3, 0, 1, item + 8, D + 3, 0]
    ids = np.concatenate([np.stack([np.full(c, i + 1), rng.integers(1, M + 1, c)], axis=1) for i, c in enumerate(n_test) if c]).astype(np.int64)
    ids[ids[:, 0] == 7, 1] = [4, 9, 4, 4, 9]                       # duplicate columns among a row's test cells
    ids = ids[rng.permutation(len(ids))]                           # the caller's order is not the storage order
    kid = np.concatenate([np.stack([np.full(c, i + 1), rng.permutation(M)[:c] + 1], axis=1) for i, c in enumerate(n_known) if c]).astype(np.int64)
    kid = kid[rng.permutation(len(kid))]
    ky = rng.standard_normal(len(kid))
    Lam, V = _spd(rng, D), 0.5 * rng.standard_normal((M, D))
    mu, mu_rows = 0.4 * rng.standard_normal(D), 0.4 * rng.standard_normal((n_new, D))
    rel = _known_relation(B, ctx, kid, ky, n_new, M)
    pairs = B.DevicePairs(ctx, ids, np.zeros(len(ids)))
    pairs.sort(0)
    Lt, Vt = ctx.tensor(Lam), ctx.tensor(V)
    worst = np.zeros(3)
    for is_matrix, prior, a_val, a_dev in ((False, mu, alpha, None), (True, mu_rows, 123.0, ctx.tensor([alpha]))):
        before = _dispatch(ctx)
        m, q, uh = _foldin(B, ctx, D, n_new, rel, Vt, ctx.tensor(prior), is_matrix, Lt, pairs, mean, a_val, a_dev)
        d = _dispatch(ctx) - before
        assert d[:3].sum() == 0 and d[3] == n_new and d[4] > n_new, d        # every system by the wave-per-row kernel, the long row in pieces
        P, b = FR.systems(Lam, prior if is_matrix else np.tile(mu, (n_new, 1)), V, alpha, kid, ky, mean)
        worst = np.maximum(worst, _check_cells(D, P, b, ids, V, mean, m, q, uh))
        m2, q2, uh2 = _foldin(B, ctx, D, n_new, rel, Vt, ctx.tensor(prior), is_matrix, Lt, pairs, mean, a_val, a_dev)
        assert np.array_equal(m, m2) and np.array_equal(q, q2) and np.array_equal(uh, uh2)
        cold = np.isin(ids[:, 0], [2, 4, 8])
        qc = NR.quad(Lam, V)[ids[cold, 1] - 1]
        assert (np.abs(q[cold] - qc) / qc).max() <= 1e-12
    print(f"foldin cells D={D}: worst relative error of uhat {worst[0]:.2e}, m {worst[1]:.2e}, q {worst[2]:.2e} (asserted: 1e-12)")
    assert worst.max() <= 1e-12, worst
    pairs.close()
    rel.close()


LONG_ROWS = [3 * BATCH - 1, 3 * BATCH, 3 * BATCH + 1, 4 * BATCH - 1, 4 * BATCH, 4 * BATCH + 1, 5 * BATCH, 5 * BATCH + 1, 0, 8 * BATCH + 1]


def _long_rows_reach_every_wave_twice_and_a_third_trip():
    """batch t of a row goes to wave t % 4 on its trip t // 4 (k_foldin_cells: k0 = k_begin + 64 wave, k0 += 256)"""
    assert LONG_ROWS == [191, 192, 193, 255, 256, 257, 320, 321, 0, 513]
    reached = {(t % 4, t // 4) for c in LONG_ROWS for t in range(-(-c // BATCH))}
    assert reached >= {(w, trip) for w in range(4) for trip in (0, 1)} and (0, 2) in reached, sorted(reached)


@pytest.mark.parametrize("D", [3, 16, 33, 64])
def test_cells_of_long_rows_match_the_restatement(B, ctx, D):
    """Ten new rows in one call.  Test cells per row: 191, 192, 193, 255, 256, 257, 320, 321, 0, 513 (one short of three full batches;
    wave 3 idle; wave 3 with a single lane; wave 3 one lane short of full; every wave exactly one full batch; wave 0's second trip
    with one lane; wave 0's second trip full; wave 1's second trip with one lane; an empty row between long ones; wave 0's third
    trip).  Known cells per row: 3, 1, 4, 0 (cold), 2, 5, 3, 2, 1, 4.  M = 40, so that a row's columns repeat many times: for a fixed
    (row, column) m and q are the same bits at every place at which the column occurs in the row -- which wave takes a cell does not
    change what is computed for it (asserted to hold over places of different batches).  D = 3: the scalar gather; 16, 33, 64: the
    three DP.  The shared prior mean and a mean per row; a second call gives the same bits."""
    _long_rows_reach_every_wave_twice_and_a_third_trip()
    rng = np.random.default_rng(4300 + D)
    n_new, M, mean, alpha = len(LONG_ROWS), 40, 0.3, 2.0
    n_known = [3, 1, 4, 0, 2, 5, 3, 2, 1, 4]
    ids = np.concatenate([np.stack([np.full(c, i + 1), rng.integers(1, M + 1, c)], axis=1) for i, c in enumerate(LONG_ROWS) if c]).astype(np.int64)
    ids = ids[rng.permutation(len(ids))]                           # the caller's order is not the storage order
    kid = np.concatenate([np.stack([np.full(c, i + 1), rng.permutation(M)[:c] + 1], axis=1) for i, c in enumerate(n_known) if c]).astype(np.int64)
    kid = kid[rng.permutation(len(kid))]
    ky = rng.standard_normal(len(kid))
    Lam, V = _spd(rng, D), 0.5 * rng.standard_normal((M, D))
    mu, mu_rows = 0.4 * rng.standard_normal(D), 0.4 * rng.standard_normal((n_new, D))
    rel = _known_relation(B, ctx, kid, ky, n_new, M)
    pairs = B.DevicePairs(ctx, ids, np.zeros(len(ids)))
    pairs.sort(0)
    # the places of every (row, column): the first of each, and that some column of every long row recurs in another batch
    stored = _storage_order(pairs, ids)
    assert np.all(np.diff(stored[:, 0]) >= 0)
    place = np.arange(len(stored)) - np.searchsorted(stored[:, 0], stored[:, 0])
    _, first, inv = np.unique(stored, axis=0, return_index=True, return_inverse=True)
    inv = inv.ravel()
    moved = (place // BATCH) != (place[first[inv]] // BATCH)
    assert set(stored[moved, 0]) == {i + 1 for i, c in enumerate(LONG_ROWS) if c}
    Lt, Vt = ctx.tensor(Lam), ctx.tensor(V)
    worst = np.zeros(3)
    for is_matrix, prior in ((False, mu), (True, mu_rows)):
        m, q, uh = _foldin(B, ctx, D, n_new, rel, Vt, ctx.tensor(prior), is_matrix, Lt, pairs, mean, alpha)
        P, b = FR.systems(Lam, prior if is_matrix else np.tile(mu, (n_new, 1)), V, alpha, kid, ky, mean)
        worst = np.maximum(worst, _check_cells(D, P, b, ids, V, mean, m, q, uh))
        ms, qs = _storage_order(pairs, m), _storage_order(pairs, q)
        same = (ms == ms[first[inv]]) & (qs == qs[first[inv]])
        assert same.all(), ("a cell differs from the first cell of its (row, column)", stored[~same][:4], place[~same][:4])
        m2, q2, uh2 = _foldin(B, ctx, D, n_new, rel, Vt, ctx.tensor(prior), is_matrix, Lt, pairs, mean, alpha)
        assert np.array_equal(m, m2) and np.array_equal(q, q2) and np.array_equal(uh, uh2)
    print(f"foldin cells of long rows D={D}: worst relative error of uhat {worst[0]:.2e}, m {worst[1]:.2e}, q {worst[2]:.2e} (asserted: 1e-12)")
    assert worst.max() <= 1e-12, worst
    pairs.close()
    rel.close()


def _offset_view(ctx, a):
    """`a` on the device as a view that starts one double into a larger tensor -- its address is 8 mod 16 -- with NaN in the doubles
    before and behind it"""
    flat = np.concatenate([[np.nan], np.asarray(a, dtype=np.float64).ravel(), np.full(3, np.nan)])
    v = ctx.tensor(flat)[1:1 + a.size].view(*a.shape)
    assert v.data_ptr() % 16 == 8 and v.is_contiguous()
    return v


def _solve(ctx, D, n_new, Pt, bt, pairs, M, Vt, mean):
    """bdf_foldin_solve -> (m, q) in the caller's order and uhat; 8 guard doubles behind each stay untouched"""
    from bdf_amd._lib import check, lib
    n = pairs.n
    m, q, uh = ctx.tensor(np.full(n + 8, -7.0)), ctx.tensor(np.full(n + 8, -7.0)), ctx.tensor(np.full(n_new * D + 8, -7.0))
    check(lib().bdf_foldin_solve(ctx.handle, D, n_new, _p(Pt), _p(bt), pairs.handle, M, _p(Vt), mean, _p(m), _p(q), _p(uh)))
    ctx.sync()
    m, q, uh = m.cpu().numpy(), q.cpu().numpy(), uh.cpu().numpy()
    assert np.array_equal(m[n:], np.full(8, -7.0)) and np.array_equal(q[n:], np.full(8, -7.0)) and np.array_equal(uh[n_new * D:], np.full(8, -7.0))
    return _caller_order(pairs, m[:n]), _caller_order(pairs, q[:n]), uh[:n_new * D].reshape(n_new, D)


@pytest.mark.parametrize("D", [16, 32, 64])
def test_a_v_that_is_not_16_byte_aligned_takes_the_scalar_gather(B, ctx, D):
    """an even D gathers a row of V by 16-byte loads only when V is 16-byte aligned (FoldinArgs::wide).  The same values from an aligned
    tensor and from a view that starts one double into a larger one give m, q and uhat bit for bit -- both gathers load the same
    doubles into the same registers -- through bdf_foldin_cells and through bdf_foldin_solve, and both match the restatement.  NaN
    stands before and behind the view: a 16-byte load that started a double early or ran one late would show.  Three rows of 65, 3
    and 0 test cells, among them the first and the last row of V"""
    rng = np.random.default_rng(4400 + D)
    n_new, M, mean, alpha = 3, 20, 0.3, 2.0
    n_test, n_known = [BATCH + 1, 3, 0], [3, 0, D + 3 if D + 3 <= M else M]
    ids = np.concatenate([np.stack([np.full(c, i + 1), rng.integers(1, M + 1, c)], axis=1) for i, c in enumerate(n_test) if c]).astype(np.int64)
    ids[:2, 1], ids[-3:, 1] = [1, M], [M, 1, 7]
    ids = ids[rng.permutation(len(ids))]
    kid = np.concatenate([np.stack([np.full(c, i + 1), rng.permutation(M)[:c] + 1], axis=1) for i, c in enumerate(n_known) if c]).astype(np.int64)
    ky = rng.standard_normal(len(kid))
    Lam, V, mu = _spd(rng, D), 0.5 * rng.standard_normal((M, D)), 0.4 * rng.standard_normal(D)
    rel = _known_relation(B, ctx, kid, ky, n_new, M)
    pairs = B.DevicePairs(ctx, ids, np.zeros(len(ids)))
    pairs.sort(0)
    Lt, mt = ctx.tensor(Lam), ctx.tensor(mu)
    V_al, V_off = ctx.tensor(V), _offset_view(ctx, V)
    assert V_al.data_ptr() % 16 == 0
    P, b = FR.systems(Lam, np.tile(mu, (n_new, 1)), V, alpha, kid, ky, mean)
    Pt, bt = ctx.tensor(P), ctx.tensor(b)
    for name, run in (("bdf_foldin_cells", lambda Vt: _foldin(B, ctx, D, n_new, rel, Vt, mt, False, Lt, pairs, mean, alpha)),
                      ("bdf_foldin_solve", lambda Vt: _solve(ctx, D, n_new, Pt, bt, pairs, M, Vt, mean))):
        wide, narrow = run(V_al), run(V_off)
        for x, y, what in zip(wide, narrow, ("m", "q", "uhat")):
            assert np.all(np.isfinite(y)) and np.array_equal(x, y), (name, what)
        assert max(_check_cells(D, P, b, ids, V, mean, *narrow)) <= 1e-12, name
        assert max(_check_cells(D, P, b, ids, V, mean, *wide)) <= 1e-12, name
    pairs.close()
    rel.close()


def test_one_new_row_and_what_the_entry_refuses(B, ctx):
    """n* = 1 with three known and two test cells; then the C ABI's refusals: NULL arguments, D outside 1..64, cells that are not
    sorted by the new row, ids outside the dims (BDF_ERR_BOUNDS), a relation of another size"""
    from bdf_amd._lib import Term, check, lib
    rng = np.random.default_rng(8)
    D, M, mean, alpha = 5, 9, -0.2, 3.0
    kid, ky = np.array([[1, 2], [1, 7], [1, 9]]), rng.standard_normal(3)
    ids = np.array([[1, 7], [1, 1]])
    Lam, V, mu = _spd(rng, D), 0.5 * rng.standard_normal((M, D)), 0.3 * rng.standard_normal(D)
    rel = _known_relation(B, ctx, kid, ky, 1, M)
    pairs = B.DevicePairs(ctx, ids, np.zeros(2))
    pairs.sort(0)
    Lt, Vt, mt = ctx.tensor(Lam), ctx.tensor(V), ctx.tensor(mu)
    m, q, uh = _foldin(B, ctx, D, 1, rel, Vt, mt, False, Lt, pairs, mean, alpha)
    P, b = FR.systems(Lam, mu[None, :], V, alpha, kid, ky, mean)
    assert max(_check_cells(D, P, b, ids, V, mean, m, q, uh)) <= 1e-12
    t = Term()
    t.rel, t.mode, t.alpha, t.mean_value = rel.handle, 0, alpha, mean
    t.factors[1] = Vt.data_ptr()
    out = ctx.zeros(16)

    def call(c=ctx.handle, D=D, n=1, term=t, mu=_p(mt), L=_p(Lt), p=pairs.handle, m=_p(out), q=_p(out), u=_p(out)):
        check(lib().bdf_foldin_cells(c, D, n, C.byref(term) if term is not None else None, mu, 0, L, p, mean, m, q, u))

    for bad in (dict(c=None), dict(term=None), dict(mu=None), dict(L=None), dict(p=None), dict(m=None), dict(q=None), dict(u=None), dict(D=0), dict(D=65),
                dict(n=0), dict(n=2)):
        with pytest.raises(B.ArgumentError, match="bdf_foldin_cells"):
            call(**bad)
    unsorted = B.DevicePairs(ctx, ids, np.zeros(2))
    with pytest.raises(B.ArgumentError, match="sorted by the new row"):
        call(p=unsorted.handle)
    unsorted.close()
    outside = B.DevicePairs(ctx, np.array([[1, M + 1]]), np.zeros(1))
    outside.sort(0)
    with pytest.raises(Exception, match="outside"):
        call(p=outside.handle)
    outside.close()
    call()
    ctx.sync()
    pairs.close()
    rel.close()


# ---- (b) chunking -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,is_matrix", [(4, True), (17, False), (33, True)])
def test_chunks_give_identical_bits(B, ctx, D, is_matrix):
    """the new rows in chunks of 1, of 2 and all at once (bdf_ctx_set_nonneg_chunk: the chunk of bdf_sample_rows_nonneg's scratch cap):
    m, q and uhat bit for bit.  Seven rows of 0 .. D + 3 known cells, so that the degree order that the chunks follow is not the rows'
    order, and five test cells each"""
    from bdf_amd._lib import check, lib
    rng = np.random.default_rng(600 + D)
    n_new, M, mean, alpha = 7, 40, 0.1, 1.5
    counts = [3, 0, D + 3, 1, 0, 7, 2]
    kid = np.concatenate([np.stack([np.full(c, i + 1), rng.permutation(M)[:c] + 1], axis=1) for i, c in enumerate(counts) if c]).astype(np.int64)
    ky = rng.standard_normal(len(kid))
    ids = np.stack([np.repeat(np.arange(1, n_new + 1), 5), rng.integers(1, M + 1, 5 * n_new)], axis=1)
    Lam, V = _spd(rng, D), 0.5 * rng.standard_normal((M, D))
    prior = 0.4 * rng.standard_normal((n_new, D) if is_matrix else D)
    rel = _known_relation(B, ctx, kid, ky, n_new, M)
    pairs = B.DevicePairs(ctx, ids, np.zeros(len(ids)))
    pairs.sort(0)
    Lt, Vt, pt = ctx.tensor(Lam), ctx.tensor(V), ctx.tensor(prior)
    got = {}
    try:
        for chunk in (1, 2, 0):
            check(lib().bdf_ctx_set_nonneg_chunk(ctx.handle, chunk))
            got[chunk] = _foldin(B, ctx, D, n_new, rel, Vt, pt, is_matrix, Lt, pairs, mean, alpha)
    finally:
        check(lib().bdf_ctx_set_nonneg_chunk(ctx.handle, 0))
    for chunk in (1, 2):
        for a, b in zip(got[chunk], got[0]):
            assert np.array_equal(a, b), chunk
    P, b = FR.systems(Lam, prior if is_matrix else np.tile(prior, (n_new, 1)), V, alpha, kid, ky, mean)
    assert max(_check_cells(D, P, b, ids, V, mean, *got[0])) <= 1e-12
    pairs.close()
    rel.close()


# ---- (c) the fold's sibling -------------------------------------------------------------------------------------------------------
def _state(pairs):
    """the running state in STORAGE order: (5, n) -- mean, M2, sum q, M, A -- and the draws it holds"""
    from bdf_amd._lib import check, lib
    st, draws = C.c_void_p(), C.c_double()
    check(lib().bdf_newrows_state(pairs.handle, C.byref(st), C.byref(draws)))
    raw = np.zeros((5, pairs.n))
    if st.value and pairs.n:
        check(lib().bdf_d2h(pairs.ctx.handle, raw.ctypes.data_as(C.c_void_p), st, raw.size * 8))
    return raw, draws.value


@pytest.mark.parametrize("n,probit,sort,score", [(GROUP + 1, False, True, 1), (GROUP + 1, True, False, 1), (GROUP + 1, False, False, 0),
                                                 (GROUP * (FINAL + 1) + 3, False, True, 1)])
def test_the_fold_sibling_equals_the_cold_update(B, ctx, n, probit, sort, score):
    """bdf_newrows_update_cells fed the (m, q) that the cold path implies -- m = mean + uhat . v_j, q = q_j of bdf_newrows_quad -- against
    bdf_newrows_update on the same cells, through the phases 0, 0, 1, 2, 0, 2 with fresh factors at every step, about a fifth of the
    values NaN, lpd on and off, identity and probit link, pairs sorted and not; n: one more than a workgroup takes, and 256 x 257 + 3
    cells, whose 258 partial sums are more than the final reduction's 256 threads take in one pass.

    EQUAL TO THE BIT, the state's five planes and the eight scalars: the two kernels run one text (csrc/newrows.h: bdf_newrows_step) on
    the same lanes, so only m could differ -- and the factors here are multiples of 1/8 of small size, so that every product and every
    partial sum of uhat . v_j is exact in any order and numpy's m IS the kernel's."""
    from bdf_amd._lib import check, lib
    rng = np.random.default_rng(7000 + n % 1000 + 2 * probit + sort)
    D, n_new, M, mean, alpha = 8, 13, 29, (0.0 if probit else 0.25), 2.5
    ids = np.stack([rng.integers(1, n_new + 1, n), rng.integers(1, M + 1, n)], axis=1)
    y = (rng.random(n) < 0.5).astype(np.float64) if probit else rng.standard_normal(n)
    y[rng.random(n) < 0.2] = np.nan
    cold, fold = B.DevicePairs(ctx, ids, y), B.DevicePairs(ctx, ids, y)
    if sort:
        cold.sort(1)
        fold.sort(1)
    if probit:
        cold.set_link(1)
        fold.set_link(1)
    cut, lo, hi = (0.5 if probit else 0.1), -0.4, 0.8
    s_cold, s_fold, qt = ctx.zeros(8), ctx.zeros(8), ctx.zeros(M)
    for phase in (0, 0, 1, 2, 0, 2):
        uh, V, Lam = rng.integers(-16, 17, (n_new, D)) / 8.0, rng.integers(-16, 17, (M, D)) / 8.0, _spd(rng, D)
        ut, vt = ctx.tensor(uh), ctx.tensor(V)
        check(lib().bdf_newrows_quad(ctx.handle, D, M, _p(ctx.tensor(Lam)), _p(vt), _p(qt)))
        ctx.sync()
        q = qt.cpu().numpy()
        m = mean + np.sum(uh[ids[:, 0] - 1] * V[ids[:, 1] - 1], axis=1)
        mt, qc = ctx.tensor(_storage_order(fold, m)), ctx.tensor(_storage_order(fold, q[ids[:, 1] - 1]))
        check(lib().bdf_newrows_update(ctx.handle, cold.handle, D, _p(ut), _p(vt), _p(qt), mean, alpha, None, phase, lo, hi, cut, score, _p(s_cold)))
        check(lib().bdf_newrows_update_cells(ctx.handle, fold.handle, _p(mt), _p(qc), alpha, None, phase, lo, hi, cut, score, _p(s_fold)))
        ctx.sync()
        a, b = s_cold.cpu().numpy(), s_fold.cpu().numpy()
        assert np.array_equal(a, b) and np.all(np.isfinite(a)) and a[4] == np.sum(~np.isnan(y)), (phase, a, b)
        (sa, da), (sb, db) = _state(cold), _state(fold)
        assert da == db and np.array_equal(sa, sb), phase
    out_a, out_b = ctx.zeros((n, 3)), ctx.zeros((n, 3))
    check(lib().bdf_newrows_result(ctx.handle, cold.handle, _p(out_a)))
    check(lib().bdf_newrows_result(ctx.handle, fold.handle, _p(out_b)))
    ctx.sync()
    assert np.array_equal(out_a.cpu().numpy(), out_b.cpu().numpy(), equal_nan=True)
    assert np.isnan(out_b.cpu().numpy()[:, 2]).all() == (score == 0 or bool(np.isnan(y).all()))
    cold.close()
    fold.close()


def test_what_the_fold_sibling_refuses(B, ctx):
    """a phase outside 0..2, phase 2 before a phase 1, a score_lpd that changed, NULL planes, a bad alpha, three modes; no cells: zeros"""
    from bdf_amd._lib import check, lib
    rng = np.random.default_rng(5)
    n = 40
    ids = np.stack([rng.integers(1, 6, n), rng.integers(1, 9, n)], axis=1)
    pairs = B.DevicePairs(ctx, ids, rng.standard_normal(n))
    mt, qt, stats = ctx.tensor(rng.standard_normal(n)), ctx.tensor(rng.random(n) + 0.1), ctx.tensor(np.full(8, 7.0))

    def update(c=ctx.handle, p=pairs.handle, m=_p(mt), q=_p(qt), a=2.0, phase=1, score=0, st=_p(stats)):
        check(lib().bdf_newrows_update_cells(c, p, m, q, a, None, phase, 1.0, -1.0, 0.0, score, st))

    for bad in (dict(c=None), dict(p=None), dict(st=None), dict(m=None), dict(q=None), dict(phase=-1), dict(phase=3), dict(a=0.0), dict(a=float("nan")),
                dict(phase=2)):
        with pytest.raises(B.ArgumentError, match="bdf_newrows_update_cells"):
            update(**bad)
    update(phase=1, score=0)
    with pytest.raises(B.ArgumentError, match="score_lpd"):
        update(phase=2, score=1)
    update(phase=2, score=0)
    ctx.sync()
    s = stats.cpu().numpy()
    assert s[4] == n and s[5] == 0.0 and s[6] == 0.0 and s[0] > 0.0
    three = B.DevicePairs(ctx, np.ones((4, 3), dtype=np.int64), np.zeros(4))
    with pytest.raises(B.ArgumentError, match="two-mode"):
        update(p=three.handle)
    three.close()
    pairs.close()
    empty = B.DevicePairs(ctx, np.zeros((0, 2), dtype=np.int64), np.zeros(0))
    stats.fill_(7.0)
    update(p=empty.handle)
    ctx.sync()
    assert np.array_equal(stats.cpu().numpy(), np.zeros(8))
    empty.close()


# ---- (d) a system that is not positive definite --------------------------------------------------------------------------------
def test_an_indefinite_system_raises_notpd_and_leaves_nan(B):
    """bdf_foldin_solve, the parity entry, on two systems of which the second is a Lambda with a negative eigenvalue: the call returns,
    the context's NOTPD flag comes at the next sync (once), the bad row's uhat, m and q are NaN, the good row's are right; and a clean
    call afterwards"""
    from bdf_amd._lib import check, lib
    ctx = B.Context(seed=5)
    rng = np.random.default_rng(3)
    D, M, mean = 12, 20, 0.2
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    ev = np.linspace(0.5, 3.0, D)
    ev[4] = -0.7
    bad = (Q * ev) @ Q.T
    P = np.stack([_spd(rng, D), 0.5 * (bad + bad.T)])
    b, V = rng.standard_normal((2, D)), 0.5 * rng.standard_normal((M, D))
    ids = np.stack([np.repeat([1, 2], 5), rng.integers(1, M + 1, 10)], axis=1)
    pairs = B.DevicePairs(ctx, ids, np.zeros(10))
    pairs.sort(0)
    Vt = ctx.tensor(V)
    m, q, uh = ctx.zeros(10), ctx.zeros(10), ctx.zeros(2, D)

    bt, keep = ctx.tensor(b), []

    def solve(Pm):
        keep.append(ctx.tensor(Pm))                                  # (alive until the launch has run)
        check(lib().bdf_foldin_solve(ctx.handle, D, 2, _p(keep[-1]), _p(bt), pairs.handle, M, _p(Vt), mean, _p(m), _p(q), _p(uh)))

    solve(P)
    with pytest.raises(B.NotPositiveDefinite):
        ctx.sync()
    ctx.sync()
    gm, gq, gu = _caller_order(pairs, m.cpu().numpy()), _caller_order(pairs, q.cpu().numpy()), uh.cpu().numpy()
    second = ids[:, 0] == 2
    assert np.isnan(gm[second]).all() and np.isnan(gq[second]).all() and np.isnan(gu[1]).all()
    ru, rm, rq = FR.solve(P[:1], b[:1], ids[~second], V, mean)
    assert np.allclose(gu[0], ru[0], rtol=1e-10) and np.allclose(gm[~second], rm, rtol=1e-10) and np.allclose(gq[~second], rq, rtol=1e-10)
    good = np.stack([P[0], _spd(rng, D)])
    solve(good)
    ctx.sync()
    ru, rm, rq = FR.solve(good, b, ids, V, mean)
    assert np.allclose(_caller_order(pairs, q.cpu().numpy()), rq, rtol=1e-10) and np.allclose(uh.cpu().numpy(), ru, rtol=1e-10)
    pairs.close()
    ctx.close()


# ---- (e) macau() end to end -------------------------------------------------------------------------------------------------------
SHAPE = dict(n_train=40, n_new=6, M=12, numF=3, density=0.5, noise=0.3)
BURNIN, PSAMPLES, SEED, KNOWN = 4, 5, 23, 3
CASES = {                          # features, alpha sampled, the entity with new rows in the relation's second column
    "feat_fixed": (True, False, False),
    "feat_sampled": (True, True, False),
    "plain_fixed": (False, False, False),
    "second_mode": (True, False, True),
}
DIMS = (4, 17)


def _case(name):
    feat, sampled, second = CASES[name]
    Ft, Fn, (ids, y), new = NR.planted(seed=900 + sorted(CASES).index(name), D=4, **SHAPE)
    (kid, ky), (tid, ty) = FR.split_known(new, KNOWN, 5)
    keep = kid[:, 0] != 2                                  # the second new row has no known cell: cold
    kid, ky = kid[keep], ky[keep]
    ty = ty.copy()
    ty[2::7] = np.nan                                      # a few cells whose value is unknown
    tid, ty = np.concatenate([tid, kid[:2]]), np.concatenate([ty, ky[:2]])       # two test cells that are also known cells
    return dict(feat=feat, sampled=sampled, second=second, Ft=Ft, Fn=Fn, ids=ids, y=y, kid=kid, ky=ky, tid=tid, ty=ty)


def _build(B, c, observed=True):
    u, v = B.Entity("u", F=c["Ft"]) if c["feat"] else B.Entity("u"), B.Entity("v")
    cols = (lambda t, val: {"v": t[:, 1], "u": t[:, 0], "y": val}) if c["second"] else (lambda t, val: {"u": t[:, 0], "v": t[:, 1], "y": val})
    ents, dims = ([v, u], [SHAPE["M"], SHAPE["n_train"]]) if c["second"] else ([u, v], [SHAPE["n_train"], SHAPE["M"]])
    rel = B.Relation(cols(c["ids"], c["y"]), "planted", ents, alpha=1.0 / 0.09, dims=dims)
    rel.model.alpha_sample = c["sampled"]
    B.assignToTest(rel, np.arange(1, 21))
    if c["feat"]:
        B.setNewRows(u, c["Fn"])
    if observed:
        B.setNewObserved(rel, u, cols(c["kid"], c["ky"]), n_rows=None if c["feat"] else SHAPE["n_new"])
    B.setNewTest(rel, u, cols(c["tid"], c["ty"]))
    return rel, u, v


CHILD = textwrap.dedent('''
    import contextlib, io, sys
    import numpy as np
    sys.path.insert(0, %r); sys.path.insert(0, %r)
    import bdf_amd as B
    from test_gpu_foldin import BURNIN, CASES, DIMS, PSAMPLES, SEED, SHAPE, _build, _case
    out, d = sys.argv[1], {}
    for name in sorted(CASES):
        for D in DIMS:
            c = _case(name)
            rel, u, v = _build(B, c)
            rd = B.RelationData(rel)
            draws = []

            def grab(data):
                a = float(rel._dev.alpha_dev.cpu().item()) if rel.model.alpha_sample else rel.model.alpha
                beta = u.model.beta.copy() if c["feat"] else np.zeros((0, D))
                draws.append((u.model.mu.copy(), u.model.Lambda.copy(), beta, v.model.sample.T.copy(), a))
                return None

            text = io.StringIO()
            with contextlib.redirect_stdout(text):
                res = B.macau(rd, num_latent=D, burnin=BURNIN, psamples=PSAMPLES, verbose=True, seed=SEED, lpd=True, f=grab)
            key = "%%s_%%d_" %% (name, D)
            nr = res["new_rows"]
            assert sorted(nr) == sorted(["RMSE", "ROC", "accuracy", "entity", "factors", "n_rows", "n_scored", "predictions", "LPD", "n_known"]), sorted(nr)
            assert nr["entity"] == "u" and nr["n_rows"] == SHAPE["n_new"]
            d[key + "native"] = np.array(int(rd._engine.native))
            d[key + "table"] = nr["predictions"].to_numpy(dtype=np.float64)
            d[key + "scalars"] = np.array([nr["RMSE"], nr["ROC"], nr["accuracy"], nr["n_scored"], nr["LPD"]], dtype=np.float64)
            d[key + "factors"] = nr["factors"]
            d[key + "n_known"] = nr["n_known"]
            d[key + "mean"] = np.array(rel.model.mean_value)
            d[key + "lines"] = np.array([t for t in text.getvalue().splitlines() if "RMSE=" in t])
            for k, nm in enumerate(("mu", "Lambda", "beta", "V", "alpha")):
                d[key + nm] = np.array([dr[k] for dr in draws])
            d[key + "test"] = np.array([res["RMSE"], res["ROC"]])
            rd._engine.close()
    np.savez(out, **d)
''') % (ROOT, os.path.join(ROOT, "tests"))


@pytest.fixture(scope="module")
def runs():
    """4 + 5 iterations of macau() on every case and D, on the native and on the step-by-step path: one child process per path"""
    return child(CHILD, no_native=False), child(CHILD, no_native=True)


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_macau_folds_in_on_both_paths(runs, name, D):
    """40 x 12 training cells, six new rows with three known cells each (the second with none: cold), features with alpha fixed and
    sampled, no features, the entity with new rows as the relation's second mode; D = 4 and 17.  Both iteration paths equal bit for
    bit.  result["new_rows"] against the restatement driven by the draws read back through f= -- (mu, Lambda, beta, V, alpha) of every
    posterior iteration -- to 1e-9: pred, stdev, lpd, the factors (the posterior mean of uhat_i), the scalars; n_known exactly.  A
    launch that read the next or the previous iteration's V, Lambda, mu_i or alpha would show as a difference of the draws' spread.
    Two of the test cells are also known cells: predicted with their own value in the conditional, as the restatement does."""
    import re
    c = _case(name)
    key = "%s_%d_" % (name, D)
    nat, step = ({k[len(key):]: v for k, v in ch.items() if k.startswith(key)} for ch in runs)
    assert nat["native"] == 1 and step["native"] == 0 and sorted(nat) == sorted(step)
    for k in nat:
        if k not in ("native", "lines"):
            assert np.array_equal(nat[k], step[k], equal_nan=nat[k].dtype.kind == "f"), k
    strip = lambda lines: [re.sub(r"\[[0-9.]+s\]", "", str(t)) for t in lines]
    assert strip(nat["lines"]) == strip(step["lines"]) and len(nat["lines"]) == BURNIN + PSAMPLES
    tid, ty, kid, ky = c["tid"], c["ty"], c["kid"], c["ky"]
    tab = nat["table"]
    cu, cv = (1, 0) if c["second"] else (0, 1)
    assert np.array_equal(tab[:, cu], tid[:, 0]) and np.array_equal(tab[:, cv], tid[:, 1]) and np.array_equal(tab[:, 2], ty, equal_nan=True)
    assert np.array_equal(nat["n_known"], np.bincount(kid[:, 0] - 1, minlength=SHAPE["n_new"])) and nat["n_known"][1] == 0
    assert len(nat["mu"]) == PSAMPLES
    mean, st = float(nat["mean"]), FR.Stream()
    fac = np.zeros_like(nat["factors"])
    for s in range(PSAMPLES):
        mu, Lam, beta, V, alpha = (nat[k][s] for k in ("mu", "Lambda", "beta", "V", "alpha"))
        mu_rows = NR.uhat(mu, beta, c["Fn"]) if c["feat"] else np.tile(mu, (SHAPE["n_new"], 1))
        uh, m, q = FR.cells(Lam, mu_rows, V, float(alpha), kid, ky, tid, mean)
        fac += uh
        p, l = FR.predict(False, m, q), FR.loglik(False, ty, m, q, float(alpha))
        avg, lp = st.update(p, q, l, 1 if s == 0 else 2)
    has = ~np.isnan(ty)
    tol = dict(rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(tab[:, 3], st.mean, **tol)
    np.testing.assert_allclose(tab[:, 4], st.stdev(False), **tol)
    np.testing.assert_allclose(nat["factors"], fac / PSAMPLES, **tol)
    assert np.array_equal(np.isnan(tab[:, 5]), ~has)
    np.testing.assert_allclose(tab[has, 5], lp[has], **tol)
    sc = FR.scalars(ty, avg, p, lp, l, (), 0.0, True)
    rmse, roc, acc, n_scored, LPD = nat["scalars"]
    assert n_scored == has.sum() == sc[4] and acc == sc[2] / sc[4]
    np.testing.assert_allclose(rmse, math.sqrt(sc[0] / sc[4]), **tol)
    np.testing.assert_allclose(LPD, sc[5] / sc[4], **tol)
    for line in nat["lines"]:
        assert re.search(r" new:RMSE=\s*(\d+\.\d{4}|nan) ROC=\s*(\d+\.\d{4}|nan) LPD=-?\d+\.\d{4} \| ", str(line)), line


# ---- (f) the runs that must not change ------------------------------------------------------------------------------------------
def test_an_empty_known_table_equals_the_cold_path(B):
    """section 24's smallest end-to-end case (test_gpu_newrows: 60 x 30 training cells, 20 new rows with features) with setNewTest alone
    and with an empty setNewObserved beside it: every row is cold, but the second run goes through bdf_foldin_cells.  pred, stdev and
    lpd to 1e-12 relative (to max(1, |value|) for lpd), the factors likewise.  Not to the bit: the cold path factorises Lambda once
    and forms q_j by a product with L^-1, the fold-in factorises P_i = Lambda per row and substitutes -- other sums in another order."""
    import test_gpu_newrows as T
    c = T._case("dense_fixed")

    def run(empty):
        rel, u, v = T._build(B, c)
        if empty:
            B.setNewObserved(rel, u, (np.zeros((0, 2), dtype=np.int64), np.zeros(0)))
        rd = B.RelationData(rel)
        res = B.macau(rd, num_latent=T.SHAPE["D"], burnin=3, psamples=4, verbose=False, seed=T.SEED, lpd=True)
        eng_new = rd._engine._new_rows
        kinds = (eng_new.foldin, eng_new.known is not None, eng_new.m is not None)
        rd._engine.close()
        return res, kinds

    (cold, k0), (fold, k1) = run(False), run(True)
    assert k0 == (False, False, False) and k1 == (True, True, True)
    assert "n_known" not in cold["new_rows"] and np.array_equal(fold["new_rows"]["n_known"], np.zeros(len(c["Fn"]), dtype=np.int64))
    a, b = cold["new_rows"]["predictions"], fold["new_rows"]["predictions"]
    worst = 0.0
    for col in ("pred", "stdev", "lpd"):
        x, y = a[col].to_numpy(), b[col].to_numpy()
        assert np.array_equal(np.isnan(x), np.isnan(y))
        ok = ~np.isnan(x)
        e = (np.abs(x[ok] - y[ok]) / np.maximum(np.abs(x[ok]), 1.0 if col == "lpd" else 1e-300)).max()
        worst = max(worst, e)
        assert e <= 1e-12, (col, e)
    fa, fb = cold["new_rows"]["factors"], fold["new_rows"]["factors"]
    assert (np.abs(fa - fb) / np.abs(fa).max(axis=1, keepdims=True)).max() <= 1e-12
    assert cold["RMSE"] == fold["RMSE"]                        # the chain itself is untouched
    print(f"empty known table against the cold path: worst relative difference {worst:.2e} (asserted: 1e-12)")


def test_a_run_without_known_cells_allocates_and_launches_nothing_new(B):
    """setNewTest without setNewObserved: the device object holds no relation of known cells and no (m, q) planes, takes the three cold
    launches -- the library's counter of fold-in launches on the row context stays where it was -- and result["new_rows"] has no
    n_known"""
    import test_gpu_newrows as T
    c = T._case("bin_fixed")
    rel, u, v = T._build(B, c)
    rd = B.RelationData(rel)
    res = B.macau(rd, num_latent=T.SHAPE["D"], burnin=2, psamples=2, verbose=False, seed=T.SEED)
    nr = rd._engine._new_rows
    assert not nr.foldin and nr.known is None and nr.term is None and nr.m is None and nr.qc is None and nr.n_known is None
    assert _dispatch(rd._engine.ctx).sum() == 0                # no system dump (entity tag 0) was ever launched on the row context
    assert sorted(res["new_rows"]) == sorted(["RMSE", "ROC", "accuracy", "entity", "factors", "n_rows", "n_scored", "predictions"])
    rd._engine.close()


# ---- (g) quality ------------------------------------------------------------------------------------------------------------------
def test_fold_in_quality_matches_the_cpu_chains(B):
    """newrows_restatement.QUALITY_SHAPE without features (300 + 100 rows, M = 60, D = 4, alpha = 1 / 0.09 fixed, 50 + 100 iterations), ten
    known cells per new row by foldin_restatement.split_known, the rest scored.  ratio = (fold-in RMSE) / (RMSE of predicting
    mean_value) must be at most the largest of the five CPU chains' ratios x 1.25, and the share of held-out values inside
    pred +- 1.645 sqrt(stdev^2 + 1 / alpha) within the CPU chains' range widened by 0.05 on each side: the chains use different random
    streams and agree in law only.  And the known cells must matter: the ratio is below half of the same run's with no known cell
    (an empty table: every row cold, predicted at the prior mean).  The CPU figures (foldin_restatement.py):
    ratios 0.18300959, 0.18294673, 0.18280405, 0.18267953, 0.18330797; coverage 0.90593343, 0.90448625, 0.90520984, 0.90593343, 0.90520984;
    a cold CPU chain (seed 1) on the same cells: ratio 0.99071144."""
    sh, (ids, y), (kid, ky), (tid, ty) = FR.quality_data()

    def run(known):
        u, v = B.Entity("u"), B.Entity("v")
        rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "planted", [u, v], alpha=NR.QUALITY_ALPHA, dims=[sh["n_train"], sh["M"]])
        B.setNewObserved(rel, u, known, n_rows=sh["n_new"])
        B.setNewTest(rel, u, {"u": tid[:, 0], "v": tid[:, 1], "y": ty})
        rd = B.RelationData(rel)
        res = B.macau(rd, num_latent=sh["D"], burnin=NR.QUALITY_ITERS[0], psamples=NR.QUALITY_ITERS[1], verbose=False, seed=7)
        mean = rel.model.mean_value
        rd._engine.close()
        t = res["new_rows"]["predictions"]
        g = FR.quality(t["pred"].to_numpy(), t["stdev"].to_numpy(), ty, mean, NR.QUALITY_ALPHA)
        assert abs(res["new_rows"]["RMSE"] - g["rmse"]) <= 1e-9
        return g

    g = run({"u": kid[:, 0], "v": kid[:, 1], "y": ky})
    cold = run((np.zeros((0, 2), dtype=np.int64), np.zeros(0)))
    print(f"fold-in: ratio {g['ratio']:.5f} (CPU chains {min(FR.QUALITY_CPU_RATIOS):.5f} ... {max(FR.QUALITY_CPU_RATIOS):.5f}), coverage "
          f"{g['coverage']:.4f} (CPU chains {min(FR.QUALITY_CPU_COVERAGE):.4f} ... {max(FR.QUALITY_CPU_COVERAGE):.4f}); cold ratio {cold['ratio']:.5f}")
    assert g["ratio"] <= 1.25 * max(FR.QUALITY_CPU_RATIOS), g["ratio"]
    assert min(FR.QUALITY_CPU_COVERAGE) - 0.05 <= g["coverage"] <= max(FR.QUALITY_CPU_COVERAGE) + 0.05, g["coverage"]
    assert g["ratio"] < 0.5 * cold["ratio"], (g["ratio"], cold["ratio"])
