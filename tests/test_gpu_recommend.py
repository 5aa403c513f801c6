"""Top-K lists from the posterior mean score (setRecommend) on the device against tests/recommend_restatement.py:
the accumulate kernel at the edges of its tile, bit-identical over the batch size and over a row subset, and past 65,535 tiles; the
lists and the metrics exactly, the lists also over three windows of listed columns; the second trip of the grid-stride loops of
the list, metrics and push kernels; macau() end to end on both iteration paths; and the planted implicit data of section 20 ranked."""
import os
import textwrap

import numpy as np
import pytest

import background_restatement as BR
import recommend_restatement as RR
from both_paths import child

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the tile of k_scores_accum (csrc/recommend.h: BDF_REC_TN x BDF_REC_TM; tests/test_recommend_host.py holds the two equal)
TN, TM = 64, 128
GUARD = 64                                                   # doubles of NaN behind the sum (BDF_REC_GUARD)
# 1e-13 of the sum of |terms| per cell: the restatement adds the same blocks of four d in the same order, the matrix instruction
# associates the four products of a block its own way -- a few ulp of the running sum per block
ACC_TOL = 1e-13

_NS = [1, 15, 16, 17, TN - 1, TN, TN + 1, 2 * TN + 3]
_MS = [1, 15, 16, 17, TM - 1, TM, TM + 1, 2 * TM + 3]
_DS = [3, 16, 17, 32, 33, 64]
# the draws S in {1, B - 1, B, B + 1, 2 B + 1} for B in {1, 3, 8}: every S is run at all three B
_SS = sorted({s for b in (1, 3, 8) for s in (1, b - 1, b, b + 1, 2 * b + 1) if s >= 1})
ACC_CASES = [(_NS[q], _MS[q], _DS[q % 6], _SS[q % len(_SS)]) for q in range(8)] + \
            [(_NS[q], _MS[7 - q], _DS[(q + 3) % 6], _SS[(q + 5) % len(_SS)]) for q in range(8)]


def _guarded(ctx, a):
    """the device copy of the rows of `a` with 16 rows of NaN behind it; the view of the rows themselves"""
    full = np.vstack([a, np.full((16, a.shape[1]), np.nan)])
    return ctx.tensor(full)[:a.shape[0]]


def _accumulate(ctx, draws_dev, n_rows, M, D, batch, rows0=None):
    """push the draws through a ring of `batch` slots; the sum and its guard on the host"""
    from bdf_amd.engine import DeviceScores
    sc = DeviceScores(ctx, n_rows, M, D, batch, rows0)
    for U, V in draws_dev:
        sc.push(U, V)
    out = sc.read(0, n_rows * M + GUARD)
    ctx.sync()
    got = out.cpu().numpy()
    sc.close()
    return got[:n_rows * M].reshape(n_rows, M), got[n_rows * M:]


def test_accumulate_cases_cover_every_size_depth_and_count():
    assert len(_SS) == 8 and {c[3] for c in ACC_CASES} == set(_SS) and {c[2] for c in ACC_CASES} == set(_DS)
    assert {c[0] for c in ACC_CASES} == set(_NS) and {c[1] for c in ACC_CASES} == set(_MS)


@pytest.mark.parametrize("n_rows,M,D,S", ACC_CASES)
def test_accumulate_against_the_restatement_and_bit_identical_over_the_batch(ctx, n_rows, M, D, S):
    rng = np.random.default_rng(n_rows * 1000 + M + D + S)
    draws = [(rng.standard_normal((n_rows, D)), rng.standard_normal((M, D))) for _ in range(S)]
    dev = [(_guarded(ctx, U), _guarded(ctx, V)) for U, V in draws]
    exp, mag = RR.score_sum(draws)
    first = None
    for batch in (1, 3, 8):
        got, guard = _accumulate(ctx, dev, n_rows, M, D, batch)
        assert np.isnan(guard).all()                          # nothing was stored behind the sum
        assert not np.isnan(got).any()                        # no guard row of the factors was read
        if first is None:
            first = got
            worst = float(np.max(np.abs(got - exp) / mag))
            print(f"accumulate n_rows={n_rows} M={M} D={D} S={S}: largest |device - restatement| / sum|terms| = {worst:.2e}")
            assert worst <= ACC_TOL
        else:
            assert np.array_equal(first, got), batch          # the same bits wherever the flushes fall


def test_accumulate_rows_subset_equals_the_same_rows_of_the_full_run(ctx):
    N, M, D, S = 2 * TN + 3, 2 * TM + 3, 17, 4
    rng = np.random.default_rng(11)
    draws = [(rng.standard_normal((N, D)), rng.standard_normal((M, D))) for _ in range(S)]
    dev = [(_guarded(ctx, U), _guarded(ctx, V)) for U, V in draws]
    full, _ = _accumulate(ctx, dev, N, M, D, 3)
    rows0 = rng.permutation(N)[:TN + 6]
    sub, guard = _accumulate(ctx, dev, len(rows0), M, D, 2, rows0)
    assert np.isnan(guard).all() and np.array_equal(sub, full[rows0])


def test_accumulate_past_65535_tiles(ctx):
    """one row of 65,536 tiles and a cell: the tile index is one flattened 64-bit number, no grid dimension caps it"""
    M, D, S = 65536 * TM + 1, 3, 2
    rng = np.random.default_rng(12)
    draws = [(rng.standard_normal((1, D)), rng.standard_normal((M, D))) for _ in range(S)]
    dev = [(_guarded(ctx, U), _guarded(ctx, V)) for U, V in draws]
    got, guard = _accumulate(ctx, dev, 1, M, D, 2)
    exp, mag = RR.score_sum(draws)
    assert np.isnan(guard).all()
    assert np.max(np.abs(got - exp) / mag) <= ACC_TOL
    assert got[0, -1] != 0.0 and got[0, 65535 * TM] != 0.0


# ---- the lists --------------------------------------------------------------------------------------------------------------------
def _topk_case(B, M, seed):
    """8 rows of sums in eighths with many duplicates, and a relation that lists: row 0 every cell, row 1 none, row 2 the first
    column, row 3 the last, row 4 all but three (fewer candidates than K = 5), rows 5 .. 7 about a third"""
    rng = np.random.default_rng(seed)
    sums = rng.integers(-6, 7, (8, M)) / 8.0
    on = rng.random((8, M)) < 0.33
    on[0, :], on[1, :], on[2, :], on[3, :] = True, False, False, False
    on[2, 0], on[3, M - 1] = True, True
    on[4, :] = True
    on[4, rng.permutation(M)[:3]] = False
    i, j = np.nonzero(on)
    p = rng.permutation(len(i))
    ids = np.stack([i[p] + 1, j[p] + 1], axis=1).astype(np.int64)
    rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": np.ones(len(ids))}, "plays", [B.Entity("u"), B.Entity("v")], dims=[8, M])
    return sums, ids, rel


@pytest.mark.parametrize("M", [1, 63, 64, 65, 257, 4097])
@pytest.mark.parametrize("K", [1, 5, 64])
def test_topk_lists_equal_the_restatement_exactly(B, ctx, M, K):
    from bdf_amd.engine import DeviceRelation, DeviceScores
    sums, ids, rel = _topk_case(B, M, 100 + M)
    dr = DeviceRelation(ctx, rel.data)
    draws, mean = 4.0, 0.5                                   # sums in eighths over four draws: every score is exact
    for rows0 in (None, np.array([6, 1, 0, 3, 4, 2])):       # (a subset: the listed columns come from the row's own id)
        n = 8 if rows0 is None else len(rows0)
        mine = sums if rows0 is None else sums[rows0]
        sc = DeviceScores(ctx, n, M, 3, 1, rows0)
        sc.write(ctx.tensor(mine), draws)
        scores = RR.scores_of(mine, draws, mean)
        for exclude in (True, False):
            items, vals = sc.topk(K, mean, dr if exclude else None)
            ctx.sync()
            ei, ev = RR.topk(scores, K, RR.listed_of(ids, n, rows0) if exclude else None)
            gi, gv = items.cpu().numpy(), vals.cpu().numpy()
            assert gi.dtype == np.int32 and np.array_equal(gi, ei), (rows0, exclude)
            assert np.array_equal(gv, ev, equal_nan=True)
            assert np.array_equal(gi == 0, np.isnan(gv))
            if exclude and rows0 is None:
                assert not gi[0].any()                        # every cell listed: padding only
                assert np.count_nonzero(gi[4]) == min(K, 3, M)
                assert np.count_nonzero(gi[1]) == min(K, M)
        sc.close()
    dr.close()


# ---- the lists past one window of listed columns -----------------------------------------------------------------------------------
WINDOW = 65536                                               # columns k_topk_rows marks in LDS at a time (csrc/recommend.h: BDF_REC_WINDOW)
M_WIN = 2 * WINDOW + 3                                       # three windows, the last of 3 columns
SUBSET = np.array([6, 1, 5, 0, 3, 4, 2])


def _plan_b():
    """row b's best entries, best first, as (window or column, sum in eighths): windows 0 and 1 in turn; exact ties between a column
    of window 0 and one of window 1 at the places 1 | 2 and 5 | 6, so that for K = 1 and K = 5 the candidate of the later window ties
    the K-th entry and is refused; a tie between window 1 and window 2 at the places 8 | 9; and place 64 (window 0) tied by a column
    of window 1 and by one of window 2"""
    plan = [("a", 500), ("b", 500), ("a", 499), ("b", 498), ("a", 497), ("b", 497), ("a", 496), ("b", 495), (2 * WINDOW, 495)]
    while len(plan) < 64:
        plan.append(("a" if len(plan) % 2 else "b", 494 - (len(plan) - 9)))
    assert plan[63] == ("a", 440)
    return plan + [("b", 440), (2 * WINDOW + 2, 440), ("a", 439), ("b", 438)]


def _window_case(B):
    """8 rows over M = 2 x 65536 + 3 columns, sums in eighths.  Rows a .. f stand on a floor of sums <= 0 with what matters planted
    above it; a: the 64 best in windows 1 and 2 only; b: _plan_b; c: the best columns all listed, in windows 1 and 2, the window
    edges among them; d: the aliasing pairs (c listed and low, c + 65536 not listed and best; c' not listed, c' + 65536 listed and
    best; the same against window 2); e: every column of windows 0 and 1 listed, and one of window 2; f: nothing listed; g, h: a random
    third listed over uniform sums, as _topk_case.  The references (RR.topk at K = 64: a shorter list is its prefix) are made once."""
    rng = np.random.default_rng(4242)
    M, W = M_WIN, WINDOW
    sums = rng.integers(-6, 1, (8, M)) / 8.0
    on = np.zeros((8, M), dtype=bool)

    def pick(lo, hi, n, avoid=()):
        return rng.permutation(np.setdiff1d(np.arange(lo, hi), np.asarray(sorted(avoid), dtype=np.int64)))[:n]

    # a
    sums[0, pick(W, 2 * W, 70)] = rng.integers(1, 6, 70) / 8.0
    sums[0, 2 * W:] = np.array([7, 3, 6]) / 8.0
    on[0, pick(0, W, 50)] = True
    # b
    cols = {"a": list(pick(0, W, 40)), "b": list(pick(W, 2 * W, 40))}
    planned_b = np.array([cols[w].pop() if isinstance(w, str) else w for w, _ in _plan_b()], dtype=np.int64)
    sums[1, planned_b] = np.array([v for _, v in _plan_b()]) / 8.0
    on[1, pick(0, M, 100, avoid=planned_b)] = True
    # c
    edges = [W - 1, W, W + 1, 2 * W - 1, 2 * W, M - 1]
    listed_c = np.concatenate([edges, pick(W + 2, 2 * W - 1, 70)])
    sums[2, listed_c] = rng.integers(700, 800, len(listed_c)) / 8.0
    sums[2, [W, 2 * W, M - 1]] = 900 / 8.0                   # the row's maximum, three times, all listed
    on[2, listed_c] = True
    free = np.concatenate([pick(0, W - 1, 40), pick(W + 2, 2 * W - 1, 40, avoid=listed_c)])
    sums[2, free] = rng.integers(100, 400, 80) / 8.0
    sums[2, 2 * W + 1] = 450 / 8.0
    # d
    c1, c2 = 1234, 4321
    on[3, [c1, c2 + W, 1, 2 * W + 2]] = True
    sums[3, [c1, c1 + W, c2, c2 + W, 1, 2 * W + 1, 2, 2 * W + 2]] = np.array([-50, 1000, 300, 1001, -40, 999, 250, 1002]) / 8.0
    free = np.concatenate([pick(3, W, 40, avoid=[c1, c2]), pick(W, 2 * W, 40, avoid=[c1 + W, c2 + W])])
    sums[3, free] = rng.integers(100, 249, 80) / 8.0
    # e
    on[4, :2 * W] = True
    on[4, 2 * W + 1] = True
    sums[4, 2 * W:] = np.array([3, 7, 3]) / 8.0
    # f
    sums[5, np.concatenate([pick(0, W, 30), pick(W, 2 * W, 30)])] = rng.integers(1, 7, 60) / 8.0
    sums[5, 2 * W:] = np.array([6, 6, 5]) / 8.0
    # g, h
    sums[6:] = rng.integers(-6, 7, (2, M)) / 8.0
    on[6:] = rng.random((2, M)) < 0.33
    i, j = np.nonzero(on)
    p = rng.permutation(len(i))
    ids = np.stack([i[p] + 1, j[p] + 1], axis=1).astype(np.int64)
    assert 200_000 <= len(ids) <= 400_000
    rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": np.ones(len(ids))}, "plays", [B.Entity("u"), B.Entity("v")], dims=[8, M])
    listed = RR.listed_of(ids, 8)
    scores = RR.scores_of(sums, 4.0, 0.5)
    ref = {}
    for sub in (False, True):
        rows = SUBSET if sub else np.arange(8)
        ref[sub, True] = RR.topk(scores[rows], 64, [listed[r] for r in rows])
        ref[sub, False] = RR.topk(scores[rows], 64)
    return dict(sums=sums, ids=ids, rel=rel, ref=ref, planned_b=planned_b)


@pytest.fixture(scope="module")
def window_case(B):
    return _window_case(B)


@pytest.mark.parametrize("K", [1, 5, 64])
def test_topk_lists_past_one_window_equal_the_restatement_exactly(B, ctx, window_case, K):
    """k_topk_rows over three windows of listed columns: the mask is zeroed again and filled relative to the window's first column,
    and the sorted list and its count pass from one window to the next.  Sums in eighths over four draws: every score is exact, and
    the lists equal RR.topk's to the bit, for all rows and for a permuted subset, the listed cells left out and kept."""
    from bdf_amd.engine import DeviceRelation, DeviceScores
    text = open(os.path.join(ROOT, "bayesiandatafusion.jl_amd", "csrc", "recommend.h")).read()
    assert "#define BDF_REC_WINDOW %d\n" % WINDOW in text
    sums, ref, planned_b = window_case["sums"], window_case["ref"], window_case["planned_b"]
    # on the CPU, before any launch: the reference lists themselves reach past window 0
    for exclude in (True, False):
        ei = ref[False, exclude][0][:, :K]
        wins = [set(int(w) for w in (ei[r][ei[r] > 0] - 1) // WINDOW) for r in range(4)]
        if K > 1:
            assert all(len(w) >= 2 for w in wins), (exclude, wins)       # each of the rows a .. d: entries of at least two windows
        else:                                                # (a list of one entry: the four rows' entries together, and row a's not in window 0)
            assert len(set.union(*wins)) >= 2 and wins[0] <= {1, 2}, (exclude, wins)
        assert np.array_equal(ei[1], planned_b[:K] + 1)      # row b: the plan itself, the smaller id first and the later tie refused
    for r in (2, 3):                                         # rows c and d: leaving the listed cells out changes the list
        assert not np.array_equal(ref[False, True][0][r, :K], ref[False, False][0][r, :K])
    assert np.count_nonzero(ref[False, True][0][4]) == 2     # row e: two candidates, both in window 2
    dr = DeviceRelation(ctx, window_case["rel"].data)
    draws, mean = 4.0, 0.5
    for sub, rows0 in ((False, None), (True, SUBSET)):
        n = 8 if rows0 is None else len(rows0)
        sc = DeviceScores(ctx, n, M_WIN, 3, 1, rows0)
        sc.write(ctx.tensor(sums if rows0 is None else sums[rows0]), draws)
        for exclude in (True, False):
            items, vals = sc.topk(K, mean, dr if exclude else None)
            ctx.sync()
            ei, ev = ref[sub, exclude][0][:, :K], ref[sub, exclude][1][:, :K]
            gi, gv = items.cpu().numpy(), vals.cpu().numpy()
            bad = [int(r) for r in np.nonzero((gi != ei).any(axis=1))[0]]
            assert gi.dtype == np.int32 and not bad, (sub, exclude, bad, gi[bad[0]][:8], ei[bad[0]][:8])
            assert np.array_equal(gv, ev, equal_nan=True)
            assert np.array_equal(gi == 0, np.isnan(gv))
            if exclude and rows0 is None:
                assert np.count_nonzero(gi[4]) == min(K, 2) and np.count_nonzero(gi[5]) == K
        sc.close()
    dr.close()


# ---- the grid-stride loops ------------------------------------------------------------------------------------------------------------
GRID_ROWS = 1 << 20                                          # rows that k_topk_rows and k_rec_metrics launch a workgroup for at most
GRID_PUSH = 65536                                            # workgroups of 256 quads that k_scores_push launches at most


def test_topk_and_metrics_past_the_row_grid(ctx):
    """2^20 + 3 rows of 3 columns, K = 2, nothing listed: the last three rows are the second trip of either kernel's row loop.  Sums in
    eighths with many ties; the lists against a stable sort of the negated scores (falling score, ties by rising column), which is
    itself held to RR.topk on the first 64 and the last 67 rows; the metrics of those lists on a few hundred relevant cells, three of
    them in the last three rows, against RR.metrics to 1e-12, the count of rows scored exactly."""
    import torch
    from bdf_amd.engine import DevicePairs, DeviceScores
    n, M, K, cut = GRID_ROWS + 3, 3, 2, 0.5
    rng = np.random.default_rng(31)
    sums = rng.integers(-2, 3, (n, M)) / 8.0
    draws, mean = 4.0, 0.5
    scores = RR.scores_of(sums, draws, mean)
    order = np.argsort(-scores, axis=1, kind="stable")[:, :K]
    ei, ev = (order + 1).astype(np.int32), np.take_along_axis(scores, order, axis=1)
    for part in (slice(0, 64), slice(n - 67, n)):
        ri, rv = RR.topk(scores[part], K)
        assert np.array_equal(ei[part], ri) and np.array_equal(ev[part], rv)
    assert np.count_nonzero(scores[:, 0] == scores[:, 1]) > n // 10
    sc = DeviceScores(ctx, n, M, 3, 1)
    sc.write(ctx.tensor(sums), draws)
    items, vals = sc.topk(K, mean)
    ctx.sync()
    gi, gv = items.cpu().numpy(), vals.cpu().numpy()
    assert np.array_equal(gi[:GRID_ROWS], ei[:GRID_ROWS]) and np.array_equal(gv[:GRID_ROWS], ev[:GRID_ROWS]), "the first trip: rows 0 .. 2^20 - 1"
    assert np.array_equal(gi[GRID_ROWS:], ei[GRID_ROWS:]) and np.array_equal(gv[GRID_ROWS:], ev[GRID_ROWS:]), \
        ("the second trip of k_topk_rows' row loop: the last three rows", gi[GRID_ROWS:], ei[GRID_ROWS:])
    # the metrics: 300 rows somewhere and the last three with test cells, the relevant ones partly in the lists
    rows = np.concatenate([rng.permutation(GRID_ROWS)[:300], np.arange(GRID_ROWS, n)])
    cells = []
    for q, r in enumerate(rows):
        if q % 9 == 4 and q < 300:
            cells.append((r + 1, int(ei[r, 0]), 0.0))         # a held-out cell below the cut alone: the row is not scored
            continue
        cells.append((r + 1, int(ei[r, q % 2]), 1.0))         # a hit at place 1 or 2
        if q % 3 == 0:
            cells.append((r + 1, 6 - int(ei[r, 0]) - int(ei[r, 1]), 1.0))      # and the column that is not in the list
    cells =[cells[q] for q in rng.permutation(len(cells))]
    ids, tv = np.array([c[:2] for c in cells], dtype=np.int64), np.array([c[2] for c in cells])
    pairs = DevicePairs(ctx, ids, tv)
    out = sc.metrics(items, K, pairs, cut)
    ctx.sync()
    # (rows without a relevant cell are left out by the definition: the restatement is run on the rows that have a test cell)
    has = np.unique(ids[:, 0] - 1)
    exp = RR.metrics(gi[has], RR.relevant_of(ids, tv, cut, len(has), has))
    got = out.cpu().numpy()
    print(f"metrics over {n} rows: device {got}, restatement {exp}")
    assert got[3] == exp[3] and exp[3] >= 250, "rows scored (the last three rows are the second trip of k_rec_metrics' row loop)"
    assert np.all(np.abs(got[:3] - np.array(exp[:3])) <= 1e-12)
    assert 0.0 < exp[0] < 1.0 and 0.0 < exp[1] < 1.0
    assert items.dtype == torch.int32
    sc.close()
    pairs.close()


def test_push_past_65536_workgroups(ctx):
    """one row against 2^20 + 1 columns at D = 64: 16 x (2^20 + 2) quads, 32 more than 65,536 workgroups of 256 take in one trip -- the
    last block of four d of the last 32 columns is the second trip of k_scores_push's loop.  Two draws through a ring of one slot
    (the second draw has the first one's V: half the host's work)"""
    n_rows, D, M = 1, 64, GRID_ROWS + 1
    quads = (n_rows + M) * ((D + 3) // 4)
    assert GRID_PUSH * 256 < quads <= 2 * GRID_PUSH * 256
    rng = np.random.default_rng(13)
    V = rng.standard_normal((M, D))
    draws = [(rng.standard_normal((n_rows, D)), V) for _ in range(2)]
    Vd = _guarded(ctx, V)
    dev = [(_guarded(ctx, U), Vd) for U, _ in draws]
    got, guard = _accumulate(ctx, dev, n_rows, M, D, 1)
    exp, mag = RR.score_sum(draws)
    assert np.isnan(guard).all() and not np.isnan(got).any()
    err = np.abs(got - exp) / mag
    print(f"push past {GRID_PUSH} workgroups: largest |device - restatement| / sum|terms| = {err.max():.2e}, over the last 32 columns {err[0, -32:].max():.2e}")
    assert err.max() <= ACC_TOL, int(np.argmax(err))
    assert got[0, -1] != 0.0 and got[0, 1 << 20] != 0.0


def test_topk_without_draws_has_no_candidates(ctx):
    from bdf_amd.engine import DeviceScores
    sc = DeviceScores(ctx, 3, 70, 4, 2)
    items, vals = sc.topk(5, 1.0)
    ctx.sync()
    assert not items.cpu().numpy().any() and np.isnan(vals.cpu().numpy()).all()
    sc.close()


# ---- the metrics ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 10])
def test_metrics_equal_the_restatement(ctx, K):
    import torch
    from bdf_amd.engine import DevicePairs, DeviceScores
    n, M, cut = 40, 50, 0.5
    rng = np.random.default_rng(20 + K)
    items, _ = RR.topk(rng.integers(0, 9, (n, M)) / 8.0, K)
    items[5, K - 1:] = 0                                     # a list that ends early: padding never hits
    relevant = [set() for _ in range(n)]
    for i in range(n):
        if i % 7 == 0:
            continue                                          # n_i = 0: left out
        size = K + 5 if i % 5 == 0 else int(rng.integers(1, 4))          # n_i > K
        relevant[i] = set(int(x) for x in rng.permutation(M)[:size] + 1)
    relevant[1].add(int(items[1, 0]))                         # a relevant item at list position 1 ...
    relevant[2] = {int(items[2, K - 1])}                      # ... and at position K
    relevant[3] = set(int(x) for x in range(1, M + 1)) - set(int(x) for x in items[3])      # no hit
    cells = [(i + 1, j, 1.0) for i in range(n) for j in sorted(relevant[i])]
    cells += [(i + 1, int(items[i, 0]), 0.0) for i in range(0, n, 7)]                       # held-out cells at or below the cut
    cells += [(4, 7, 0.5)]
    relevant_cut = RR.relevant_of(np.array([c[:2] for c in cells]), [c[2] for c in cells], cut, n)
    assert relevant_cut[1] == relevant[1] and not relevant_cut[0]
    order = rng.permutation(len(cells))
    pairs = DevicePairs(ctx, np.array([cells[q][:2] for q in order], dtype=np.int64), np.array([cells[q][2] for q in order]))
    sc = DeviceScores(ctx, n, M, 3, 1)
    sc.write(ctx.zeros(n * M), 1.0)
    out = sc.metrics(ctx.tensor(items, dtype=torch.int32), K, pairs, cut)
    ctx.sync()
    got, exp = out.cpu().numpy(), RR.metrics(items, relevant_cut)
    print(f"metrics K={K}: device {got}, restatement {exp}")
    assert got[3] == exp[3] == n - len(range(0, n, 7))
    assert np.all(np.abs(got[:3] - np.array(exp[:3])) <= 1e-12)
    assert 0.0 < exp[0] < 1.0 and 0.0 < exp[1] < 1.0
    sc.close()
    pairs.close()


# ---- macau() end to end ---------------------------------------------------------------------------------------------------------------
CHILD = textwrap.dedent('''
    import sys
    import numpy as np
    sys.path.insert(0, %r); sys.path.insert(0, %r)
    import bdf_amd as B
    import background_restatement as BR
    out, d = sys.argv[1], {}
    ids, y, _ = BR.listing()
    on = np.zeros((37, 29), dtype=bool)
    on[ids[:, 0] - 1, ids[:, 1] - 1] = True
    free = np.argwhere(~on)
    test = free[np.random.default_rng(5).permutation(len(free))[:120]] + 1
    tv = np.resize([1.0, 0.0, 1.0], len(test))
    for D in (5, 32, 40):
        for rec in (1, 0):
            rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "plays", [B.Entity("u"), B.Entity("v")], class_cut=0.5, alpha=2.0, dims=[37, 29])
            B.setTest(rel, {"u": test[:, 0], "v": test[:, 1], "y": tv})
            B.setBackground(rel, 0.2)
            if rec:
                B.setRecommend(rel, 6, batch=2)
            rd = B.RelationData(rel)
            res = B.macau(rd, num_latent=D, burnin=3, psamples=5, verbose=False, seed=17, full_prediction=True)
            key = "%%d_%%d_" %% (D, rec)
            d[key + "native"] = np.array(int(rd._engine.native))
            d[key + "has"] = np.array(int("recommend" in res))
            d[key + "full"], d[key + "pred"] = res["predictions_full"], res["predictions"]["pred"].to_numpy()
            d[key + "rmse"] = np.array([res["RMSE"], res["ROC"]])
            for k, en in enumerate(rd.entities):
                d[key + "S%%d" %% k] = en.model.sample.T
            if rec:
                r = res["recommend"]
                d[key + "items"], d[key + "scores"], d[key + "rows"] = r["items"], r["scores"], r["rows"]
                d[key + "metrics"] = np.array([r["recall"], r["ndcg"], r["hit_rate"], r["rows_scored"]])
                d[key + "k"] = np.array(r["k"])
            rd._engine.close()
    np.savez(out, test=test, tv=tv, **d)
''') % (ROOT, os.path.join(ROOT, "tests"))


@pytest.fixture(scope="module")
def runs():
    """BR.listing with a background, 3 + 5 iterations, batch 2 (two full flushes and a partial one), with and without setRecommend,
    on the native and on the step-by-step path: one child process per path"""
    return child(CHILD, no_native=False), child(CHILD, no_native=True)


@pytest.mark.parametrize("D", [5, 32, 40])
def test_macau_lists_agree_with_full_prediction_on_both_paths(runs, D):
    nat, step = runs
    key = "%d_1_" % D
    assert nat[key + "native"] == 1 and step[key + "native"] == 0
    for k in ("items", "scores", "rows", "metrics", "k"):
        assert nat[key + k].tobytes() == step[key + k].tobytes(), k          # the two paths: byte for byte
    items, scores, full = nat[key + "items"], nat[key + "scores"], nat[key + "full"]
    assert items.shape == (37, 6) and items.dtype == np.int32 and scores.dtype == np.float64 and nat[key + "k"] == 6
    assert np.array_equal(nat[key + "rows"], np.arange(1, 38))
    ids, _, _ = BR.listing()
    listed = RR.listed_of(ids, 37)
    for i in range(37):
        cand = np.array(sorted(set(range(29)) - listed[i]), dtype=np.int64)
        n = min(6, len(cand))
        assert np.count_nonzero(items[i]) == n and not items[i, n:].any() and np.isnan(scores[i, n:]).all()
        if n == 0:
            continue
        got = items[i, :n] - 1
        assert not (set(int(x) for x in got) & listed[i]) and len(set(got)) == n          # no listed cell, no repeat
        assert np.all(np.abs(scores[i, :n] - full[i, got]) <= 1e-12 * np.abs(full[i, got]))
        kth = np.sort(full[i, cand])[::-1][n - 1]
        assert np.all(full[i, got] >= kth - 1e-10)            # tie-tolerant: every returned item is among the K best
        assert np.all(np.diff(scores[i, :n]) <= 0)
    assert not items[1].any()                                 # BR.listing's row 2 lists every cell
    # the metrics against the restatement on the returned lists
    exp = RR.metrics(items, RR.relevant_of(nat["test"], nat["tv"], 0.5, 37))
    assert nat[key + "metrics"][3] == exp[3] > 0 and np.all(np.abs(nat[key + "metrics"][:3] - np.array(exp[:3])) <= 1e-12)


@pytest.mark.parametrize("D", [5, 32, 40])
def test_macau_without_setrecommend_returns_no_lists_and_the_same_chain(runs, D):
    for path in runs:
        with_, without = {k[len("%d_1_" % D):]: v for k, v in path.items() if k.startswith("%d_1_" % D)}, \
                         {k[len("%d_0_" % D):]: v for k, v in path.items() if k.startswith("%d_0_" % D)}
        assert with_["has"] == 1 and without["has"] == 0
        for k in without:
            if k != "has":
                assert with_[k].tobytes() == without[k].tobytes(), k


def test_macau_scores_a_row_subset_and_psamples_zero(B):
    ids, y, _ = BR.listing()
    rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "plays", [B.Entity("u"), B.Entity("v")], alpha=2.0, dims=[37, 29])
    B.setRecommend(rel, 4, rows=[30, 3, 1, 2], exclude_listed=False, batch=3)
    rd = B.RelationData(rel)
    res = B.macau(rd, num_latent=8, burnin=2, psamples=4, verbose=False, seed=3, full_prediction=True)
    r, full = res["recommend"], res["predictions_full"]
    rd._engine.close()
    assert np.array_equal(r["rows"], [30, 3, 1, 2]) and r["items"].shape == (4, 4) and "recall" not in r
    for q, row in enumerate([29, 2, 0, 1]):
        got = r["items"][q] - 1
        assert np.all(np.abs(r["scores"][q] - full[row, got]) <= 1e-12 * np.abs(full[row, got]))
        assert np.all(full[row, got] >= np.sort(full[row])[::-1][3] - 1e-10)
    B.assignToTest(rel, np.arange(1, 40))
    B.setRecommend(rel, 4)
    rd = B.RelationData(rel)
    r = B.macau(rd, num_latent=8, burnin=2, psamples=0, verbose=False, seed=3)["recommend"]
    rd._engine.close()
    assert not r["items"].any() and np.isnan(r["scores"]).all()
    assert np.isnan([r["recall"], r["ndcg"], r["hit_rate"]]).all()


def test_a_reused_engine_starts_the_sum_again(B):
    ids, y, _ = BR.listing()
    rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "plays", [B.Entity("u"), B.Entity("v")], alpha=2.0, dims=[37, 29])
    B.setRecommend(rel, 4, batch=2)
    rd = B.RelationData(rel)
    B.macau(rd, num_latent=8, burnin=2, psamples=3, verbose=False, seed=3)
    res = B.macau(rd, num_latent=8, burnin=0, psamples=3, verbose=False, seed=3, engine=rd._engine, reset_model=False, full_prediction=True)
    r, full = res["recommend"], res["predictions_full"]
    rd._engine.close()
    for i in range(37):
        got = r["items"][i][r["items"][i] > 0] - 1
        assert np.all(np.abs(r["scores"][i, :len(got)] - full[i, got]) <= 1e-12 * np.abs(full[i, got]))


# ---- it ranks -----------------------------------------------------------------------------------------------------------------------------
# tests/recommend_restatement.py::planted_ranking on the CPU, seeds 0, 1, 2: (recall@10, NDCG@10) of the background model's lists and
# of the popularity ranking
CPU_MODEL = [(0.4932, 0.8524), (0.4984, 0.8508), (0.4901, 0.8533)]
CPU_POPULARITY = [(0.1086, 0.1765), (0.0820, 0.1373), (0.1050, 0.1893)]
HALF_MARGIN = [0.5 * min(m[q] - p[q] for m, p in zip(CPU_MODEL, CPU_POPULARITY)) for q in (0, 1)]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_background_lists_beat_the_popularity_ranking(B, seed):
    """the planted data of DESIGN.md section 20 (p = sigma(3 u.v - 1), 300 x 200, D = 8, alpha = 10, c0 = 0.1, 20 + 20 iterations),
    K = 10: recall@10 and NDCG@10 of the device's lists exceed the popularity ranking's -- items by listed count, the listed cells
    left out, scored by the same restatement -- by at least half the smallest margin the CPU sampler showed over the three seeds"""
    train, test, tv = BR.planted(seed)
    rel = B.Relation({"u": train[:, 0], "v": train[:, 1], "y": np.ones(len(train))}, "plays", [B.Entity("u"), B.Entity("v")],
                     class_cut=0.5, alpha=10.0, dims=[300, 200])
    B.setTest(rel, {"u": test[:, 0], "v": test[:, 1], "y": tv})
    B.setBackground(rel, 0.1)
    B.setRecommend(rel, 10)
    rd = B.RelationData(rel)
    r = B.macau(rd, num_latent=8, burnin=20, psamples=20, verbose=False, seed=seed)["recommend"]
    rd._engine.close()
    relevant = RR.relevant_of(test, tv, 0.5, 300)
    exp = RR.metrics(r["items"], relevant)
    assert r["rows_scored"] == exp[3] and abs(r["recall"] - exp[0]) <= 1e-12 and abs(r["ndcg"] - exp[1]) <= 1e-12 and abs(r["hit_rate"] - exp[2]) <= 1e-12
    pop = RR.metrics(RR.topk(RR.popularity_scores(train, 300, 200), 10, RR.listed_of(train, 300))[0], relevant)
    print(f"planted implicit data, seed {seed}: recall@10 {r['recall']:.4f} (popularity {pop[0]:.4f}), NDCG@10 {r['ndcg']:.4f} (popularity {pop[1]:.4f})")
    assert r["recall"] - pop[0] >= HALF_MARGIN[0] and r["ndcg"] - pop[1] >= HALF_MARGIN[1]
