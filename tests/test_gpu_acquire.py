"""Acquisition lists from the moments of u.v over the posterior draws (setAcquire) on the device against
tests/acquire_restatement.py: the accumulate kernel at the edges of its tile, bit-identical over the batch size, with and without the
psum plane and over a row subset, with a precision read from device memory, and past 65,535 tiles; the lists of the three rules
exactly on dyadic planes, the score expression on random ones, the edges of the draw count and of the threshold; macau() end to end
on both iteration paths; and the spread of unlisted cells on planted data."""
import ctypes as C
import os
import textwrap

import numpy as np
import pytest

import acquire_restatement as AR
import background_restatement as BR
import recommend_restatement as RR
from both_paths import child

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the tile of k_acquire_accum (csrc/acquire.h: BDF_ACQ_TN x BDF_ACQ_TM; tests/test_acquire_host.py holds the two equal)
TN, TM = 64, 64
GUARD = 64                                                   # doubles of NaN behind every plane (BDF_REC_GUARD)
# the mean: 1e-13 of the largest per-draw sum_d |u_d v_d| of the cell, the bound of tests/test_gpu_recommend.py -- the restatement adds
# the same blocks of four d in the same order, the matrix instruction associates the four products of a block its own way
MEAN_TOL = 1e-13
# M2 relative to n mag^2 and psum relative to n: ten times the largest deviation measured over all ACC_CASES on an MI355X
# (M2: 1.48e-16; psum: 6.11e-16 -- DESIGN.md section 30), the margin for other seeds
M2_TOL = 1.48e-15
PSUM_TOL = 6.11e-15

_NS = [1, 15, 16, 17, TN - 1, TN, TN + 1, 2 * TN + 3]
_MS = [1, 15, 16, 17, TM - 1, TM, TM + 1, 2 * TM + 3]
_DS = [3, 16, 17, 32, 33, 64]
# the draws S in {1, 2, B - 1, B, B + 1, 2 B + 1} for B in {1, 3, 8}: every S is run at all three B
_SS = sorted({s for b in (1, 3, 8) for s in (1, 2, b - 1, b, b + 1, 2 * b + 1) if s >= 1})
ACC_CASES = [(_NS[q], _MS[q], _DS[q % 6], _SS[q % len(_SS)]) for q in range(8)] + \
            [(_NS[q], _MS[7 - q], _DS[(q + 3) % 6], _SS[(q + 5) % len(_SS)]) for q in range(8)]
MEAN_VALUE, THRESHOLD = 0.25, 0.5


def _guarded(ctx, a):
    """the device copy of the rows of `a` with 16 rows of NaN behind it; the view of the rows themselves"""
    full = np.vstack([a, np.full((16, a.shape[1]), np.nan)])
    return ctx.tensor(full)[:a.shape[0]]


def _planes(ctx, ac):
    """the planes and their guards on the host, after a flush"""
    out, guards = {}, []
    cells = ac.n_rows * ac.M
    for name in ("mean", "M2") + (("psum",) if ac.want_prob else ()):
        t = ac.read(name, 0, cells + GUARD)
        ctx.sync()
        got = t.cpu().numpy()
        out[name] = got[:cells].reshape(ac.n_rows, ac.M)
        guards.append(got[cells:])
    return out, np.concatenate(guards)


def _accumulate(ctx, draws_dev, alphas, n_rows, M, D, batch, rows0=None, threshold=THRESHOLD):
    """push the draws through a ring of `batch` slots; the planes and their guards on the host"""
    from bdf_amd.engine import DeviceAcquire
    ac = DeviceAcquire(ctx, n_rows, M, D, batch, rows0, MEAN_VALUE, threshold)
    for (U, V), a in zip(draws_dev, alphas):
        ac.push(U, V, a)
    out = _planes(ctx, ac)
    ac.close()
    return out


def test_accumulate_cases_cover_every_size_depth_and_count():
    assert len(_SS) == 8 and {c[3] for c in ACC_CASES} == set(_SS) and {c[2] for c in ACC_CASES} == set(_DS)
    assert {c[0] for c in ACC_CASES} == set(_NS) and {c[1] for c in ACC_CASES} == set(_MS)
    assert set(_SS) == {1, 2, 3, 4, 7, 8, 9, 17}


def _deviations(got, exp, mag, n):
    with np.errstate(invalid="ignore", divide="ignore"):
        d = {"mean": float(np.max(np.abs(got["mean"] - exp["mean"]) / mag)), "M2": float(np.max(np.abs(got["M2"] - exp["M2"]) / (n * mag * mag)))}
    if "psum" in exp:
        d["psum"] = float(np.max(np.abs(got["psum"] - exp["psum"]) / n))
    return d


@pytest.mark.parametrize("n_rows,M,D,S", ACC_CASES)
def test_accumulate_against_the_restatement_and_bit_identical_over_the_batch(ctx, n_rows, M, D, S):
    rng = np.random.default_rng(n_rows * 1000 + M + D + S)
    draws = [(rng.standard_normal((n_rows, D)), rng.standard_normal((M, D))) for _ in range(S)]
    alphas = [float(a) for a in rng.uniform(0.5, 4.0, S)]
    dev = [(_guarded(ctx, U), _guarded(ctx, V)) for U, V in draws]
    exp, mag = AR.fold(draws, None, alphas, MEAN_VALUE, THRESHOLD)
    first = None
    for batch in (1, 3, 8):
        got, guard = _accumulate(ctx, dev, alphas, n_rows, M, D, batch)
        assert np.isnan(guard).all()                          # nothing was stored behind a plane
        assert not any(np.isnan(p).any() for p in got.values())          # no guard row of the factors was read
        if first is None:
            first = got
            d = _deviations(got, exp, mag, S)
            print(f"accumulate n_rows={n_rows} M={M} D={D} S={S}: largest |device - restatement|: mean {d['mean']:.2e} of sum|terms|, "
                  f"M2 {d['M2']:.2e} of n mag^2, psum {d['psum']:.2e} of n")
            assert d["mean"] <= MEAN_TOL and d["M2"] <= M2_TOL and d["psum"] <= PSUM_TOL
        else:
            for name in first:
                assert np.array_equal(first[name], got[name]), (batch, name)          # the same bits wherever the flushes fall
    # without the psum plane: the other instantiation of the kernel leaves the same mean and M2
    plain, guard = _accumulate(ctx, dev, alphas, n_rows, M, D, 3, threshold=None)
    assert np.isnan(guard).all() and sorted(plain) == ["M2", "mean"]
    assert np.array_equal(plain["mean"], first["mean"]) and np.array_equal(plain["M2"], first["M2"])


def test_accumulate_reads_a_sampled_alpha_from_the_device(ctx):
    """alpha_dev points at another value for every draw and the host's alpha is wrong: the psum plane is the restatement's with the
    device's values, to the bit of the run that was handed the same values as host doubles"""
    from bdf_amd._lib import check, lib
    from bdf_amd.engine import DeviceAcquire
    n_rows, M, D, S = 17, TM + 1, 5, 4
    rng = np.random.default_rng(21)
    draws = [(rng.standard_normal((n_rows, D)), rng.standard_normal((M, D))) for _ in range(S)]
    alphas = [0.5, 3.0, 1.25, 7.0]
    dev = [(_guarded(ctx, U), _guarded(ctx, V)) for U, V in draws]
    on_dev = ctx.tensor(np.array(alphas))
    ac = DeviceAcquire(ctx, n_rows, M, D, 3, None, MEAN_VALUE, THRESHOLD)
    for b, (U, V) in enumerate(dev):
        check(lib().bdf_acquire_push(ac.handle, C.c_void_p(U.data_ptr()), C.c_void_p(V.data_ptr()), 1000.0, C.c_void_p(on_dev.data_ptr() + 8 * b)))
    got, guard = _planes(ctx, ac)
    ac.close()
    host, _ = _accumulate(ctx, dev, alphas, n_rows, M, D, 3)
    exp, mag = AR.fold(draws, None, alphas, MEAN_VALUE, THRESHOLD)
    wrong, _ = AR.fold(draws, None, [1000.0] * S, MEAN_VALUE, THRESHOLD)
    assert np.isnan(guard).all() and all(np.array_equal(got[k], host[k]) for k in got)
    assert np.max(np.abs(got["psum"] - exp["psum"])) / S <= PSUM_TOL < np.max(np.abs(got["psum"] - wrong["psum"])) / S
    # a host alpha that is not a precision is refused unless the device's is given
    ac = DeviceAcquire(ctx, n_rows, M, D, 3, None, MEAN_VALUE, THRESHOLD)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(Exception, match="alpha=.* must be positive and finite"):
            ac.push(dev[0][0], dev[0][1], bad)
    ac.close()


def test_accumulate_rows_subset_equals_the_same_rows_of_the_full_run(ctx):
    N, M, D, S = 2 * TN + 3, 2 * TM + 3, 17, 4
    rng = np.random.default_rng(11)
    draws = [(rng.standard_normal((N, D)), rng.standard_normal((M, D))) for _ in range(S)]
    alphas = [2.0, 1.0, 0.5, 3.0]
    dev = [(_guarded(ctx, U), _guarded(ctx, V)) for U, V in draws]
    full, _ = _accumulate(ctx, dev, alphas, N, M, D, 3)
    rows0 = rng.permutation(N)[:TN + 6]
    sub, guard = _accumulate(ctx, dev, alphas, len(rows0), M, D, 2, rows0)
    assert np.isnan(guard).all() and all(np.array_equal(sub[k], full[k][rows0]) for k in full)


def test_accumulate_past_65535_tiles(ctx):
    """one row of 65,536 tiles and a cell: the tile index is one flattened 64-bit number, no grid dimension caps it"""
    M, D, S = 65536 * TM + 1, 3, 2
    rng = np.random.default_rng(12)
    draws = [(rng.standard_normal((1, D)), rng.standard_normal((M, D))) for _ in range(S)]
    dev = [(_guarded(ctx, U), _guarded(ctx, V)) for U, V in draws]
    got, guard = _accumulate(ctx, dev, [1.0] * S, 1, M, D, 2, threshold=None)
    exp, mag = AR.fold(draws)
    d = _deviations(got, exp, mag, S)
    assert np.isnan(guard).all()
    assert d["mean"] <= MEAN_TOL and d["M2"] <= M2_TOL
    assert got["mean"][0, -1] != 0.0 and got["mean"][0, 65535 * TM] != 0.0 and got["M2"][0, -1] != 0.0


# ---- the lists --------------------------------------------------------------------------------------------------------------------
N_UCB, N_PROB = 5.0, 4.0          # the draws the planes stand for: M2 / (5 - 1) is exact, and 4 is a power of two
LIST_MEAN = 0.5


def _list_case(B, M, seed):
    """8 rows of dyadic planes with many equal scores -- mean in eighths, M2 = 4 (j / 8)^2 so that sd = j / 8 over 5 draws, psum whole
    numbers 0 .. 4; j comes back, and M2 = (n - 1) (j / 8)^2 serves another count of draws n -- and a relation that lists: row 0 every cell, row 1 none, row 2 the first column, row 3 the last, row 4 all but
    three (fewer candidates than K = 5), rows 5 .. 7 about a third"""
    rng = np.random.default_rng(seed)
    j = rng.integers(0, 5, (8, M))
    planes = {"mean": rng.integers(-6, 7, (8, M)) / 8.0, "M2": 4.0 * (j / 8.0) ** 2, "psum": rng.integers(0, 5, (8, M)).astype(np.float64)}
    on = rng.random((8, M)) < 0.33
    on[0, :], on[1, :], on[2, :], on[3, :] = True, False, False, False
    on[2, 0], on[3, M - 1] = True, True
    on[4, :] = True
    on[4, rng.permutation(M)[:3]] = False
    i, jj = np.nonzero(on)
    p = rng.permutation(len(i))
    ids = np.stack([i[p] + 1, jj[p] + 1], axis=1).astype(np.int64)
    rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": np.ones(len(ids))}, "assays", [B.Entity("u"), B.Entity("v")], dims=[8, M])
    return planes, j, ids, rel


RULE_CASES = [("ucb", 0.75, N_UCB), ("ucb", 0.0, N_UCB), ("sd", 0.0, N_UCB), ("prob_above", 0.0, N_PROB)]


@pytest.mark.parametrize("M", [1, 63, 64, 65, 257, 4097])
@pytest.mark.parametrize("K", [1, 5, 64])
def test_lists_of_the_three_rules_equal_the_restatement_exactly(B, ctx, M, K):
    from bdf_amd.engine import DeviceAcquire, DeviceRelation
    planes, j, ids, rel = _list_case(B, M, 300 + M)
    dr = DeviceRelation(ctx, rel.data)
    for rows0 in (None, np.array([6, 1, 0, 3, 4, 2])):       # (a subset: the listed columns come from the row's own id)
        n = 8 if rows0 is None else len(rows0)
        ac = DeviceAcquire(ctx, n, M, 3, 1, rows0, LIST_MEAN, 0.0)
        for rule, kappa, draws in RULE_CASES:
            mine = dict(planes, M2=(draws - 1.0) * (j / 8.0) ** 2)          # sd = j / 8 exactly over this count of draws
            if rows0 is not None:
                mine = {k: np.ascontiguousarray(v[rows0]) for k, v in mine.items()}
            ac.write({k: ctx.tensor(v) for k, v in mine.items()}, draws)
            scores = AR.scores_of(mine, draws, rule, kappa, LIST_MEAN)
            assert len(np.unique(scores)) < scores.size or M == 1          # equal scores: the item ids decide
            for exclude in (True, False):
                got = ac.topk(K, rule, kappa, dr if exclude else None)
                ctx.sync()
                got = {k: v.cpu().numpy() for k, v in got.items()}
                ei, ev = AR.topk(scores, K, RR.listed_of(ids, n, rows0) if exclude else None)
                assert got["items"].dtype == np.int32 and np.array_equal(got["items"], ei), (rule, rows0, exclude)
                assert np.array_equal(got["scores"], ev, equal_nan=True)
                assert np.array_equal(got["items"] == 0, np.isnan(got["scores"]))
                eg = AR.gathered(mine, draws, ei, LIST_MEAN)
                for k in ("mean", "sd", "prob"):
                    assert np.array_equal(got[k], eg[k], equal_nan=True), (rule, k)
                if exclude and rows0 is None:
                    assert not got["items"][0].any()          # every cell listed: padding only
                    assert np.count_nonzero(got["items"][4]) == min(K, 3, M)
                    assert np.count_nonzero(got["items"][1]) == min(K, M)
        ac.close()
    dr.close()


def _ulp(x):
    return np.spacing(np.abs(x))


def test_the_score_expression_on_random_planes(ctx):
    """the score plane of every rule against numpy on random planes: within 4 ulp of max(|m|, kappa sd) -- a division, a square root and
    a multiply-add, each correctly rounded or contracted once"""
    from bdf_amd.engine import DeviceAcquire
    n, M, draws, kappa, mv = 9, 301, 7.0, 1.7, 0.3
    rng = np.random.default_rng(33)
    planes = {"mean": rng.standard_normal((n, M)) * 2, "M2": rng.random((n, M)) * 9, "psum": rng.random((n, M)) * draws}
    ac = DeviceAcquire(ctx, n, M, 3, 1, None, mv, 0.0)
    ac.write({k: ctx.tensor(v) for k, v in planes.items()}, draws)
    for rule in AR.RULES:
        ac.topk(3, rule, kappa)
        t = ac.read("score")
        ctx.sync()
        got = t.cpu().numpy().reshape(n, M)
        m, sd = planes["mean"] + mv, np.sqrt(planes["M2"] / (draws - 1.0))
        exp = {"ucb": m + kappa * sd, "sd": sd, "prob_above": planes["psum"] / draws}[rule]
        scale = np.maximum(np.abs(m), kappa * sd) if rule == "ucb" else exp
        worst = float(np.max(np.abs(got - exp) / _ulp(scale)))
        print(f"score plane, rule {rule}: largest |device - numpy| = {worst:.2f} ulp of max(|m|, kappa sd)")
        assert worst <= 4.0
    ac.close()


def test_the_edges_of_the_draw_count(ctx):
    from bdf_amd.engine import DeviceAcquire
    n, M = 3, 70
    rng = np.random.default_rng(5)
    planes = {"mean": rng.standard_normal((n, M)), "M2": np.zeros((n, M)), "psum": rng.random((n, M))}
    ac = DeviceAcquire(ctx, n, M, 4, 2, None, 1.0, 0.0)
    dev = {k: ctx.tensor(v) for k, v in planes.items()}
    # nothing pushed or written: no candidates for any rule
    for rule in AR.RULES:
        got = ac.topk(5, rule, 1.0)
        ctx.sync()
        assert not got["items"].cpu().numpy().any() and all(np.isnan(got[k].cpu().numpy()).all() for k in ("scores", "mean", "sd", "prob")), rule
    ac.write(dev, 1)
    for rule in ("ucb", "sd"):                               # one draw: no spread, no candidates
        got = ac.topk(5, rule, 1.0)
        ctx.sync()
        assert not got["items"].cpu().numpy().any() and np.isnan(got["scores"].cpu().numpy()).all(), rule
    got = ac.topk(5, "prob_above")                            # ... but a probability, and the mean beside it
    ctx.sync()
    got = {k: v.cpu().numpy() for k, v in got.items()}
    ei, ev = AR.topk(AR.scores_of(planes, 1, "prob_above"), 5)
    assert np.array_equal(got["items"], ei) and np.array_equal(got["scores"], ev) and np.array_equal(got["prob"], ev)
    assert np.array_equal(got["mean"], AR.gathered(planes, 1, ei, 1.0)["mean"]) and np.isnan(got["sd"]).all()
    ac.write(dev, 0)
    for rule in AR.RULES:
        got = ac.topk(5, rule, 1.0)
        ctx.sync()
        assert not got["items"].cpu().numpy().any() and np.isnan(got["scores"].cpu().numpy()).all(), rule
    ac.close()
    # no psum plane: prob_above is refused, not ranked from nothing
    ac = DeviceAcquire(ctx, n, M, 4, 2)
    with pytest.raises(Exception, match="no psum plane is kept"):
        ac.topk(5, "prob_above")
    ac.close()


@pytest.mark.parametrize("threshold,prob", [(1e300, 0.0), (-1e300, 1.0)])
def test_a_threshold_out_of_reach_gives_probability_exactly_zero_and_one(ctx, threshold, prob):
    from bdf_amd.engine import DeviceAcquire
    n, M, D = 5, 33, 6
    rng = np.random.default_rng(8)
    ac = DeviceAcquire(ctx, n, M, D, 2, None, 0.5, threshold)
    for _ in range(3):
        ac.push(ctx.tensor(rng.standard_normal((n, D))), ctx.tensor(rng.standard_normal((M, D))), 2.0)
    got = ac.topk(4, "prob_above")
    ctx.sync()
    got = {k: v.cpu().numpy() for k, v in got.items()}
    assert np.all(got["prob"] == prob) and np.all(got["scores"] == prob) and np.array_equal(got["items"], np.tile(np.arange(1, 5, dtype=np.int32), (n, 1)))
    ac.close()


# ---- macau() end to end -----------------------------------------------------------------------------------------------------------
PSAMPLES = 5
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

    def run(D, mode, alpha_sample=False):
        rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "assays", [B.Entity("u"), B.Entity("v")], class_cut=0.5, alpha=2.0, dims=[37, 29])
        B.setTest(rel, {"u": test[:, 0], "v": test[:, 1], "y": tv})
        rel.model.alpha_sample = alpha_sample
        if mode == "top":
            B.setAcquire(rel, 6, kappa=0.0, batch=2)
        elif mode == "rec":
            B.setRecommend(rel, 6, batch=2)
        elif mode == "all":
            B.setAcquire(rel, 29, kappa=1.5, exclude_listed=False, batch=2)
        elif mode == "prob":
            B.setAcquire(rel, 29, rule="prob_above", threshold=1.0, exclude_listed=False, batch=3)
        rd = B.RelationData(rel)
        res = B.macau(rd, num_latent=D, burnin=3, psamples=%d, verbose=False, seed=17, full_prediction=True)
        key = "%%s%%d_%%s_" %% ("as" if alpha_sample else "", D, mode)
        d[key + "native"] = np.array(int(rd._engine.native))
        d[key + "has"] = np.array(int("acquire" in res))
        d[key + "full"], d[key + "pred"], d[key + "stdev"] = res["predictions_full"], res["predictions"]["pred"].to_numpy(), res["predictions"]["stdev"].to_numpy()
        d[key + "rmse"] = np.array([res["RMSE"], res["ROC"]])
        d[key + "mean_value"] = np.array(rel.model.mean_value)
        for k, en in enumerate(rd.entities):
            d[key + "S%%d" %% k] = en.model.sample.T
        if "acquire" in res:
            for k, v in res["acquire"].items():
                if v is not None and not isinstance(v, str):
                    d[key + "acq_" + k] = np.asarray(v)
        if "recommend" in res:
            d[key + "rec_items"], d[key + "rec_scores"] = res["recommend"]["items"], res["recommend"]["scores"]
        rd._engine.close()

    for D in (5, 32, 40):
        for mode in ("none", "top", "rec", "all"):
            run(D, mode)
    for mode in ("none", "prob"):
        run(5, mode, alpha_sample=True)
    np.savez(out, test=test, tv=tv, **d)
''') % (ROOT, os.path.join(ROOT, "tests"), PSAMPLES)


@pytest.fixture(scope="module")
def runs():
    """BR.listing as plain Gaussian measurements with 120 held-out cells, 3 + 5 iterations; per D: no list, the six best by the mean
    (kappa = 0), setRecommend's six, and every item by ucb with the listed cells kept (k = M: the lists hold the whole planes); at
    D = 5 also with a sampled alpha, without a list and by prob_above.  One child process per iteration path"""
    return child(CHILD, no_native=False), child(CHILD, no_native=True)


def _of(path, key):
    return {k[len(key):]: v for k, v in path.items() if k.startswith(key)}


@pytest.mark.parametrize("D", [5, 32, 40])
def test_macau_on_both_paths_and_the_chain_is_untouched(runs, D):
    nat, step = runs
    assert nat["%d_all_native" % D] == 1 and step["%d_all_native" % D] == 0
    for mode in ("top", "all"):
        a, b = _of(nat, "%d_%s_acq_" % (D, mode)), _of(step, "%d_%s_acq_" % (D, mode))
        assert sorted(a) == ["items", "k", "kappa", "mean", "rows", "scores", "sd"]          # (rule is a string, threshold None: not saved)
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), (mode, k)          # the two paths: byte for byte
    for path in runs:
        without = _of(path, "%d_none_" % D)
        assert without["has"] == 0
        for mode in ("top", "all"):
            with_ = _of(path, "%d_%s_" % (D, mode))
            assert with_["has"] == 1
            for k in without:
                if k != "has":
                    assert with_[k].tobytes() == without[k].tobytes(), (mode, k)          # RMSE, ROC, the predictions, the last draw


@pytest.mark.parametrize("D", [5, 32, 40])
def test_macau_planes_agree_with_full_prediction_and_the_test_cells_stdev(runs, D):
    """k = M with the listed cells kept: every row's list is a permutation of the items, so the gathered mean and sd are the planes.
    mean + mean_value against predictions_full, which is sum_b (u_b.v_b + mean_value) / n by a dense product: two orders of adding n
    terms of magnitude at most |m| + |mean_value| + sqrt(n - 1) sd (no draw is further from the mean than sqrt M2), 1e-12 of it as in
    tests/test_gpu_recommend.py.  sd against result["predictions"].stdev at the test cells: the driver's is
    sqrt((sum y^2 - n avg^2) / (n - 1)) with y = u.v + mean_value, the same n - 1 divisor, defined for n >= 3 and equal to sd when
    nothing is clamped; as a difference of two sums of n squares it carries (n + 4) 2^-52 (sum y^2 + n avg^2) / (n - 1) of rounding in
    the variance, which is the bound"""
    nat, _ = runs
    r, base = _of(nat, "%d_all_acq_" % D), _of(nat, "%d_all_" % D)
    n, mv = PSAMPLES, float(base["mean_value"])
    items, full = r["items"], base["full"]
    assert items.shape == (37, 29) and np.array_equal(np.sort(items, axis=1), np.tile(np.arange(1, 30), (37, 1)))
    assert np.array_equal(r["rows"], np.arange(1, 38)) and r["k"] == 29 and r["kappa"] == 1.5
    mean, sd = np.empty((37, 29)), np.empty((37, 29))
    np.put_along_axis(mean, items - 1, r["mean"], axis=1)
    np.put_along_axis(sd, items - 1, r["sd"], axis=1)
    scale = np.abs(full) + abs(mv) + np.sqrt(n - 1.0) * sd
    worst = float(np.max(np.abs(mean - full) / scale))
    print(f"D={D}: mean plane + mean_value against predictions_full: {worst:.2e} of |m| + |mean_value| + sqrt(n - 1) sd")
    assert worst <= 1e-12
    # the scores are the expression of the gathered moments, and fall along every list
    assert np.array_equal(r["scores"], 1.5 * r["sd"] + r["mean"]) and np.all(np.diff(r["scores"], axis=1) <= 0)
    t = nat["test"] - 1
    avg, stdev = base["pred"], base["stdev"]
    var_bound = (n + 4) * 2.0 ** -52 * ((n - 1) * stdev ** 2 + 2 * n * avg ** 2) / (n - 1)
    got = sd[t[:, 0], t[:, 1]]
    worst = float(np.max(np.abs(got ** 2 - stdev ** 2) / var_bound))
    print(f"D={D}: sd plane at the 120 test cells against predictions.stdev: {worst:.2e} of the variance's rounding bound")
    assert np.all(stdev > 0) and worst <= 1.0


@pytest.mark.parametrize("D", [5, 32, 40])
def test_kappa_zero_ranks_as_setrecommend_does(runs, D):
    """the same seed, the same chain: the six best by mean + 0 sd are setRecommend's six wherever the neighbouring scores of its list
    differ by more than the two means' rounding (1e-12 of the score's scale, as above); the scores agree to it everywhere"""
    nat, _ = runs
    a, rec = _of(nat, "%d_top_acq_" % D), _of(nat, "%d_rec_" % D)
    ai, ri, rs = a["items"], rec["rec_items"], rec["rec_scores"]
    assert ai.shape == ri.shape == (37, 6)
    bound = 1e-12 * (np.abs(rs) + 1.0 + np.sqrt(PSAMPLES - 1.0) * np.nan_to_num(a["sd"]))
    assert np.array_equal(np.isnan(a["scores"]), np.isnan(rs)) and np.all(np.nan_to_num(np.abs(a["scores"] - rs)) <= np.nan_to_num(bound) * 2 + 1e-300)
    for i, q in np.argwhere(ai != ri):
        near = [abs(rs[i, q] - rs[i, p]) for p in (q - 1, q + 1) if 0 <= p < 6 and not np.isnan(rs[i, p])]
        assert near and min(near) <= 2 * bound[i, q], (i, q)
    ids, _, _ = BR.listing()
    listed = RR.listed_of(ids, 37)
    for i in range(37):
        assert not (set(int(x) - 1 for x in ai[i] if x > 0) & listed[i])
    assert not ai[1].any()                                    # BR.listing's row 2 lists every cell


def test_macau_with_a_sampled_alpha_on_both_paths(runs):
    """alpha_sample: the native iteration hands the device's alpha to the push, the step-by-step one the double the host read from it
    -- the same lists, probabilities and moments to the byte; prob lies in (0, 1), orders the list, and the chain is the one without"""
    nat, step = runs
    a, b = _of(nat, "as5_prob_acq_"), _of(step, "as5_prob_acq_")
    assert sorted(a) == ["items", "k", "kappa", "mean", "prob", "rows", "scores", "sd", "threshold"] and a["threshold"] == 1.0
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert np.array_equal(a["scores"], a["prob"]) and np.all((a["prob"] > 0) & (a["prob"] < 1)) and np.all(np.diff(a["prob"], axis=1) <= 0)
    # a cell whose mean is far above the threshold is likelier to exceed it than one far below
    hi, lo = a["mean"] > 1.0 + 2 * a["sd"] + 1.5, a["mean"] < 1.0 - 2 * a["sd"] - 1.5
    assert (not hi.any() or a["prob"][hi].min() > 0.5) and (not lo.any() or a["prob"][lo].max() < 0.5)
    for path in runs:
        with_, without = _of(path, "as5_prob_"), _of(path, "as5_none_")
        for k in without:
            if k != "has":
                assert with_[k].tobytes() == without[k].tobytes(), k


def _plain(B):
    ids, y, _ = BR.listing()
    return B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "assays", [B.Entity("u"), B.Entity("v")], alpha=2.0, dims=[37, 29])


def test_macau_scores_a_row_subset_and_psamples_zero_and_one(B):
    rel = _plain(B)
    B.setAcquire(rel, 4, rule="sd", rows=[30, 3, 1, 2], exclude_listed=False, batch=3)
    rd = B.RelationData(rel)
    sub = B.macau(rd, num_latent=8, burnin=2, psamples=4, verbose=False, seed=3)["acquire"]
    rd._engine.close()
    B.setAcquire(rel, 4, rule="sd", exclude_listed=False, batch=2)
    rd = B.RelationData(rel)
    res = B.macau(rd, num_latent=8, burnin=2, psamples=4, verbose=False, seed=3)
    full = res["acquire"]
    rd._engine.close()
    assert sub["rule"] == "sd" and sub["threshold"] is None and "prob" not in sub and np.array_equal(sub["rows"], [30, 3, 1, 2])
    for k in ("items", "scores", "mean", "sd"):
        assert sub[k].shape == (4, 4) and np.array_equal(sub[k], full[k][[29, 2, 0, 1]]), k          # the same rows of the full run, to the bit
    assert np.array_equal(sub["scores"], sub["sd"]) and np.all(sub["sd"] > 0)
    for psamples, rule, kw in ((0, "ucb", {}), (1, "ucb", {}), (0, "prob_above", {"threshold": 0.0})):
        B.setAcquire(rel, 4, rule=rule, **kw)
        rd = B.RelationData(rel)
        r = B.macau(rd, num_latent=8, burnin=2, psamples=psamples, verbose=False, seed=3)["acquire"]
        rd._engine.close()
        assert not r["items"].any() and np.isnan(r["scores"]).all() and np.isnan(r["mean"]).all() and np.isnan(r["sd"]).all(), (psamples, rule)
    B.setAcquire(rel, 4, rule="prob_above", threshold=0.0)
    rd = B.RelationData(rel)
    r = B.macau(rd, num_latent=8, burnin=2, psamples=1, verbose=False, seed=3)["acquire"]
    rd._engine.close()
    assert np.count_nonzero(r["items"][0]) == 4 and np.isnan(r["sd"]).all() and np.array_equal(np.isnan(r["prob"]), r["items"] == 0)


def test_a_reused_engine_starts_the_planes_again(B):
    rel = _plain(B)
    B.setAcquire(rel, 29, kappa=0.0, exclude_listed=False, batch=2)
    rd = B.RelationData(rel)
    B.macau(rd, num_latent=8, burnin=2, psamples=3, verbose=False, seed=3)
    res = B.macau(rd, num_latent=8, burnin=0, psamples=3, verbose=False, seed=3, engine=rd._engine, reset_model=False, full_prediction=True)
    r, full = res["acquire"], res["predictions_full"]
    rd._engine.close()
    got = np.take_along_axis(full, r["items"] - 1, axis=1)
    assert np.all(np.abs(r["mean"] - got) <= 1e-12 * (np.abs(got) + 1.0 + np.sqrt(2.0) * r["sd"]))          # three draws, not six


# ---- the spread ---------------------------------------------------------------------------------------------------------------------
# tests/acquire_restatement.py::cpu_spread on the CPU, seeds 0, 1, 2: the median sd over the unlisted cells of the rows with 2 listed
# cells and of the rows with 40
CPU_SPREAD = [(0.9428, 0.2654), (0.8545, 0.2678), (0.8390, 0.2703)]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_a_row_with_few_listed_cells_is_less_certain(B, seed):
    """planted Gaussian data, 40 x 60: rows that list 2 cells against rows that list 40, D = 4, alpha = 5, 20 + 30 iterations.  The median
    sd over the unlisted cells is larger in the sparse group, as it was in the numpy chain for every seed"""
    assert all(s > f for s, f in CPU_SPREAD)
    sp = AR.SPREAD
    ids, y = AR.planted_spread(seed)
    rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "assays", [B.Entity("u"), B.Entity("v")], alpha=sp["alpha"], dims=[sp["N"], sp["M"]])
    B.setAcquire(rel, sp["M"], rule="sd", exclude_listed=False)
    rd = B.RelationData(rel)
    r = B.macau(rd, num_latent=sp["D"], burnin=sp["burnin"], psamples=sp["psamples"], verbose=False, seed=seed)["acquire"]
    rd._engine.close()
    sd = np.empty((sp["N"], sp["M"]))
    np.put_along_axis(sd, r["items"] - 1, r["sd"], axis=1)
    sparse, full = AR.unlisted_medians(sd, ids)
    print(f"planted spread, seed {seed}: median sd of unlisted cells {sparse:.4f} (2 listed) against {full:.4f} (40 listed); CPU {CPU_SPREAD[seed]}")
    assert sparse > full
