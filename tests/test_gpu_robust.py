"""The robust (Student-t) noise model and observation weights on the GPU: the weighted row system of
k_rows_w against numpy (two, three and four modes; row lengths on the software pipeline's trip boundaries; weights together with
linear_values; launches that mix a weighted and an unweighted relation), unit weights against the unweighted general path bit for bit, bdf_robust_draw and bdf_pairs_weighted_sse
against the restatement (tests/robust_restatement.py), whole macau() iterations against the restated chain on both iteration
paths, the Gaussian chain untouched by a robust engine in the same process, planted outliers, and the errors of the C ABI."""
import ctypes as C
import os
import textwrap

import numpy as np
import pytest

from both_paths import child
import robust_restatement as RR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1234


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _facs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _terms(*rels):
    """rels: (DeviceRelation, mode0, alpha, mean, [factor tensors], linear tensor | None, weight tensor | None) per relation"""
    from bdf_amd._lib import Term
    terms = (Term * len(rels))()
    for t, (dr, mode0, alpha, mean, facs, lin, weights) in enumerate(rels):
        terms[t].rel, terms[t].mode, terms[t].alpha, terms[t].mean_value = dr.handle, mode0, alpha, mean
        terms[t].linear_values = lin.data_ptr() if lin is not None else None
        terms[t].obs_precision = weights.data_ptr() if weights is not None else None
        for k, f in enumerate(facs):
            terms[t].factors[k] = f.data_ptr() if f is not None else None
    return terms


def _term(dr, mode0, alpha, mean, facs, lin=None, weights=None):
    return _terms((dr, mode0, alpha, mean, facs, lin, weights))


# ---- (a) the weighted row system ---------------------------------------------------------------------------------------------
def _system_problem(rng, n_modes, D):
    """N = 40 rows, other modes 23 (and 11, and 7), n = 1003 observations; row 2 has no observation, row 5 holds 300; weights log-uniform
    on 1e-3 .. 1e3 with both ends present.  Factor entries are N(0, 0.3^2): with weights up to 1e3 the off-diagonal entries
    of P then stay of the size (tens to hundreds; the diagonal of the long row reaches a few thousand and is held by the relative
    part) at which the absolute tolerance of tests/test_gpu_rows.py, 1e-12, was set for unit weights."""
    dims = [40, 23, 11, 7][:n_modes]
    n = 1003
    ids = np.stack([rng.integers(1, d + 1, n) for d in dims], axis=1).astype(np.int64)
    ids[ids[:, 0] == 3, 0] = 4
    ids[:300, 0] = 6
    vals = rng.standard_normal(n)
    w = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), n))
    w[0], w[1], w[500], w[501] = 1e-3, 1e3, 1e-3, 1e3
    facs = [0.3 * rng.standard_normal((d, D)) for d in dims]
    A = rng.standard_normal((D, D))
    Lam = A @ A.T / D + np.eye(D)
    return dims, ids, vals, w, facs, Lam


@pytest.mark.parametrize("n_modes", [2, 3, 4])
@pytest.mark.parametrize("D", [5, 16, 17, 32, 33, 64])
def test_weighted_row_system_and_draw(B, O, D, n_modes):
    """bdf_row_system and bdf_sample_rows with obs_precision against numpy, at the tolerances tests/test_gpu_rows.py holds them to
    (1e-12 for the system, 1e-8 / 1e-9 for the sample); item size 64: the row of 300 observations is split over several items.
    A shared prior mean, and (every D, two modes) a prior mean per row.  Four modes: accumulate_reg<DP, 3, true>, one k-step per
    trip."""
    from bdf_amd._lib import check, lib
    rng = np.random.default_rng(500 + 10 * D + n_modes)
    dims, ids, vals, w, facs, Lam = _system_problem(rng, n_modes, D)
    N = dims[0]
    assert not np.any(ids[:, 0] == 3) and np.sum(ids[:, 0] == 6) >= 300
    c2 = B.Context(seed=SEED)
    c2.set_item_size(64)
    dr = B.DeviceRelation(c2, B.IndexedDF((ids, vals), dims))
    ft = [None] + [c2.tensor(f) for f in facs[1:]]
    wt, Lam_t = c2.tensor(w), c2.tensor(Lam)
    alpha, mean = 1.7, 0.25
    terms = _term(dr, 0, alpha, mean, ft, weights=wt)
    worst = 0.0
    for mu_rows in ([False, True] if n_modes == 2 else [False]):
        mu = rng.standard_normal((N, D)) if mu_rows else rng.standard_normal(D)
        mu_t = c2.tensor(mu)
        P_t, b_t = c2.zeros(N, D, D), c2.zeros(N, D)
        check(lib().bdf_row_system(c2.handle, D, N, 1, terms, _p(mu_t), int(mu_rows), _p(Lam_t), _p(P_t), _p(b_t)))
        c2.sync()
        P, b = P_t.cpu().numpy(), b_t.cpu().numpy()
        c2.set_sweep(3)
        out_t = c2.zeros(N, D)
        check(lib().bdf_sample_rows(c2.handle, D, N, 1, terms, _p(mu_t), int(mu_rows), _p(Lam_t), 11, 0, 1, _p(out_t), None))
        c2.sync()
        out = out_t.cpu().numpy()
        for row in range(N):
            mu_i = mu[row] if mu_rows else mu
            Pe, be = RR.row_system(ids, vals, w, 0, row, alpha, mean, facs, mu_i, Lam)
            worst = max(worst, np.abs(P[row].T - Pe).max())
            np.testing.assert_allclose(P[row].T, Pe, rtol=1e-12, atol=1e-12, err_msg="P of row %d" % row)
            np.testing.assert_allclose(b[row], be, rtol=1e-12, atol=1e-12, err_msg="b of row %d" % row)
            xe = RR.sample_row(Pe, be, O.normals(SEED, 3, 1, 11, row, D))
            np.testing.assert_allclose(out[row], xe, rtol=1e-8, atol=1e-9, err_msg="sample of row %d" % row)
        np.testing.assert_allclose(P[2], Lam, rtol=1e-12, atol=1e-12)          # the row without observations: the prior alone
    disp, runs = c2.rows_dispatch(11), 2 if n_modes == 2 else 1                         # (the launches of one iteration number add up)
    assert disp["k1"] == runs * N and disp["k1_items"] > runs * N and c2.rows_unfinished() == 0, disp      # K1 alone, the long row in pieces
    print(f"weighted row system D={D} modes={n_modes}: max |P_dev - P_numpy| = {worst:.3e}, largest |P| = {np.abs(P).max():.1f}")
    dr.close()
    c2.close()


def _weights(rng, n):
    """log-uniform on 1e-3 .. 1e3 with both ends present"""
    w = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), n))
    w[0], w[1] = 1e-3, 1e3
    return w


def _prior(rng, D):
    A = rng.standard_normal((D, D))
    return A @ A.T / D + np.eye(D), rng.standard_normal(D)


def _check_rows(O, c2, D, N, terms, system_of, mu, Lam, tag, sweep, what):
    """bdf_row_system at rtol = atol = 1e-12 and bdf_sample_rows at rtol 1e-8 / atol 1e-9 (test_weighted_row_system_and_draw's
    bounds) against system_of(row) -> (P, b) in numpy; the launch went whole to K1.  Returns the sampled rows."""
    from bdf_amd._lib import check, lib
    mu_t, Lam_t = c2.tensor(mu), c2.tensor(Lam)
    P_t, b_t, out_t = c2.zeros(N, D, D), c2.zeros(N, D), c2.tensor(np.full((N, D), np.nan))
    check(lib().bdf_row_system(c2.handle, D, N, len(terms), terms, _p(mu_t), 0, _p(Lam_t), _p(P_t), _p(b_t)))
    c2.set_sweep(sweep)
    check(lib().bdf_sample_rows(c2.handle, D, N, len(terms), terms, _p(mu_t), 0, _p(Lam_t), tag, 0, 1, _p(out_t), None))
    c2.sync()
    P, b, out = P_t.cpu().numpy(), b_t.cpu().numpy(), out_t.cpu().numpy()
    worst = 0.0
    for row in range(N):
        Pe, be = system_of(row)
        worst = max(worst, np.abs(P[row].T - Pe).max())
        np.testing.assert_allclose(P[row].T, Pe, rtol=1e-12, atol=1e-12, err_msg="P of row %d" % row)
        np.testing.assert_allclose(b[row], be, rtol=1e-12, atol=1e-12, err_msg="b of row %d" % row)
        xe = RR.sample_row(Pe, be, O.normals(SEED, sweep, 1, tag, row, D))
        np.testing.assert_allclose(out[row], xe, rtol=1e-8, atol=1e-9, err_msg="sample of row %d" % row)
    disp = c2.rows_dispatch(tag)
    assert disp["k1"] == N and disp["lowrank"] == disp["small"] == disp["col"] == 0 and c2.rows_unfinished() == 0, disp
    print(f"{what}: max |P_dev - P_numpy| = {worst:.3e}, largest |P| = {np.abs(P).max():.1f}, dispatch {disp}")
    return out, disp


TRIP_COUNTS = (0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 24, 25, 300)


@pytest.mark.parametrize("n_modes", [2, 3, 4])
@pytest.mark.parametrize("D", [16, 64])
def test_weighted_rows_on_the_trip_boundaries(B, O, D, n_modes):
    """row r has exactly TRIP_COUNTS[r] observations.  accumulate_reg's software pipeline takes 4 KS observations per trip and loads
    ids, residuals and sqrt(omega) two trips ahead: KS = 2 for one and for two other modes (trips of 8: no trip, a partial one,
    one short of / exactly / one past one, two and three trips), KS = 1 for three (trips of 4: the same around 1, 2, 4 and 6
    trips).  Item size 64: the row of 300 is cut into pieces, the last one partial."""
    rng = np.random.default_rng(700 + 10 * D + n_modes)
    N = len(TRIP_COUNTS)
    dims = [N, 23, 11, 7][:n_modes]
    rows = rng.permutation(np.repeat(np.arange(1, N + 1), TRIP_COUNTS))
    n = len(rows)
    ids = np.stack([rows] + [rng.integers(1, d + 1, n) for d in dims[1:]], axis=1).astype(np.int64)
    assert tuple(np.bincount(ids[:, 0] - 1, minlength=N)) == TRIP_COUNTS
    vals, w = rng.standard_normal(n), _weights(rng, n)
    facs = [0.3 * rng.standard_normal((d, D)) for d in dims]
    Lam, mu = _prior(rng, D)
    c2 = B.Context(seed=SEED)
    c2.set_item_size(64)
    dr = B.DeviceRelation(c2, B.IndexedDF((ids, vals), dims))
    ft = [None] + [c2.tensor(f) for f in facs[1:]]
    wt = c2.tensor(w)
    terms = _term(dr, 0, 1.7, 0.25, ft, weights=wt)
    out, disp = _check_rows(O, c2, D, N, terms, lambda row: RR.row_system(ids, vals, w, 0, row, 1.7, 0.25, facs, mu, Lam), mu, Lam, 12, 5,
                            f"trip boundaries D={D} modes={n_modes}")
    assert disp["k1_items"] > N, disp                                 # the row of 300 in pieces
    dr.close()
    c2.close()


@pytest.mark.parametrize("n_modes", [2, 3])
@pytest.mark.parametrize("D", [10, 64])
def test_weights_together_with_linear_values(B, O, D, n_modes):
    """one term that carries obs_precision and linear_values, a baseline per observation drawn N(0, 1): what every Polya-Gamma
    iteration launches"""
    rng = np.random.default_rng(800 + 10 * D + n_modes)
    dims, ids, vals, w, facs, Lam = _system_problem(rng, n_modes, D)
    base, mu = rng.standard_normal(len(vals)), rng.standard_normal(D)
    c2 = B.Context(seed=SEED)
    c2.set_item_size(64)
    dr = B.DeviceRelation(c2, B.IndexedDF((ids, vals), dims))
    ft = [None] + [c2.tensor(f) for f in facs[1:]]
    lin_t, wt = c2.tensor(base), c2.tensor(w)
    terms = _term(dr, 0, 1.7, 123.0, ft, lin=lin_t, weights=wt)                             # (with linear_values the mean is a decoy)
    _check_rows(O, c2, D, dims[0], terms, lambda row: RR.row_system(ids, vals, w, 0, row, 1.7, base, facs, mu, Lam), mu, Lam, 13, 6,
                f"weights and linear_values D={D} modes={n_modes}")
    dr.close()
    c2.close()


@pytest.mark.parametrize("D", [12, 64])
def test_launches_that_mix_a_weighted_and_an_unweighted_relation(B, O, D):
    """the sampled entity shares a three-mode relation A and a two-mode relation B (test_rows_tensor_multi_relation_mu_matrix_linear's
    shapes): (i) A weighted, B unweighted with linear_values; (ii) A unweighted, B weighted and with linear_values -- launch_kind
    sends the whole launch to k_rows_w, where the term without weights takes s = 1 -- against the sum of the two terms' numpy
    systems.  Then (i) with unit weights: bit for bit the two-term launch without weights on the general gather (A forced onto it
    by linear_values = its mean)."""
    from bdf_amd._lib import check, lib
    rng = np.random.default_rng(950 + D)
    N = 23
    dimsA, dimsB, nA, nB = [N, 9, 6], [N, 14], 700, 300
    idsA = np.stack([rng.integers(1, d + 1, nA) for d in dimsA], axis=1).astype(np.int64)
    idsB = np.stack([rng.integers(1, d + 1, nB) for d in dimsB], axis=1).astype(np.int64)
    idsA[idsA[:, 0] == 2, 0] = 1
    idsB[idsB[:, 0] == 2, 0] = 1                                      # row 2: no observation in either relation
    idsB[idsB[:, 0] == 5, 0] = 4                                      # row 5: observations in A alone
    valsA, valsB = rng.standard_normal(nA), rng.standard_normal(nB)
    SA = [0.3 * rng.standard_normal((d, D)) for d in dimsA]
    SB = [SA[0], 0.3 * rng.standard_normal((dimsB[1], D))]
    wA, wB, linB = _weights(rng, nA), _weights(rng, nB), rng.standard_normal(nB)
    Lam, mu = _prior(rng, D)
    aA, mA, aB, mB = 2.0, 0.1, 0.7, -0.3
    c2 = B.Context(seed=SEED)
    c2.set_item_size(64)
    drA, drB = B.DeviceRelation(c2, B.IndexedDF((idsA, valsA), dimsA)), B.DeviceRelation(c2, B.IndexedDF((idsB, valsB), dimsB))
    fA, fB = [None, c2.tensor(SA[1]), c2.tensor(SA[2])], [None, c2.tensor(SB[1])]
    lin_t = c2.tensor(linB)
    for tag, (omA, omB) in ((21, (wA, None)), (22, (None, wB))):
        wA_t, wB_t = (c2.tensor(om) if om is not None else None for om in (omA, omB))
        terms = _terms((drA, 0, aA, mA, fA, None, wA_t), (drB, 0, aB, mB, fB, lin_t, wB_t))
        ref = [(idsA, valsA, omA, 0, aA, mA, SA), (idsB, valsB, omB, 0, aB, linB, SB)]
        _check_rows(O, c2, D, N, terms, lambda row: RR.row_system_terms(ref, row, mu, Lam), mu, Lam, tag, 7,
                    f"mixed launch D={D} weighted={'A' if omA is not None else 'B'}")
    # unit weights on A are no weights
    mu_t, Lam_t = c2.tensor(mu), c2.tensor(Lam)
    outs = []
    for termA in ((drA, 0, aA, mA, fA, None, c2.tensor(np.ones(nA))), (drA, 0, aA, mA, fA, c2.tensor(np.full(nA, mA)), None)):
        terms = _terms(termA, (drB, 0, aB, mB, fB, lin_t, None))
        out_t = c2.tensor(np.full((N, D), np.nan))
        c2.set_sweep(8)
        check(lib().bdf_sample_rows(c2.handle, D, N, 2, terms, _p(mu_t), 0, _p(Lam_t), 23, 0, 1, _p(out_t), None))
        c2.sync()
        outs.append(out_t.cpu().numpy())
    disp = c2.rows_dispatch(23)                                       # (the two launches of one iteration number add up)
    assert disp["k1"] == 2 * N and disp["lowrank"] == disp["small"] == disp["col"] == 0, disp
    assert np.all(np.isfinite(outs[0])) and np.array_equal(outs[0], outs[1])
    drA.close(); drB.close()
    c2.close()


# ---- (b) unit weights are no weights ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_modes", [2, 3])
@pytest.mark.parametrize("D", [10, 32, 64])
def test_unit_weights_give_the_unweighted_general_path_bit_for_bit(B, ctx, D, n_modes):
    from bdf_amd._lib import check, lib
    rng = np.random.default_rng(900 + D + n_modes)
    dims = [57, 41, 9][:n_modes]
    n = 2500
    ids = np.stack([rng.integers(1, d + 1, n) for d in dims], axis=1).astype(np.int64)
    ids[:400, 0] = 7                                                  # a row long enough to be split at the default item size
    vals = rng.standard_normal(n)
    facs = [rng.standard_normal((d, D)) for d in dims]
    A = rng.standard_normal((D, D))
    Lam, mu = A @ A.T / D + np.eye(D), rng.standard_normal(D)
    dr = B.DeviceRelation(ctx, B.IndexedDF((ids, vals), dims))
    ft = [None] + [ctx.tensor(f) for f in facs[1:]]
    mean = 0.2
    ones, lin = ctx.tensor(np.ones(n)), ctx.tensor(np.full(n, mean))
    mu_t, Lam_t = ctx.tensor(mu), ctx.tensor(Lam)
    ctx.set_sweep(600 + 10 * D + n_modes)                             # (its own iteration number: the dispatch counts below start at 0)
    outs = []
    for terms in (_term(dr, 0, 1.3, mean, ft, weights=ones), _term(dr, 0, 1.3, mean, ft, lin=lin)):
        out_t = ctx.tensor(np.full((dims[0], D), np.nan))
        check(lib().bdf_sample_rows(ctx.handle, D, dims[0], 1, terms, _p(mu_t), 0, _p(Lam_t), 21, 0, 1, _p(out_t), None))
        ctx.sync()
        outs.append(out_t.cpu().numpy())
    disp = ctx.rows_dispatch(21)                                      # (the launches of one iteration number add up)
    assert disp["k1"] == 2 * dims[0] and disp["lowrank"] == disp["small"] == disp["col"] == 0, disp     # both whole to K1
    assert np.all(np.isfinite(outs[0])) and np.array_equal(outs[0], outs[1])
    dr.close()


# ---- (c) the draw ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sort", [False, True])
@pytest.mark.parametrize("n_modes", [2, 3])
@pytest.mark.parametrize("D", [1, 7, 10, 32, 64])
def test_robust_draw_matches_the_restatement(B, ctx, D, n_modes, sort):
    from bdf_amd._lib import check, lib
    rng = np.random.default_rng(2000 + 100 * D + 10 * n_modes + sort)
    dims = [37, 23, 11][:n_modes]
    n = 1003                                               # not a multiple of 8: the last group of lanes is partly idle
    ids = np.stack([rng.integers(1, d + 1, n) for d in dims], axis=1)
    ids[1::7] = ids[0]                                     # the same cell many times over
    y = rng.standard_normal(n)
    pairs = B.DevicePairs(ctx, ids, y)
    if sort:
        pairs.sort(n_modes - 1)
    S = [rng.standard_normal((d, D)) for d in dims]
    St = [ctx.tensor(s) for s in S]
    mean = 0.3
    e = (y - mean) - RR.udot(ids, S)
    sweep, worst, worst_s = 3, 0.0, 0.0
    for nu in (1.0, 4.0, 30.0):
        for alpha in (0.04, 5.0, 900.0):
            for through_dev in (False, True):
                sweep += 1
                tag = 1 + sweep % 3
                # through alpha_dev the scalar argument is a decoy: the device value wins
                a_arg, a_dev = (alpha, None) if not through_dev else (123.0, ctx.tensor([alpha]))
                om, om2, om3 = (ctx.tensor(np.full(n, np.nan)) for _ in range(3))
                s1, s2 = ctx.tensor([np.nan]), ctx.tensor([np.nan])
                ctx.set_sweep(sweep)
                check(lib().bdf_robust_draw(ctx.handle, pairs.handle, D, _facs(St), mean, a_arg, _p(a_dev), nu, tag, _p(om), _p(s1)))
                check(lib().bdf_robust_draw(ctx.handle, pairs.handle, D, _facs(St), mean, a_arg, _p(a_dev), nu, tag, _p(om2), _p(s2)))
                check(lib().bdf_robust_draw(ctx.handle, pairs.handle, D, _facs(St), mean, a_arg, _p(a_dev), nu, tag, _p(om3), None))
                ctx.sync()
                om, om2, om3, s1, s2 = om.cpu().numpy(), om2.cpu().numpy(), om3.cpu().numpy(), float(s1.item()), float(s2.item())
                ref, ref_s = RR.omegas(SEED, sweep, tag, e, alpha, nu)
                assert np.all(np.isfinite(om)) and np.all(om > 0)
                err = np.abs(om / ref - 1.0).max()
                worst, worst_s = max(worst, err), max(worst_s, abs(s1 / ref_s - 1.0))
                assert err <= 1e-9, (nu, alpha, through_dev, err)
                assert abs(s1 - ref_s) <= 1e-9 * ref_s, (nu, alpha, through_dev, s1, ref_s)
                assert s1 == s2 and np.array_equal(om, om2) and np.array_equal(om, om3)      # a fixed order; wsse_out is optional
    # known weights: the same sum without the draw
    w = np.exp(rng.uniform(-3.0, 3.0, n))
    s = ctx.tensor([np.nan])
    check(lib().bdf_pairs_weighted_sse(ctx.handle, pairs.handle, D, _facs(St), mean, _p(ctx.tensor(w)), _p(s)))
    ctx.sync()
    assert abs(float(s.item()) - np.sum(w * e * e)) <= 1e-9 * np.sum(w * e * e)
    print(f"robust draw D={D} modes={n_modes} sort={sort}: max rel. error of omega {worst:.3e}, of sum omega e^2 {worst_s:.3e} over 18 draws")
    pairs.close()


# ---- (d) whole iterations ---------------------------------------------------------------------------------------------------
CASES = [("robust", n_modes, with_feat, alpha_sample) for n_modes in (2, 3) for with_feat in (0, 1) for alpha_sample in (0, 1)] + \
        [("weights", 2, 0, alpha_sample) for alpha_sample in (0, 1)]
NU = 4.0

CHILD = textwrap.dedent('''
    import sys
    import numpy as np
    sys.path.insert(0, %r); sys.path.insert(0, %r)
    import bdf_amd as B
    import robust_restatement as RR
    out, d = sys.argv[1], {}
    cases = [("robust", m, f, a) for m in (2, 3) for f in (0, 1) for a in (0, 1)] + [("weights", 2, 0, a) for a in (0, 1)]
    for kind, n_modes, with_feat, alpha_sample in cases:
        ids, y, dims, D, feats, n_test, alpha, _, weights = RR.iteration_case(n_modes, with_feat, alpha_sample)
        names = ["a", "b", "c"][:n_modes]
        ents = [B.Entity(nm, F=feats[k]) for k, nm in enumerate(names)]
        table = {nm: ids[:, k] for k, nm in enumerate(names)}
        table["y"] = y
        rel = B.Relation(table, "rob", ents, alpha=alpha, dims=list(dims))
        rel.model.alpha_sample = bool(alpha_sample)
        B.assignToTest(rel, np.arange(1, n_test + 1))
        if kind == "robust":
            B.setRobust(rel, %r)
        else:
            B.setWeights(rel, weights)
        rd = B.RelationData(rel)
        res = B.macau(rd, num_latent=D, burnin=1, psamples=1, verbose=False, seed=91)
        key = "%%s%%d%%d%%d_" %% (kind, n_modes, with_feat, alpha_sample)
        d[key + "native"], d[key + "pred"] = np.array(int(rd._engine.native)), res["predictions"]["pred"].to_numpy()
        d[key + "mean"], d[key + "alpha"] = np.array(rel.model.mean_value), np.array(rel.model.alpha)
        d[key + "k1"] = np.array([rd._engine.rows_dispatch(j)["k1"] for j in range(n_modes)])
        if kind == "robust":
            d[key + "omega"] = res["robust"]["weights"]
        else:
            assert "robust" not in res
        for k, en in enumerate(rd.entities):
            d[key + "S%%d" %% k], d[key + "mu%%d" %% k], d[key + "Lam%%d" %% k] = en.model.sample.T, en.model.mu, en.model.Lambda
            if feats[k] is not None:
                d[key + "beta%%d" %% k], d[key + "lb%%d" %% k] = en.model.beta, np.array(en.lambda_beta)
        rd._engine.close()
    np.savez(out, **d)
''') % (ROOT, os.path.join(ROOT, "tests"), NU)


@pytest.fixture(scope="module")
def chains():
    """two iterations of every case of CASES on the native and on the step-by-step path: one child process per path"""
    return child(CHILD, no_native=False), child(CHILD, no_native=True)


@pytest.mark.parametrize("kind,n_modes,with_feat,alpha_sample", CASES)
def test_whole_iterations_match_the_restated_chain_on_both_paths(chains, kind, n_modes, with_feat, alpha_sample):
    ids, y, dims, D, feats, n_test, alpha, _, weights = RR.iteration_case(n_modes, with_feat, alpha_sample)
    key = "%s%d%d%d_" % (kind, n_modes, with_feat, alpha_sample)
    nat, step = ({k[len(key):]: v for k, v in ch.items() if k.startswith(key)} for ch in chains)
    assert nat["native"] == 1 and step["native"] == 0
    assert sorted(nat) == sorted(step) and len(nat) >= 5 + 3 * n_modes
    for k in nat:
        if k != "native":
            assert np.array_equal(nat[k], step[k]), k       # the two paths enqueue the same launches: the same bits
    assert np.array_equal(nat["k1"], dims)                  # every row of every entity by the wave-per-row kernel
    how = dict(nu=NU) if kind == "robust" else dict(weights=weights)
    ref = RR.run_chain(ids[n_test:], y[n_test:], dims, D, 91, 2, alpha=alpha, alpha_sample=alpha_sample, feats=feats,
                       test_ids=ids[:n_test], burnin=1, **how)
    tol = dict(rtol=1e-6, atol=1e-6)
    assert abs(nat["mean"] - ref["mean"]) <= 1e-12
    np.testing.assert_allclose(nat["alpha"], ref["alpha"], rtol=1e-6)
    assert (nat["alpha"] != alpha) == bool(alpha_sample)
    for k in range(n_modes):
        np.testing.assert_allclose(nat["S%d" % k], ref["S"][k], err_msg="sample of entity %d" % k, **tol)
        np.testing.assert_allclose(nat["mu%d" % k], ref["mu"][k], **tol)
        np.testing.assert_allclose(nat["Lam%d" % k], ref["Lam"][k], **tol)
        if feats[k] is not None:
            np.testing.assert_allclose(nat["beta%d" % k], ref["beta"][k], rtol=1e-5, atol=1e-6, err_msg="beta of entity %d" % k)
            assert abs(nat["lb%d" % k] - ref["lb"][k]) <= 1e-5 * ref["lb"][k]
    np.testing.assert_allclose(nat["pred"], ref["pred"], **tol)
    if kind == "robust":
        np.testing.assert_allclose(nat["omega"], ref["omega_mean"], rtol=1e-6)
    # and the weights matter: the Gaussian chain on the same data is somewhere else
    gauss = RR.run_chain(ids[n_test:], y[n_test:], dims, D, 91, 2, alpha=alpha, alpha_sample=alpha_sample, feats=feats)
    assert np.abs(gauss["S"][0] - ref["S"][0]).max() > 1e-3


# ---- (e) nothing else moved --------------------------------------------------------------------------------------------------
def test_gaussian_chain_is_untouched_by_a_robust_engine_in_the_process(B):
    ids, y, extra, n_test = RR.planted(seed=5, N1=120, N2=90, n_cells=4000, n_test=500)

    def gaussian():
        rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y + 0.25 * ids[:, 0] % 3}, "g", [B.Entity("u"), B.Entity("v")], dims=[120, 90])
        B.assignToTest(rel, np.arange(4000 - n_test + 1, 4001))
        rd = B.RelationData(rel)
        res = B.macau(rd, num_latent=16, burnin=2, psamples=2, verbose=False, seed=17)
        assert "robust" not in res
        out = [en.model.sample.copy() for en in rd.entities] + [res["predictions"]["pred"].to_numpy().copy()]
        rd._engine.close()
        return out

    alone = gaussian()
    rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "p", [B.Entity("u"), B.Entity("v")], dims=[120, 90])
    B.assignToTest(rel, np.arange(4000 - n_test + 1, 4001))
    B.setRobust(rel, 4.0)
    rdr = B.RelationData(rel)
    res = B.macau(rdr, num_latent=16, burnin=1, psamples=1, verbose=False, seed=17)
    assert len(res["robust"]["weights"]) == 4000 - n_test and np.all(res["robust"]["weights"] > 0)
    beside = gaussian()                                     # the robust engine is alive: its relation carries omega
    assert rdr._engine.gibbs is not None or not rdr._engine.native
    for a, b in zip(alone, beside):
        assert np.array_equal(a, b)
    rdr._engine.close()


# ---- (f) planted outliers -----------------------------------------------------------------------------------------------------
def test_planted_outliers(B):
    """150 x 100, rank 3, 5,000 cells of which 1,500 are held out and scored against their clean values; noise sd 0.3 and an extra
    N(0, 5^2) on 10 % of the training cells.  D = 4, 30 + 50 iterations, alpha = 1 / 0.09 fixed, the same seed for both models.
    The restated chain on the CPU (planted seeds 0, 1, 2) gave RMSE(robust) / RMSE(Gaussian) of 0.075, 0.067
    and 0.021, all below 1/4: the bound 1/2 stands as the issue set it."""
    ids, y, extra, n_test = RR.planted()
    n = len(y)

    def run(robust):
        rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "planted", [B.Entity("u"), B.Entity("v")], alpha=1.0 / 0.09, dims=[150, 100])
        B.assignToTest(rel, np.arange(n - n_test + 1, n + 1))
        if robust:
            B.setRobust(rel, 4.0)
        rd = B.RelationData(rel)
        res = B.macau(rd, num_latent=4, burnin=30, psamples=50, verbose=False, seed=1)
        pred = res["predictions"]["pred"].to_numpy()
        rd._engine.close()
        assert abs(res["RMSE"] - np.sqrt(np.mean((y[-n_test:] - pred) ** 2))) <= 1e-9
        return float(res["RMSE"]), res.get("robust")

    rmse_r, rob = run(True)
    rmse_g, none = run(False)
    w, ex = rob["weights"], extra[:n - n_test]
    out, clean = w[np.abs(ex) > 3.0].mean(), w[ex == 0.0].mean()
    print(f"planted outliers: RMSE robust {rmse_r:.4f}, Gaussian {rmse_g:.4f}, ratio {rmse_r / rmse_g:.3f}; "
          f"mean posterior weight: outliers beyond 3 {out:.4f}, clean cells {clean:.4f}")
    assert none is None and rob["nu"] == 4.0 and len(w) == n - n_test
    assert rmse_r <= 0.5 * rmse_g, (rmse_r, rmse_g)
    assert out < clean / 3.0, (out, clean)


# ---- (g) errors through the C ABI ---------------------------------------------------------------------------------------------
def test_robust_c_abi_errors(B, ctx):
    import torch
    from bdf_amd._lib import GibbsRelation, check, lib
    ids, y, extra, n_test = RR.planted(seed=9, N1=60, N2=50, n_cells=1500, n_test=0)
    rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "e", [B.Entity("u"), B.Entity("v")], dims=[60, 50])
    eng = B.GibbsEngine(B.RelationData(rel), 8, seed=3)
    assert eng.native
    n = len(y)
    train = B.DevicePairs(eng.ctx, ids, y)
    op = B.FeatOperator(eng.ctx, np.ones((n, 2)))
    lin, beta, alpha = eng.ctx.tensor(np.full(n, rel.model.mean_value)), eng.ctx.zeros(2), eng.ctx.tensor([1.0])
    om = eng.ctx.tensor(np.ones(n))
    flags = eng.ctx.tensor(np.zeros(n, dtype=np.int8), dtype=torch.int8)
    bounds = eng.ctx.tensor(np.stack([y, y], axis=1))

    def record(**kw):
        arr = (GibbsRelation * 1)()
        g = arr[0]
        g.rel, g.mean_value, g.alpha_dev, g.rel_tag, g.nnz = eng.rel[0].handle, rel.model.mean_value, alpha.data_ptr(), 1, n
        g.entity_of_mode[0], g.entity_of_mode[1] = 0, 1
        g.train, g.first_obs, g.obs_block, g.robust_nu, g.obs_precision = train.handle, 0, n, 4.0, om.data_ptr()
        for k, v in kw.items():
            setattr(g, k, v)
        return arr

    def register(arr):
        check(lib().bdf_gibbs_set_relations(eng.gibbs, 1, C.cast(arr, C.c_void_p)))

    for bad in (dict(probit=1, linear=lin.data_ptr()), dict(censor=flags.data_ptr(), linear=lin.data_ptr()),
                dict(interval=bounds.data_ptr(), linear=lin.data_ptr()), dict(feat=op.handle, beta=beta.data_ptr(), linear=lin.data_ptr())):
        with pytest.raises(B.ArgumentError, match="observation weights"):
            register(record(**bad))
        with pytest.raises(B.ArgumentError, match="observation weights"):
            register(record(robust_nu=0.0, **bad))           # known weights are refused alike
    for nu in (0.5, -1.0, float("nan"), float("inf")):
        with pytest.raises(B.ArgumentError, match="robust_nu"):
            register(record(robust_nu=nu))
    with pytest.raises(B.ArgumentError, match="robust"):
        register(record(obs_precision=None))
    with pytest.raises(B.ArgumentError, match="robust"):
        register(record(train=None))
    facs = _facs(eng.factors_of(rel))
    s = eng.ctx.zeros(1)

    def draw(train_h=train.handle, D=8, fp=facs, a=1.0, a_dev=None, nu=4.0, out=om):
        check(lib().bdf_robust_draw(eng.ctx.handle, train_h, D, fp, 0.0, a, _p(a_dev), nu, 1, _p(out), None))

    for bad in (dict(train_h=None), dict(fp=None), dict(out=None), dict(D=0), dict(D=65), dict(a=0.0), dict(a=-1.0), dict(a=float("nan")),
                dict(a=float("inf")), dict(nu=0.999), dict(nu=0.0), dict(nu=-3.0), dict(nu=float("nan")), dict(nu=float("inf"))):
        with pytest.raises(B.ArgumentError, match="bdf_robust_draw"):
            draw(**bad)
    for bad in (dict(p=None), dict(fp=None), dict(w=None), dict(o=None), dict(D=0)):
        kw = dict(p=train.handle, D=8, fp=facs, w=om, o=s)
        kw.update(bad)
        with pytest.raises(B.ArgumentError, match="bdf_pairs_weighted_sse"):
            check(lib().bdf_pairs_weighted_sse(eng.ctx.handle, kw["p"], kw["D"], kw["fp"], 0.0, _p(kw["w"]), _p(kw["o"])))
    draw(a=0.0, a_dev=alpha)                                 # alpha_dev wins over the scalar
    register(record(alpha_sample=1, alpha_lambda0=1.0, alpha_nu0=2.0))      # and the well-formed record is accepted: one iteration runs
    eng.sweep(1)
    eng.sync()
    assert np.all(np.isfinite(rel.entities[0].model.sample))
    w = om.cpu().numpy()
    assert np.all(np.isfinite(w)) and np.all(w > 0) and w.std() > 0 and float(alpha.item()) != 1.0
    op.close()
    train.close()
    eng.close()
