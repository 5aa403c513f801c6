"""Background cells (setBackground) on the GPU.  The oracle is the existing code: the same data listed densely
as an N M-row relation with setWeights -- omega_k on the listed cells, c0 and the background value on the rest -- has, with the same
seed, the same row normals and the same alpha stream, so the same chain up to rounding.  The row systems of the folded call against
the dense explicit call, the fold alone against numpy, alpha's folded sum of squares against bdf_pairs_weighted_sse over the dense
listing, whole chains on both iteration paths, the lean path against k_rows_w, two invariants, and planted implicit data."""
import ctypes as C
import os
import textwrap

import numpy as np
import pytest

from both_paths import child
import background_restatement as BR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1234
# How far the dense explicit run moves from itself when its 1,073 rows are listed in a permuted order, over the chain cases below
# (max |difference| / max(1, max |value|) over samples, predictions and the alpha trace after 3 + 3 iterations): the reference's own
# rounding floor, measured on an MI355X.  The chains are held to ten times that, and to 1e-6 at most.
FLOOR = 1.0e-14            # (the 13 cases: 8.2e-16 .. 1.0e-14, the largest at D = 32 with weights and a sampled alpha; the background runs: 1.1e-15 .. 1.0e-14)
CHAIN_TOL = min(10.0 * FLOOR, 1e-6)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _facs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _term(dr, mode0, alpha, mean, fac_other, lin=None, weights=None, alpha_dev=None):
    from bdf_amd._lib import Term
    terms = (Term * 1)()
    terms[0].rel, terms[0].mode, terms[0].alpha, terms[0].mean_value = dr.handle, mode0, alpha, mean
    terms[0].linear_values = lin.data_ptr() if lin is not None else None
    terms[0].obs_precision = weights.data_ptr() if weights is not None else None
    terms[0].alpha_dev = alpha_dev.data_ptr() if alpha_dev is not None else None
    terms[0].factors[1 - mode0] = fac_other.data_ptr()
    return terms


def _fold(c2, D, N, V_t, alpha, c0, rb, mu_t, is_matrix, Lam_t, alpha_dev=None, pack=True):
    """bdf_hyper_sums of the other entity's rows, then bdf_background_prior -> (s, G, Lambda_eff, mu_eff, pack | None, alpha_rows) tensors"""
    from bdf_amd._lib import BackgroundTerm, check, lib
    s_t, G_t = c2.zeros(D), c2.zeros(D, D)
    check(lib().bdf_hyper_sums(c2.handle, D, V_t.shape[0], _p(V_t), None, _p(s_t), _p(G_t)))
    bg = (BackgroundTerm * 1)()
    bg[0].sum, bg[0].gram, bg[0].alpha, bg[0].weight, bg[0].resid = s_t.data_ptr(), G_t.data_ptr(), alpha, c0, rb
    bg[0].alpha_dev = alpha_dev.data_ptr() if alpha_dev is not None else None
    Le_t, me_t = c2.zeros(D, D), (c2.zeros(N, D) if is_matrix else c2.zeros(D))
    pk_t = c2.zeros(lib().bdf_prior_pack_doubles(D)) if (pack and not is_matrix) else None
    ar_t = c2.tensor([np.nan])
    check(lib().bdf_background_prior(c2.handle, D, N, 1, bg, _p(mu_t), int(is_matrix), _p(Lam_t), _p(Le_t), _p(me_t), _p(pk_t), _p(ar_t)))
    return s_t, G_t, Le_t, me_t, pk_t, ar_t


def _prior(rng, D):
    A = rng.standard_normal((D, D))
    return A @ A.T / D + np.eye(D)


# ---- (a) the row systems ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("D", [3, 16, 17, 32, 33, 64])
def test_row_systems_of_the_background_call_equal_the_dense_explicit_call(B, D, weights):
    """bdf_row_system of the background call -- (Lambda_eff, mu_eff) from bdf_background_prior, the listed cells folded: unit weights
    through the values y' and alpha (1 - c0) read from alpha_rows, weights through obs_precision and linear_values -- against the
    dense explicit call (every cell listed, omega_k or c0 as obs_precision), for the rows of both modes at N = 37, M = 29, a shared
    and a per-row prior mean: to 1e-12 max |P|.  ((N + M) 2^-52 with two orders of margin; no subtraction occurs, omega > c0.)"""
    from bdf_amd._lib import check, lib
    rng = np.random.default_rng(900 + D)
    N, M = 37, 29
    ids, y, w = BR.listing(N, M, weights=weights)
    alpha, c0, value = 1.7, 0.3 * float(w.min()), -0.5
    mean = BR.all_cells_mean(N, M, y, value)
    rb = value - mean
    ida, ya, wa = BR.dense_listing(N, M, ids, y, w, c0, value)
    facs = [0.5 * rng.standard_normal((N, D)), 0.5 * rng.standard_normal((M, D))]
    Lam = _prior(rng, D)
    c2 = B.Context(seed=SEED)
    ft = [c2.tensor(f) for f in facs]
    Lam_t, wa_t = c2.tensor(Lam), c2.tensor(wa)
    dense = B.DeviceRelation(c2, B.IndexedDF((ida, ya), [N, M]))
    if weights:
        prec, lin = BR.weighted_terms(y, w, mean, c0, rb)
        listed, prec_t, lin_t = B.DeviceRelation(c2, B.IndexedDF((ids, y), [N, M])), c2.tensor(prec), c2.tensor(lin)
    else:
        listed, prec_t, lin_t = B.DeviceRelation(c2, B.IndexedDF((ids, BR.unit_values(y, mean, c0, rb)), [N, M])), None, None
    worst = 0.0
    for mode0 in (0, 1):
        n = (N, M)[mode0]
        for is_matrix in (False, True):
            mu = rng.standard_normal((n, D)) if is_matrix else rng.standard_normal(D)
            mu_t = c2.tensor(mu)
            _, _, Le_t, me_t, _, ar_t = _fold(c2, D, n, ft[1 - mode0], alpha, c0, rb, mu_t, is_matrix, Lam_t)
            P_t, b_t, Pd_t, bd_t = c2.zeros(n, D, D), c2.zeros(n, D), c2.zeros(n, D, D), c2.zeros(n, D)
            tb = _term(listed, mode0, alpha, mean, ft[1 - mode0], lin=lin_t, weights=prec_t, alpha_dev=None if weights else ar_t)
            check(lib().bdf_row_system(c2.handle, D, n, 1, tb, _p(me_t), int(is_matrix), _p(Le_t), _p(P_t), _p(b_t)))
            td = _term(dense, mode0, alpha, mean, ft[1 - mode0], weights=wa_t)
            check(lib().bdf_row_system(c2.handle, D, n, 1, td, _p(mu_t), int(is_matrix), _p(Lam_t), _p(Pd_t), _p(bd_t)))
            c2.sync()
            P, b, Pd, bd = (t.cpu().numpy() for t in (P_t, b_t, Pd_t, bd_t))
            scale = np.abs(Pd).max()
            eP, eb = np.abs(P - Pd).max() / scale, np.abs(b - bd).max() / scale
            worst = max(worst, eP, eb)
            print(f"background row systems D={D} weights={weights} mode={mode0} matrix mean={is_matrix}: |dP| {eP:.2e} |db| {eb:.2e} of max |P| = {scale:.1f}")
            assert eP <= 1e-12 and eb <= 1e-12, (mode0, is_matrix, eP, eb)
            # ... and both are the numpy restatement's
            V = facs[1 - mode0]
            idm = ids if mode0 == 0 else ids[:, ::-1]
            Pn, bn = BR.systems_folded(n, idm, y, w, mean, c0, value, V, alpha, Lam, mu)
            assert np.abs(P - Pn).max() <= 1e-11 * scale and np.abs(b - bn).max() <= 1e-11 * scale
    listed.close()
    dense.close()
    c2.close()


# ---- (b) the fold alone --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [3, 16, 17, 32, 33, 64])
def test_fold_alone_against_numpy(B, D):
    """Lambda_eff, mu_eff, alpha_rows and the pack of bdf_background_prior against numpy on the device's own s and G, alpha as an
    argument and read from alpha_dev.  Lambda_eff: the same operations in the same order, 4 ulp.  mu_eff: the forward error of a
    Cholesky solve is bounded by c_D kappa_2(Lambda_eff) u with c_D of order D^2 (Higham, Accuracy and Stability, section 10.1);
    held to the tighter 8 D kappa_2 2^-52 normwise.  Its residual Lambda_eff mu_eff - rhs, which is what reaches the rows and what the
    refinement step reduces to a few rounding errors per row of Lambda_eff, to D 2^-50 of |Lambda_eff| |mu_eff|.  The pack: a row launch given it and a row launch left to derive its own (the existing
    pre-launch on (mu_eff, Lambda_eff)) write the same bits."""
    from bdf_amd._lib import check, lib
    rng = np.random.default_rng(300 + D)
    N, M, alpha, c0, rb = 37, 29, 2.5, 0.2, -0.7
    V, Lam, mu, mus = rng.standard_normal((M, D)), _prior(rng, D), rng.standard_normal(D), rng.standard_normal((N, D))
    c2 = B.Context(seed=SEED)
    V_t, Lam_t, mu_t, mus_t = c2.tensor(V), c2.tensor(Lam), c2.tensor(mu), c2.tensor(mus)
    got = {}
    for how, a_arg, a_dev in (("argument", alpha, None), ("alpha_dev", 123.0, c2.tensor([alpha]))):
        s_t, G_t, Le_t, me_t, pk_t, ar_t = _fold(c2, D, N, V_t, a_arg, c0, rb, mu_t, False, Lam_t, alpha_dev=a_dev)
        _, _, Lm_t, mm_t, _, _ = _fold(c2, D, N, V_t, a_arg, c0, rb, mus_t, True, Lam_t, alpha_dev=a_dev)
        c2.sync()
        s, G, Le, me, pk, ar, Lm, mm = (t.cpu().numpy() for t in (s_t, G_t, Le_t, me_t, pk_t, ar_t, Lm_t, mm_t))
        assert np.allclose(G, V.T @ V, rtol=1e-12, atol=1e-12) and np.allclose(s, V.sum(axis=0), rtol=1e-12, atol=1e-12)
        ref = Lam + (alpha * c0) * G
        assert np.abs(Le - ref).max() <= 4 * 2.0 ** -52 * np.abs(ref).max() and np.array_equal(Le, Lm)
        assert ar[0] == alpha * (1.0 - c0)
        kappa = np.linalg.cond(ref)
        t = (alpha * c0 * rb) * s
        for m_dev, m_in in ((me, mu), (mm, mus)):
            rhs = m_in @ Lam.T + t
            want = np.linalg.solve(ref, rhs.T).T
            err = np.abs(m_dev - want).max() / np.abs(want).max()
            res = np.abs(m_dev @ Le.T - rhs).max() / (np.abs(Le).sum(axis=1).max() * np.abs(want).max())
            print(f"fold D={D} alpha by {how} rows={m_in.ndim}: kappa {kappa:.1f}, forward error {err:.2e}, residual {res:.2e}")
            assert err <= 8 * D * kappa * 2.0 ** -52 and res <= D * 2.0 ** -50
        # the pack: Lambda_eff mu_eff, then the accumulator-layout image of the index-reversed Lambda_eff (identity on the padding)
        assert np.allclose(pk[:D], Le @ me, rtol=1e-13, atol=1e-13 * np.abs(Le @ me).max())
        DP = 16 if D <= 16 else (32 if D <= 32 else 64)
        full = np.eye(DP)
        full[:D, :D] = Le[::-1, ::-1]
        img, e = pk[D:].reshape(-1, 64), 0
        for I in range(DP // 16):
            for J in range(I + 1):
                for r in range(4):
                    lane = np.arange(64)
                    assert np.array_equal(img[e], full[16 * I + (lane >> 4) + 4 * r, 16 * J + (lane & 15)]), (I, J, r)
                    e += 1
        assert e == len(img)
        got[how] = (Le, me, pk, mm)
    for a, b in zip(got["argument"], got["alpha_dev"]):
        assert np.array_equal(a, b)
    # a row launch with the fold's pack and one that derives its own from (mu_eff, Lambda_eff)
    ids, y, _ = BR.listing(N, M)
    dr = B.DeviceRelation(c2, B.IndexedDF((ids, y), [N, M]))
    terms = _term(dr, 0, alpha, 0.3, V_t)
    c2.set_sweep(5)
    o1, o2 = c2.zeros(N, D), c2.zeros(N, D)
    check(lib().bdf_sample_rows(c2.handle, D, N, 1, terms, _p(me_t), 0, _p(Le_t), 7, 0, 1, _p(o1), _p(pk_t)))
    check(lib().bdf_sample_rows(c2.handle, D, N, 1, terms, _p(me_t), 0, _p(Le_t), 7, 0, 1, _p(o2), None))
    c2.sync()
    assert np.array_equal(o1.cpu().numpy(), o2.cpu().numpy()) and np.all(np.isfinite(o1.cpu().numpy()))
    dr.close()
    c2.close()


# ---- (c) alpha's sum of squares -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sort", [False, True])
@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("D", [3, 16, 17, 32, 33, 64])
def test_folded_sum_of_squares_equals_the_dense_sum_and_draws_the_same_alpha(B, D, weights, sort):
    """bdf_background_sse over the listed cells against bdf_pairs_weighted_sse over the dense listing, and bdf_sample_alpha with n =
    N M on each: both to 1e-12 relative; the folded sum twice: the same bits"""
    from bdf_amd._lib import check, lib
    rng = np.random.default_rng(40 + D)
    N, M = 37, 29
    ids, y, w = BR.listing(N, M, weights=weights)
    c0, value = 0.3 * float(w.min()), -0.5
    mean = BR.all_cells_mean(N, M, y, value)
    ida, ya, wa = BR.dense_listing(N, M, ids, y, w, c0, value)
    U, V = 0.5 * rng.standard_normal((N, D)), 0.5 * rng.standard_normal((M, D))
    c2 = B.Context(seed=SEED)
    ft = [c2.tensor(U), c2.tensor(V)]
    pl, pd = B.DevicePairs(c2, ids, y), B.DevicePairs(c2, ida, ya)
    if sort:
        pl.sort(1)
        pd.sort(1)
    sums = [c2.zeros(D), c2.zeros(D, D), c2.zeros(D), c2.zeros(D, D)]
    for k in (0, 1):
        check(lib().bdf_hyper_sums(c2.handle, D, ft[k].shape[0], _p(ft[k]), None, _p(sums[2 * k]), _p(sums[2 * k + 1])))
    out = c2.tensor([np.nan, np.nan, np.nan])
    w_t = c2.tensor(w) if weights else None
    for k in (0, 1):
        check(lib().bdf_background_sse(c2.handle, pl.handle, D, _facs(ft), mean, _p(w_t), value, c0, *[_p(t) for t in sums], N, M,
                                       C.c_void_p(out.data_ptr() + 8 * k)))
    check(lib().bdf_pairs_weighted_sse(c2.handle, pd.handle, D, _facs(ft), mean, _p(c2.tensor(wa)), C.c_void_p(out.data_ptr() + 16)))
    c2.set_sweep(2)
    al = c2.tensor([np.nan, np.nan])
    check(lib().bdf_sample_alpha(c2.handle, 1.0, 2.0, N * M, C.c_void_p(out.data_ptr()), 1, C.c_void_p(al.data_ptr())))
    check(lib().bdf_sample_alpha(c2.handle, 1.0, 2.0, N * M, C.c_void_p(out.data_ptr() + 16), 1, C.c_void_p(al.data_ptr() + 8)))
    c2.sync()
    s, a = out.cpu().numpy(), al.cpu().numpy()
    ref = BR.sse_dense(ids, y, w, mean, c0, value, U, V)
    print(f"background sse D={D} weights={weights} sort={sort}: folded {s[0]:.15g} dense {s[2]:.15g} rel {abs(s[0] / s[2] - 1):.2e}; alpha {a[0]:.15g} {a[1]:.15g}")
    assert s[0] == s[1]
    assert abs(s[0] - s[2]) <= 1e-12 * s[2] and abs(s[2] - ref) <= 1e-12 * ref
    assert a[0] > 0 and abs(a[0] - a[1]) <= 1e-12 * a[1]
    pl.close()
    pd.close()
    c2.close()


# ---- (d) chains ------------------------------------------------------------------------------------------------------------------------
CASES = [(D, a, w, 0) for D in (5, 32, 40) for a in (0, 1) for w in (0, 1)] + [(5, 1, 0, 1)]

CHILD = textwrap.dedent('''
    import os, sys
    import numpy as np
    sys.path.insert(0, %r); sys.path.insert(0, %r)
    import bdf_amd as B
    import background_restatement as BR
    out, d = sys.argv[1], {}
    cases = [(D, a, w, 0) for D in (5, 32, 40) for a in (0, 1) for w in (0, 1)] + [(5, 1, 0, 1)]

    def run(key, D, alpha_sample, F, ids, y, weights, background, dims):
        ents = [B.Entity("u", F=F), B.Entity("v")]
        rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "plays", ents, alpha=2.0, dims=list(dims))
        rel.model.alpha_sample = bool(alpha_sample)
        B.setTest(rel, {"u": c["test"][:, 0], "v": c["test"][:, 1], "y": c["test_y"]})
        if weights is not None:
            B.setWeights(rel, weights)
        if background is not None:
            B.setBackground(rel, *background)
        rd = B.RelationData(rel)
        res = B.macau(rd, num_latent=D, burnin=3, psamples=3, verbose=False, seed=91,
                      f=lambda data: float(data.relations[0]._dev.alpha_dev.item()))
        d[key + "native"] = np.array(int(rd._engine.native))
        d[key + "pred"], d[key + "trace"] = res["predictions"]["pred"].to_numpy(), np.array(res["f_output"])
        d[key + "mean"], d[key + "alpha"] = np.array(rel.model.mean_value), np.array(rel.model.alpha)
        for k, en in enumerate(rd.entities):
            d[key + "S%%d" %% k] = en.model.sample.T
        disp = [rd._engine.rows_dispatch(j) for j in (0, 1)]
        d[key + "col"], d[key + "k1"] = np.array([x["col"] for x in disp]), np.array([x["k1"] for x in disp])
        d[key + "bg"] = np.array(res["background"]["plays"]["cells"] if "background" in res else -1)
        rd._engine.close()

    for D, alpha_sample, weights, feat in cases:
        c = BR.chain_case(bool(weights), bool(feat))
        N, M, ids, y, w, c0, value = c["N"], c["M"], c["ids"], c["y"], c["w"], c["c0"], c["value"]
        ida, ya, wa = BR.dense_listing(N, M, ids, y, w, c0, value)
        key = "%%d%%d%%d%%d_" %% (D, alpha_sample, weights, feat)
        run(key + "bg_", D, alpha_sample, c["F"], ids, y, w if weights else None, (c0, value), (N, M))
        run(key + "dense_", D, alpha_sample, c["F"], ida, ya, wa, None, (N, M))
        if not os.environ.get("BDF_NO_NATIVE"):
            p = np.random.default_rng(3).permutation(N * M)
            run(key + "perm_", D, alpha_sample, c["F"], ida[p], ya[p], wa[p], None, (N, M))
        if not weights:
            run(key + "ones_", D, alpha_sample, c["F"], ids, y, np.ones(len(y)), (c0, value), (N, M))
    # a relation that lists every cell, with and without a background
    c = BR.chain_case(False, False)
    ida, ya, _ = BR.dense_listing(c["N"], c["M"], c["ids"], c["y"], c["w"], 0.0, 0.25)
    run("full_bg_", 5, 1, None, ida, ya, None, (0.3, 1.5), (c["N"], c["M"]))
    run("full_plain_", 5, 1, None, ida, ya, None, None, (c["N"], c["M"]))
    np.savez(out, **d)
''') % (ROOT, os.path.join(ROOT, "tests"))


@pytest.fixture(scope="module")
def chains():
    """3 + 3 iterations of every case on the native and on the step-by-step path: one child process per path"""
    return child(CHILD, no_native=False), child(CHILD, no_native=True)


def _take(ch, key):
    return {k[len(key):]: v for k, v in ch.items() if k.startswith(key)}


def _distance(a, b):
    """max |difference| / max(1, max |value|) over the samples, the test predictions and the alpha trace of two runs"""
    return max(np.abs(a[k] - b[k]).max() / max(1.0, np.abs(b[k]).max()) for k in ("S0", "S1", "pred", "trace", "alpha"))


@pytest.mark.parametrize("D,alpha_sample,weights,feat", CASES)
def test_chains_equal_the_dense_explicit_run_on_both_paths(chains, D, alpha_sample, weights, feat):
    """samples, test predictions and the alpha trace of the background run against the dense explicit run (every cell listed, with
    setWeights), 3 + 3 iterations, on both iteration paths -- which enqueue the same launches: the same bits"""
    key = "%d%d%d%d_" % (D, alpha_sample, weights, feat)
    nat, step = _take(chains[0], key), _take(chains[1], key)
    for k in nat:
        if not k.endswith("native") and not k.startswith("perm_"):
            assert np.array_equal(nat[k], step[k]), k
    bg, dense, perm = _take(nat, "bg_"), _take(nat, "dense_"), _take(nat, "perm_")
    assert bg["native"] == 1 and _take(step, "bg_")["native"] == 0
    assert bg["bg"] == 37 * 29 - len(BR.chain_case(bool(weights), False)["y"]) and dense["bg"] == -1
    assert abs(bg["mean"] - dense["mean"]) <= 1e-14
    assert (len(set(bg["trace"])) == 3) == bool(alpha_sample) and np.all(bg["trace"] > 0)
    floor, dist = _distance(perm, dense), _distance(bg, dense)
    print(f"background chain D={D} alpha_sample={alpha_sample} weights={weights} feat={feat}: permuted dense run {floor:.2e}, background run {dist:.2e}")
    assert dist <= CHAIN_TOL, (dist, floor)
    assert np.abs(bg["S0"]).max() > 0.1                     # (a chain, not zeros)


@pytest.mark.parametrize("D,alpha_sample,weights,feat", [c for c in CASES if not c[2]])
def test_unit_weights_stay_on_the_lean_path_and_equal_the_weighted_kernel(chains, D, alpha_sample, weights, feat):
    """without setWeights the listed cells go through the unweighted kernels (packed values; K1c at D = 32) with the values y' and
    alpha (1 - c0); the same run under setWeights(ones) goes through k_rows_w with omega - c0 and linear_values: the same chain"""
    nat = _take(chains[0], "%d%d%d%d_" % (D, alpha_sample, weights, feat))
    bg, ones = _take(nat, "bg_"), _take(nat, "ones_")
    dist = _distance(bg, ones)
    print(f"background lean path D={D} alpha_sample={alpha_sample} feat={feat}: against setWeights(ones) {dist:.2e}; K1c rows {bg['col']}, K1 rows {bg['k1']}")
    assert dist <= CHAIN_TOL
    assert np.array_equal(ones["k1"], [37, 29]) and np.array_equal(ones["col"], [0, 0])
    if D == 32:
        assert np.array_equal(bg["col"], [37, 29]) and np.array_equal(bg["k1"], [0, 0])      # K1c took every row of both entities


def test_a_relation_that_lists_every_cell_is_untouched_by_a_background(chains):
    for ch in chains:
        a, b = _take(ch, "full_bg_"), _take(ch, "full_plain_")
        assert a["bg"] == 0 and b["bg"] == -1
        dist = _distance(a, b)
        print(f"every cell listed, with and without setBackground(rel, 0.3): {dist:.2e}")
        assert dist <= CHAIN_TOL


# ---- (e) it learns ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_background_learns_from_where_the_ones_sit(B, seed):
    """Planted preferences p_ij = sigma(3 u.v - 1), N = 300, M = 200, rank 4 (u, v ~ N(0, I)); the listed cells all hold 1; held out
    are a fifth of the ones and as many unlisted cells.  D = 8, alpha = 10 fixed, 20 + 20 iterations.  Without a background the
    residuals are all zero and U, V follow their prior.  The numpy restatement on the CPU (tests/background_restatement.py,
    gibbs_auc) gave AUC with / without a background of 0.9442 / 0.4938, 0.9424 / 0.5039 and 0.9426 / 0.5050 for seeds 0, 1, 2."""
    train, test, tv = BR.planted(seed)

    def run(background):
        rel = B.Relation({"u": train[:, 0], "v": train[:, 1], "y": np.ones(len(train))}, "plays", [B.Entity("u"), B.Entity("v")],
                         class_cut=0.5, alpha=10.0, dims=[300, 200])
        B.setTest(rel, {"u": test[:, 0], "v": test[:, 1], "y": tv})
        if background:
            B.setBackground(rel, 0.1)
        rd = B.RelationData(rel)
        res = B.macau(rd, num_latent=8, burnin=20, psamples=20, verbose=False, seed=seed)
        pred = res["predictions"]["pred"].to_numpy()
        rd._engine.close()
        assert abs(res["ROC"] - BR.auc(tv < 0.5, -pred)) <= 1e-9
        return float(res["ROC"])

    with_bg, without = run(True), run(False)
    print(f"planted implicit data, seed {seed}: AUC with a background {with_bg:.4f}, listed cells only {without:.4f}")
    assert with_bg > without


# ---- (f) errors through the C ABI ---------------------------------------------------------------------------------------------------------
def test_background_c_abi_errors(B, ctx):
    from bdf_amd._lib import BackgroundTerm, lib
    D = 4
    z, Z, o, O2 = ctx.zeros(D), ctx.tensor(np.eye(D)), ctx.zeros(D), ctx.zeros(D, D)
    pk, ar = ctx.zeros(lib().bdf_prior_pack_doubles(D)), ctx.zeros(1)
    bg = (BackgroundTerm * 1)()
    bg[0].sum, bg[0].gram, bg[0].alpha, bg[0].weight, bg[0].resid = z.data_ptr(), Z.data_ptr(), 1.0, 0.5, 0.0

    def prior(D=D, n_bg=1, mu=z, matrix=0, Lam=Z, Lo=O2, mo=o, pack=pk):
        return lib().bdf_background_prior(ctx.handle, D, 3, n_bg, bg, _p(mu), matrix, _p(Lam), _p(Lo), _p(mo), _p(pack), _p(ar))

    assert prior() == 0
    assert prior(D=0) == -1 and prior(D=65) == -1 and prior(n_bg=0) == -1 and prior(n_bg=5) == -1
    assert prior(Lo=Z) == -1 and prior(mo=z) == -1 and prior(mu=None) == -1
    assert prior(matrix=1, mu=ctx.zeros(3, D), mo=ctx.zeros(3, D)) == -1            # per-row prior means have no pack
    assert prior(matrix=1, mu=ctx.zeros(3, D), mo=ctx.zeros(3, D), pack=None) == 0
    for field, bad in (("weight", 0.0), ("weight", 1.5), ("resid", float("nan")), ("alpha", 0.0)):
        keep = getattr(bg[0], field)
        setattr(bg[0], field, bad)
        assert prior() == -1, field
        setattr(bg[0], field, keep)
    ctx.sync()
    ids = np.array([[1, 1, 1], [2, 1, 2]], dtype=np.int64)
    p3 = B.DevicePairs(ctx, ids, np.zeros(2))
    f3 = [ctx.zeros(2, D)] * 3
    rc = lib().bdf_background_sse(ctx.handle, p3.handle, D, _facs(f3), 0.0, None, 0.0, 0.5, _p(z), _p(Z), _p(z), _p(Z), 2, 2, _p(ar))
    assert rc == -1 and b"two-mode" in lib().bdf_last_error()
    p2 = B.DevicePairs(ctx, ids[:, :2], np.zeros(2))
    assert lib().bdf_background_sse(ctx.handle, p2.handle, D, _facs(f3[:2]), 0.0, None, 0.0, 0.0, _p(z), _p(Z), _p(z), _p(Z), 2, 2, _p(ar)) == -1
    Z0 = ctx.zeros(D, D)
    assert lib().bdf_background_sse(ctx.handle, p2.handle, D, _facs(f3[:2]), 0.0, None, 0.0, 0.5, _p(z), _p(Z0), _p(z), _p(Z0), 2, 2, _p(ar)) == 0
    ctx.sync()
    assert float(ar.item()) == 0.0                           # all factors zero, values at the mean, rb = 0
    p3.close()
    p2.close()
