"""The robust (Student-t) noise model and observation weights on the host (no GPU): setRobust / setWeights and what they guard,
the stream purposes in include/bdf.h, the restated gamma variates of tests/robust_restatement.py against the oracle's Philox and
against the law they must follow, the weighted row system against the system with repeated rows, and the resource listings the
build leaves for the new kernels."""
import os
import re

import numpy as np
import pytest

import robust_restatement as RR
from test_probit_host import _resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _relation(B, n=40, test=None, alpha=2.0, names=("u", "v"), dims=(8, 6)):
    rng = np.random.default_rng(3)
    table = {nm: rng.integers(1, d + 1, n) for nm, d in zip(names, dims)}
    table["y"] = rng.standard_normal(n)
    rel = B.Relation(table, "ratings", [B.Entity(nm) for nm in names], alpha=alpha, dims=list(dims))
    if test is not None:
        B.assignToTest(rel, test)
    return rel


def _weights(n, seed=5):
    return np.exp(np.random.default_rng(seed).uniform(-3.0, 3.0, n))


# ---- setRobust / setWeights -------------------------------------------------------------------------------------------------
def test_default_has_neither(B):
    m = _relation(B).model
    assert m.robust is None and m.weights is None and B.RelationModel().robust is None and B.RelationModel().weights is None


def test_setrobust_stores_nu_and_resets_the_device_state(B):
    rel = _relation(B, test=np.arange(1, 11))
    rel._dev = object()
    assert B.setRobust(rel) is None
    assert rel.model.robust == {"nu": 4.0} and rel._dev is None
    assert rel.model.alpha == 2.0 and rel.model.alpha_sample is False
    B.setRobust(rel, nu=1)
    assert rel.model.robust == {"nu": 1.0}
    B.setRobust(rel, 30.5)
    assert rel.model.robust == {"nu": 30.5}
    B.setPrecision(rel, 3.0)                                       # the precision stays a parameter, fixed or sampled
    rel.model.alpha_sample = True
    assert rel.model.alpha == 3.0 and rel.model.robust is not None


@pytest.mark.parametrize("bad", [0.999, 0, -4.0, float("nan"), float("inf"), "4", None, True])
def test_setrobust_refuses_nu_below_one_or_not_finite(B, bad):
    rel = _relation(B)
    with pytest.raises(B.ArgumentError, match="nu"):
        B.setRobust(rel, bad)
    assert rel.model.robust is None


def test_setweights_stores_float64_weights(B):
    rel = _relation(B, test=np.arange(1, 11))
    rel._dev = object()
    w = _weights(30)
    assert B.setWeights(rel, w) is None
    assert rel.model.weights.dtype == np.float64 and np.array_equal(rel.model.weights, w) and rel._dev is None
    B.setWeights(rel, [2] * 30)                                    # a list of integers works; the weights are replaced
    assert np.all(rel.model.weights == 2.0)


def test_setweights_refuses_a_wrong_length_and_bad_values(B):
    rel = _relation(B, test=np.arange(1, 11))
    good = _weights(30)
    bads = [_weights(40), _weights(29), np.ones((30, 1)), ["a"] * 30]
    for v in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        w = good.copy()
        w[7] = v
        bads.append(w)
    for bad in bads:
        with pytest.raises(B.ArgumentError):
            B.setWeights(rel, bad)
    assert rel.model.weights is None


def test_weights_come_after_the_test_split(B):
    rel = _relation(B)
    B.setWeights(rel, _weights(40))
    with pytest.raises(B.ArgumentError, match="assignToTest before setWeights"):
        B.assignToTest(rel, np.arange(1, 11))
    assert rel.data.nnz() == 40 and len(rel.test_vec) == 0
    B.setTest(rel, {"u": [1, 2, 3], "v": [1, 1, 2], "y": [0.1, 1.0, -1.0]})     # setTest leaves the training rows alone
    assert len(rel.model.weights) == 40
    rel2 = _relation(B)
    B.setRobust(rel2)                                              # nu is not per row: the split may follow
    B.assignToTest(rel2, np.arange(1, 11))
    assert rel2.model.robust == {"nu": 4.0}


SETTERS = {"robust": lambda B, rel: B.setRobust(rel, 4.0), "weights": lambda B, rel: B.setWeights(rel, _weights(rel.data.nnz()))}


@pytest.mark.parametrize("which", ["robust", "weights"])
def test_exclusions_in_both_orders(B, which):
    mine = SETTERS[which]
    other = SETTERS["weights" if which == "robust" else "robust"]
    # each other
    rel = _relation(B)
    other(B, rel)
    with pytest.raises(B.ArgumentError, match="setRobust|setWeights"):
        mine(B, rel)
    # relation features
    rel = _relation(B)
    rel.F = np.ones((40, 2))
    with pytest.raises(B.ArgumentError, match="features"):
        mine(B, rel)
    # censored, interval, binned, ordinal, WAIC: refused whichever comes first
    def fresh(kind):
        if kind != "ordinal":
            return _relation(B)
        r = _relation(B)
        r.data.values[:] = np.arange(40) % 5 + 1
        return r

    theirs = {
        "censored": lambda r: B.setCensored(r, np.zeros(40, dtype=int)),
        "interval": lambda r: B.setInterval(r, r.data.values - 1.0, r.data.values + 1.0),
        "binned": lambda r: B.setBinned(r, [-1.0, 0.0, 1.0]),
        "ordinal": lambda r: B.setOrdinal(r),
        "waic": lambda r: B.setWaic(r),
    }
    for kind, setter in theirs.items():
        r = fresh(kind)
        setter(r)
        with pytest.raises(B.ArgumentError):
            mine(B, r)
        assert r.model.robust is None and r.model.weights is None, kind
        r = fresh(kind)
        mine(B, r)
        with pytest.raises(B.ArgumentError):
            setter(r)
        assert r.model.censor is None and r.model.interval is None and r.model.ordinal is None and r.model.waic is None, kind
    # probit
    vals = (np.arange(40) % 2).astype(np.float64)
    ids = np.stack([np.arange(40) % 8 + 1, np.arange(40) % 6 + 1], axis=1)

    def binary():
        return B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": vals}, "bin", [B.Entity("u"), B.Entity("v")], dims=[8, 6])

    r = binary()
    B.setProbit(r)
    with pytest.raises(B.ArgumentError, match="probit"):
        mine(B, r)
    r = binary()
    mine(B, r)
    with pytest.raises(B.ArgumentError):
        B.setProbit(r)
    assert r.model.probit is False


@pytest.mark.parametrize("which", ["robust", "weights"])
def test_samplers_refuse_what_the_model_does_not_cover(B, which):
    rel = _relation(B, test=np.arange(1, 6))
    SETTERS[which](B, rel)
    rd = B.RelationData(rel)
    with pytest.raises(B.ArgumentError):
        B.bpmf_vb(rd, num_latent=4, verbose=False, niter=1)
    with pytest.raises(B.ArgumentError):
        B.macau_hmc(rd, num_latent=4, verbose=False, burnin=1, psamples=1)
    with pytest.raises(B.ArgumentError, match="one rank"):
        B.GibbsEngine(rd, 4, shard=(0, 2))
    with pytest.raises(B.ArgumentError, match="lpd"):
        B.macau(rd, num_latent=4, burnin=1, psamples=1, verbose=False, lpd=True)
    # changed behind the setter's back: the engine looks again (check_robust)
    from bdf_amd.relation_data import check_robust
    rel.model.waic = {"pointwise": False}
    with pytest.raises(B.ArgumentError, match="WAIC"):
        B.GibbsEngine(rd, 4)
    rel.model.waic = None
    rel.F = np.ones((35, 2))
    with pytest.raises(B.ArgumentError, match="features"):
        B.GibbsEngine(rd, 4)
    rel.F = None
    if which == "robust":
        rel.model.robust = {"nu": 0.5}
        with pytest.raises(B.ArgumentError, match="nu"):
            check_robust(rel)
        rel.model.robust = {"nu": 4.0}
        rel.model.weights = _weights(35)
        with pytest.raises(B.ArgumentError):
            check_robust(rel)
        rel.model.weights = None
    else:
        keep = rel.model.weights
        rel.model.weights = keep[:-1]
        with pytest.raises(B.ArgumentError):
            B.GibbsEngine(rd, 4)
        rel.model.weights = -keep
        with pytest.raises(B.ArgumentError):
            check_robust(rel)
        rel.model.weights = keep
    check_robust(rel)


def test_tostr_names_the_model_and_leaves_the_others_alone(B):
    rel = _relation(B, alpha=2.0)
    assert B.toStr(rel) == "rati[α=2.0]"
    B.setRobust(rel, 4)
    assert B.toStr(rel) == "rati[α=2.0 t:4]"
    rel = _relation(B, alpha=2.0)
    B.setWeights(rel, _weights(40))
    assert B.toStr(rel) == "rati[α=2.0 wts]"


# ---- the streams ------------------------------------------------------------------------------------------------------------
def test_stream_purposes_are_defined_and_unused_by_others():
    h = open(os.path.join(ROOT, "include", "bdf.h")).read()
    purposes = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (BDF_P_[A-Z0-9_]+)\s+(\d+)", h)}
    assert purposes["BDF_P_ROBUST_N"] == 16 and purposes["BDF_P_ROBUST_U"] == 17
    assert len(set(purposes.values())) == len(purposes)           # no two purposes share a number
    from bdf_amd import _lib
    assert (_lib.P_ROBUST_N, _lib.P_ROBUST_U) == (RR.P_ROBUST_N, RR.P_ROBUST_U) == (16, 17)


def test_vectorised_gamma_is_marsaglia_tsang_on_the_oracles_streams(O):
    """gamma_mt draws one variate at a time from oracle.draw and oracle.normals; gamma_variates must be the same numbers"""
    for seed, sweep, tag, a in ((1234, 3, 1, 1.0), (91, 1, 2, 2.5), (2 ** 40 + 7, 77, 3, 15.5)):
        rows = np.array([0, 1, 2, 5, 17, 1002, 2 ** 33 + 5])
        got = RR.gamma_variates(seed, sweep, tag, rows, a)
        want = np.array([RR.gamma_mt(seed, sweep, tag, int(r), a) for r in rows])
        np.testing.assert_allclose(got, want, rtol=1e-13)
    # and not sample_alpha's stream: the oracle's gamma at variate 0 of the same entity is another number
    assert abs(O.gamma(1234, 3, 0x800000 | 1, 0, 2.5) - RR.gamma_mt(1234, 3, 1, 0, 2.5)) > 1e-6


@pytest.mark.parametrize("nu,alpha,e", [(1.0, 5.0, 0.3), (4.0, 0.04, -2.0), (4.0, 900.0, 0.1), (30.0, 5.0, 1.5)])
def test_omega_has_the_right_law(nu, alpha, e):
    """omega | e ~ Gamma((nu + 1) / 2, rate (nu + alpha e^2) / 2): mean (nu + 1) / (nu + alpha e^2), variance
    2 (nu + 1) / (nu + alpha e^2)^2; one observation over 20,000 sweeps.  Bounds: 5 standard errors of the sample mean, and of
    the sample variance (whose variance is (mu4 - sigma^4) / n with the gamma's mu4 = 3 a (a + 2) / rate^4)."""
    n = 20000
    G = RR.gamma_variates(77, np.arange(1, n + 1), 2, np.full(n, 11), 0.5 * (nu + 1.0))
    w = RR.draw_omega(e, alpha, nu, G)
    a, rate = 0.5 * (nu + 1.0), 0.5 * (nu + alpha * e * e)
    mean, var = a / rate, a / rate ** 2
    assert np.all(w > 0) and np.all(np.isfinite(w))
    assert abs(w.mean() - mean) <= 5.0 * np.sqrt(var / n)
    mu4 = 3.0 * a * (a + 2.0) / rate ** 4
    assert abs(w.var(ddof=1) - var) <= 5.0 * np.sqrt((mu4 - var ** 2) / n)


# ---- the weighted row system ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_modes", [2, 3])
def test_integer_weights_are_repeated_rows(n_modes):
    rng = np.random.default_rng(11 + n_modes)
    dims, D, n = [9, 7, 5][:n_modes], 6, 120
    ids = np.stack([rng.integers(1, d + 1, n) for d in dims], axis=1)
    y = rng.standard_normal(n)
    w = rng.integers(1, 5, n)
    S = [rng.standard_normal((d, D)) for d in dims]
    A = rng.standard_normal((D, D))
    Lam, mu = A @ A.T + D * np.eye(D), rng.standard_normal(D)
    rep = np.repeat(np.arange(n), w)
    for mode in range(n_modes):
        for row in range(dims[mode]):
            P, b = RR.row_system(ids, y, w.astype(float), mode, row, 2.5, 0.1, S, mu, Lam)
            P2, b2 = RR.row_system(ids[rep], y[rep], np.ones(len(rep)), mode, row, 2.5, 0.1, S, mu, Lam)
            assert np.abs(P - P2).max() <= 1e-12 * np.abs(P2).max() and np.abs(b - b2).max() <= 1e-12 * max(np.abs(b2).max(), 1.0)
            z = rng.standard_normal(D)
            x = RR.sample_row(P, b, z)
            L = np.linalg.cholesky(np.linalg.inv(P))
            np.testing.assert_allclose(x, L @ z + np.linalg.solve(P, b), rtol=1e-9, atol=1e-12)


def test_unit_weights_are_the_oracles_rows(O):
    """with omega == 1 the numpy row sampler is the oracle's sample_rows (the reference's map) to rounding"""
    rng = np.random.default_rng(21)
    dims, D, n = [12, 9], 5, 150
    ids = np.stack([rng.integers(1, d + 1, n) for d in dims], axis=1)
    y = rng.standard_normal(n)
    S = [rng.standard_normal((d, D)) for d in dims]
    Lam, mu = 3.0 * np.eye(D), rng.standard_normal(D)
    term = O.Term(ids, y, dims, 0, 2.0, 0.2, [None, S[1]])
    want = O.sample_rows(D, dims[0], [term], mu, Lam, 5, 3, 1)
    got = RR.sample_rows(ids, y, np.ones(n), dims, 0, 2.0, 0.2, S, mu, Lam, 5, 3, 1)
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-11)


def test_unit_weight_forms_are_the_oracles_row_system(O):
    """what the GPU tests of k_rows_w take as their reference beyond one two- or three-mode term -- row_system on a four-mode
    relation, with a baseline per observation, and row_system_terms over a three-mode and a two-mode relation that share the
    entity -- against oracle.row_system with unit weights, at 1e-13 of the largest entry"""
    rng = np.random.default_rng(31)
    D = 6
    A = rng.standard_normal((D, D))
    Lam, mu = A @ A.T / D + np.eye(D), rng.standard_normal(D)

    def relation(dims, n):
        ids = np.stack([rng.integers(1, d + 1, n) for d in dims], axis=1)
        return ids, rng.standard_normal(n), [rng.standard_normal((d, D)) for d in dims]

    def close(got, want):
        for g, w in zip(got, want):
            assert np.abs(g - w).max() <= 1e-13 * max(np.abs(w).max(), 1.0)

    dims4 = [9, 7, 5, 4]
    ids4, y4, S4 = relation(dims4, 200)
    lin4 = rng.standard_normal(200)
    for mode in range(4):
        facs = [None if k == mode else S4[k] for k in range(4)]
        for lin in (None, lin4):
            term = O.Term(ids4, y4, dims4, mode, 1.7, 0.25, facs, linear_values=lin)
            for row in range(dims4[mode]):
                got = RR.row_system(ids4, y4, np.ones(200), mode, row, 1.7, 0.25 if lin is None else lin, S4, mu, Lam)
                close(got, O.row_system(D, [term], row, mu, Lam))
    dimsA, dimsB = [9, 7, 5], [9, 8]
    idsA, yA, SA = relation(dimsA, 150)
    idsB, yB, SB = relation(dimsB, 90)
    SB[0] = SA[0]
    linB = rng.standard_normal(90)
    tA = O.Term(idsA, yA, dimsA, 0, 2.0, 0.1, [None, SA[1], SA[2]])
    tB = O.Term(idsB, yB, dimsB, 0, 0.7, -0.3, [None, SB[1]], linear_values=linB)
    for wA, wB in ((None, None), (np.ones(150), None), (None, np.ones(90))):
        for row in range(9):
            got = RR.row_system_terms([(idsA, yA, wA, 0, 2.0, 0.1, SA), (idsB, yB, wB, 0, 0.7, linB, SB)], row, mu, Lam)
            close(got, O.row_system(D, [tA, tB], row, mu, Lam))
    # and the weights of one term leave the other term's part alone
    w = np.exp(rng.uniform(-3.0, 3.0, 150))
    P1, b1 = RR.row_system_terms([(idsA, yA, w, 0, 2.0, 0.1, SA), (idsB, yB, None, 0, 0.7, linB, SB)], 0, mu, Lam)
    PA, bA = RR.row_system(idsA, yA, w, 0, 0, 2.0, 0.1, SA, mu, Lam)
    PB, bB = RR.row_system(idsB, yB, np.ones(90), 0, 0, 0.7, linB, SB, np.zeros(D), np.zeros((D, D)))
    close((P1, b1), (PA + PB, bA + bB))


# ---- the build's listings ---------------------------------------------------------------------------------------------------
def test_weighted_row_kernels_use_no_scratch():
    rows = {k: v for k, v in _resources("k_sample_rows").items() if "k_rows_w" in k}
    assert sorted(rows) == sorted("8k_rows_wILi%dELb%dEEEv10SampleArgs7PlanDev" % (dp, dump) for dp in (16, 32, 64) for dump in (0, 1))
    for k, (vgprs, scratch, occupancy) in rows.items():
        assert scratch == 0 and occupancy >= 2, (k, vgprs, scratch, occupancy)
    path = os.path.join(ROOT, "bayesiandatafusion.jl_amd", "csrc", "k_sample_rows.o.res")
    name, spills = None, {}
    for line in open(path):
        m = re.search(r"remark: \s*(Function Name|VGPRs Spill|SGPRs Spill): (\S+)", line)
        if m and m.group(1) == "Function Name":
            name = m.group(2)
        elif m and name and "k_rows_w" in name:
            spills[(name, m.group(1))] = int(m.group(2))
    assert len(spills) == 12 and not any(spills.values()), spills
    assert rows["8k_rows_wILi32ELb0EEEv10SampleArgs7PlanDev"][2] >= 4 and rows["8k_rows_wILi16ELb0EEEv10SampleArgs7PlanDev"][2] >= 6


def test_robust_draw_kernels_use_no_scratch():
    res = _resources("k_robust")
    draws = {k: v for k, v in res.items() if "k_robust_draw" in k}
    sums = {k: v for k, v in res.items() if "k_weighted_sse" in k}
    assert len(draws) == 9 and len(sums) == 9 and "14k_robust_finalEiPKdPd" in res
    for k, v in {**draws, **sums}.items():
        assert v[1] == 0 and v[2] >= 2, (k, v)
    assert draws["13k_robust_drawILi2ELi4ELi1EEEvNS_10RobustArgsE"][2] >= 3      # two modes, D <= 32: the MovieLens draw
