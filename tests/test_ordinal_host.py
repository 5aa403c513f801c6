"""The ordinal probit noise model on the host (no GPU): the maps of tests/ordinal_restatement.py (round trip, the Jacobian term
against a finite-difference determinant, its Philox numbers against the oracle's), csrc/ordinal.h compiled for the host against the
restatement, the Metropolis step's invariant law against a grid integration of the exact posterior, setOrdinal / setTestOrdinal and
what they guard, and the resource listing the build leaves for k_ordinal."""
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import ordinal_restatement as OR
from test_probit_host import _resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.inf


def _random_edges(rng, K):
    g = rng.uniform(0.05, 1.0, K - 2)
    g *= (K - 2.0) / g.sum()
    return np.concatenate([[-INF, 1.5], 1.5 + np.cumsum(g)[:-1], [K - 0.5, INF]])


# ---- the maps -------------------------------------------------------------------------------------------------------------------
def test_theta_and_gaps_round_trip():
    rng = np.random.default_rng(1)
    for K in (4, 5, 6, 11, 16):
        e = _random_edges(rng, K)
        th = OR.theta(e)
        assert th.shape == (K - 3,)
        g = OR.gaps_from_theta(th, e[K - 1] - e[1])
        assert np.abs(g - np.diff(e[1:K])).max() <= 1e-14
        out, jac, ok = OR.propose(e, 0.7, np.zeros(K - 3))           # a step of length 0 proposes the edges themselves
        assert ok and np.abs(out[1:K] - e[1:K]).max() <= 1e-14 and abs(jac) <= 1e-13
        assert out[0] == -INF and out[K] == INF and out[1] == 1.5 and out[K - 1] == K - 0.5      # the anchors are copied, not summed
        assert np.array_equal(OR.start_edges(K)[1:K], np.arange(1, K) + 0.5)


def test_jacobian_term_is_the_log_determinant_of_the_edges_in_theta():
    """The prior is uniform on the ordered interior edges; the random walk is symmetric in theta.  So the target's density in theta
    carries |det d(edges) / d(theta)|, and the acceptance ratio the ratio of two such determinants: the difference of
    sum_k log g_k over ALL K - 2 gaps.  Central differences of the map theta -> interior edges (step 1e-6) give the determinant
    to about 1e-9 relative."""
    rng = np.random.default_rng(2)
    for K in (4, 5, 7, 16):
        e = _random_edges(rng, K)
        R = e[K - 1] - e[1]

        def logdet(th):
            J = np.zeros((K - 3, K - 3))
            for j in range(K - 3):
                d = np.zeros(K - 3)
                d[j] = 1e-6
                J[:, j] = (np.cumsum(OR.gaps_from_theta(th + d, R))[:-1] - np.cumsum(OR.gaps_from_theta(th - d, R))[:-1]) / 2e-6
            return np.linalg.slogdet(J)[1]

        for sigma in (0.1, 0.9):
            eps = rng.standard_normal(K - 3)
            out, jac, ok = OR.propose(e, sigma, eps)
            assert ok
            th0, th1 = OR.theta(e), OR.theta(out)
            assert np.abs(th1 - (th0 + sigma * eps)).max() <= 1e-12          # the proposal IS the random walk in theta
            assert abs((logdet(th1) - logdet(th0)) - jac) <= 1e-7, (K, sigma)
            # a Jacobian over the K - 3 free gaps only is another number
            assert abs(jac - (np.log(np.diff(out[1:K - 1])).sum() - np.log(np.diff(e[1:K - 1])).sum())) > 1e-3


def test_gap_guard_and_step_size_rule():
    e = OR.start_edges(5)
    out, jac, ok = OR.propose(e, 10.0, np.array([-2.0, 0.0]))        # exp(-20): a first gap of 3e-9
    assert not ok and out[2] - out[1] < 1e-6
    assert OR.propose(e, 1.0, np.array([-2.0, 0.0]))[2]
    s = 0.1
    for i, acc in enumerate([True, False, False, True], start=1):
        s2 = OR.adapt(s, acc, i)
        assert abs(np.log(s2) - np.log(s) - ((1.0 if acc else 0.0) - 0.3) / np.sqrt(i)) <= 1e-15
        s = s2
    assert OR.adapt(9.9, True, 1) == 10.0 and OR.adapt(1.1e-8, False, 1) == 1e-8


def test_step_numbers_are_the_librarys_streams(O):
    """normal k of (15, 0x800000 | rel_tag, row 0) and the first double of block (15, ..., row 1, pair 0), against the oracle's
    Philox and Box-Muller"""
    for seed, sweep, tag in ((1234, 7, 1), (2 ** 40 + 5, 0xfffe0003, 3)):
        ent = 0x800000 | tag
        ref = O.normals(seed, sweep, OR.P_ORDINAL, ent, 0, 13)
        assert np.abs(OR.normals(seed, sweep, tag, 13) - ref).max() <= 1e-14
        w = O.draw(seed, sweep, OR.P_ORDINAL, ent, 1, 0)
        u = ((((int(w[1]) << 32) | int(w[0])) >> 11) + 0.5) * 2.0 ** -53
        assert OR.uniform(seed, sweep, tag) == u
    from bdf_amd import _lib
    assert _lib.P_ORDINAL == OR.P_ORDINAL == 15
    assert "#define BDF_P_ORDINAL      15" in open(os.path.join(ROOT, "include", "bdf.h")).read()


# ---- the header against the restatement -------------------------------------------------------------------------------------------
def _compile_and_run(text):
    """csrc/ordinal.h compiled for the host; lines "K sigma e_0 .. e_K eps_1 .. eps_{K-3}" -> "ok jac out_0 .. out_K", and lines
    "0 sigma accepted i" -> the adapted step size"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cxx = [shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")]
    if cxx[0] is None:
        cxx = [hipcc, "-x", "c++"]
    src = r'''
        #include <cstdio>
        #include "ordinal.h"
        int main() { int K; double s; while (scanf("%d %lf", &K, &s) == 2) {
            if (K == 0) { int a; double i; if (scanf("%d %lf", &a, &i) != 2) return 1; printf("%.17g\n", bdf_ordinal_adapt(s, a != 0, i)); continue; }
            double e[17], eps[16], out[17], jac;
            for (int k = 0; k <= K; k++) if (scanf("%lf", &e[k]) != 1) return 1;
            for (int k = 0; k < K - 3; k++) if (scanf("%lf", &eps[k]) != 1) return 1;
            const bool ok = bdf_ordinal_propose(K, e, s, eps, out, &jac);
            printf("%d %.17g", ok ? 1 : 0, jac);
            for (int k = 0; k <= K; k++) printf(" %.17g", out[k]);
            printf("\n"); } return 0; }
    '''
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "t.cpp"), "w").write(src)
        subprocess.run(cxx + ["-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "bayesiandatafusion.jl_amd", "csrc"), os.path.join(td, "t.cpp"),
                        "-o", os.path.join(td, "t")], check=True)
        return subprocess.run([os.path.join(td, "t")], input=text, capture_output=True, text=True, check=True).stdout.splitlines()


def test_header_and_restatement_state_the_same_maps():
    """600 proposals, K in 4 .. 16, gaps from even to 1 : 20, step sizes 1e-3 ... 10 (the large ones run into the gap guard), and the
    step-size rule: the same loops on two libms, 1e-12"""
    rng = np.random.default_rng(3)
    cases, lines = [], []
    for t in range(600):
        K = int(rng.integers(4, 17))
        e = _random_edges(rng, K) if t % 3 else OR.start_edges(K)
        sigma = float(10.0 ** rng.uniform(-3.0, 1.0))
        eps = rng.standard_normal(K - 3)
        cases.append((e, sigma, eps))
        lines.append(" ".join([str(K), "%.17g" % sigma] + ["%.17g" % x for x in e] + ["%.17g" % x for x in eps]).replace("inf", "INF"))
    adapts = [(float(10.0 ** rng.uniform(-8.0, 1.0)), int(rng.integers(0, 2)), float(rng.integers(1, 5000))) for _ in range(200)]
    lines += ["0 %.17g %d %.17g" % a for a in adapts]
    got = _compile_and_run("\n".join(lines) + "\n")
    assert len(got) == 800
    refused = 0
    for (e, sigma, eps), line in zip(cases, got):
        f = [float(x) for x in line.split()]
        out, jac, ok = OR.propose(e, sigma, eps)
        assert bool(f[0]) == ok
        refused += not ok
        K = len(e) - 1
        assert f[2] == -INF and f[2 + K] == INF
        assert np.abs(np.array(f[3:2 + K]) - out[1:K]).max() <= 1e-12
        if ok:
            assert abs(f[1] - jac) <= 1e-12 * max(1.0, abs(jac))
    assert 0 < refused < 300
    for (s, a, i), line in zip(adapts, got[600:]):
        assert abs(float(line) - OR.adapt(s, bool(a), i)) <= 1e-12 * OR.adapt(s, bool(a), i)


# ---- the step leaves the right law invariant ------------------------------------------------------------------------------------
def test_metropolis_step_leaves_the_exact_posterior_invariant():
    """K = 5, 200 cells with fixed means m, alpha = 4: the posterior of the two free edges (e_2, e_3) given the levels is known up to
    a constant -- the product of the cells' bin masses on 1.5 < e_2 < e_3 < 4.5 -- and is integrated on a 300 x 300 grid.  20,000
    steps of the restated kernel (step size 0.5, not adapted) must reproduce its two means within four batch-means standard errors
    (20 batches of 1,000).  Measured: 2.1519 / 3.8787 against the exact 2.1553 / 3.8794, standard errors 0.0019 / 0.0015.  The step
    without its Jacobian term gives 2.1460 / 3.8862 (5.6 and 4.1 standard errors off), with a Jacobian over the K - 3 free gaps only
    2.1535 / 3.8869 (5.7 off in the second): both sample the posterior under another prior, and both fail here."""
    rng = np.random.default_rng(4)
    n, K, alpha = 200, 5, 4.0
    m = rng.uniform(0.5, 5.5, n)
    true = np.array([-INF, 1.5, 2.2, 3.9, 4.5, INF])
    codes = np.searchsorted(true[1:K], m + 0.5 * rng.standard_normal(n), side="right") + 1
    ra = np.sqrt(alpha)
    # the grid: level 2 reads e_2 alone, level 4 e_3 alone, level 3 both
    x = np.linspace(1.5, 4.5, 302)[1:-1]
    P = lambda t: OR.LR.phi(t)                                                                    # noqa: E731
    l2 = np.log(P((x[:, None] - m[codes == 2]) * ra) - P((1.5 - m[codes == 2]) * ra)).sum(axis=1)
    l4 = np.log(P((4.5 - m[codes == 4]) * ra) - P((x[:, None] - m[codes == 4]) * ra)).sum(axis=1)
    m3 = m[codes == 3]
    with np.errstate(all="ignore"):
        l3 = np.log(np.maximum(P((x[None, :, None] - m3) * ra) - P((x[:, None, None] - m3) * ra), 1e-300)).sum(axis=2)      # [e_2, e_3]
    logp = l2[:, None] + l4[None, :] + l3
    logp[x[:, None] >= x[None, :]] = -INF
    w = np.exp(logp - logp.max())
    w /= w.sum()
    exact = np.array([(w.sum(axis=1) * x).sum(), (w.sum(axis=0) * x).sum()])
    # the chain
    st = OR.State(K, 0.5)
    draws = np.zeros((20000, 2))
    for it in range(20000):
        st.step(m, codes, alpha, 77, it + 1, 1, False)
        draws[it] = st.e[2:4]
    rate = st.accepts / st.proposals
    bm = draws.reshape(20, 1000, 2).mean(axis=1)
    se = bm.std(axis=0, ddof=1) / np.sqrt(20.0)
    print(f"invariance: exact means {exact[0]:.4f} {exact[1]:.4f}, chain {draws.mean(axis=0)[0]:.4f} {draws.mean(axis=0)[1]:.4f}, "
          f"batch-means standard errors {se[0]:.4f} {se[1]:.4f}, acceptance {rate:.2f}")
    assert 0.05 < rate < 0.95
    assert np.all(np.abs(draws.mean(axis=0) - exact) <= 4.0 * se), (draws.mean(axis=0), exact, se)


def test_gpu_test_cases_decide_both_ways_and_never_on_a_knifes_edge():
    """what tests/test_gpu_ordinal.py relies on, checked where no GPU is needed: over the 120 step-parity steps, and again over the
    32 steps of the whole-iteration cases, the restatement accepts some proposals and refuses others, and every decision's
    margin |log u - S| is at least 1e-6 -- the device's S, good to 8e-9, then decides the same way"""
    del OR.MARGINS[:]
    acc = [s["accepted"] for D in (1, 7, 10, 32, 64) for n_modes in (2, 3) for K in (4, 5, 16) for s in OR.step_sequence(D, n_modes, K)]
    assert len(acc) == 120 and len(OR.MARGINS) == 120 and any(acc) and not all(acc)
    assert min(OR.MARGINS) >= 1e-6
    for K in (4, 5, 16):
        codes = OR.step_case(10, 2, K)[3]
        assert len(codes) == 1003 and np.count_nonzero(np.bincount(codes, minlength=K + 1)[1:] == 0) >= 1      # a level nobody reported
    del OR.MARGINS[:]
    acc = np.concatenate([r["accepted"] for r in OR.restated_iterations().values()])
    assert len(acc) == 32 and len(OR.MARGINS) == 32 and acc.any() and not acc.all()
    assert min(OR.MARGINS) >= 1e-6


def test_planted_gains_are_what_the_restatement_computes():
    """the three held-out LPD gains of sampled over fixed edges that DESIGN.md section 16 prints and the GPU quality test takes its
    bound from (half the smallest), recomputed: six restated chains of 120 iterations on the planted six-level data"""
    gains = [OR.planted_gain(seed) for seed in (2, 3, 4)]
    print("planted gains: " + " ".join(f"{g:.4f}" for g in gains))
    assert np.abs(np.array(gains) - OR.PLANTED_GAINS).max() <= 5e-5
    assert min(OR.PLANTED_GAINS) == 0.1127


# ---- setOrdinal / setTestOrdinal ------------------------------------------------------------------------------------------------
def _relation(B, n=60, test=None, values=None, K=5):
    rng = np.random.default_rng(3)
    ids = np.stack([rng.integers(1, 9, n), rng.integers(1, 7, n)], axis=1)
    y = (np.arange(n) % K + 1.0) if values is None else np.asarray(values, dtype=np.float64)
    rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "ratings", [B.Entity("u"), B.Entity("v")], alpha=2.0, dims=[8, 6])
    if test is not None:
        B.assignToTest(rel, test)
    return rel


def test_setordinal_stores_codes_edges_and_the_binned_bounds(B):
    m = B.RelationModel()
    assert m.ordinal is None and m.ordinal_codes is None and m.ordinal_edges is None and m.test_ordinal is None
    rel = _relation(B, test=np.arange(1, 13))
    assert B.setOrdinal(rel) is None
    assert rel.model.ordinal == {"K": 5, "step": 0.1, "sample_edges": True}
    assert rel.model.ordinal_codes.dtype == np.int8 and np.array_equal(rel.model.ordinal_codes, rel.data.values)
    assert np.array_equal(rel.model.ordinal_edges, [1.5, 2.5, 3.5, 4.5])
    ref = _relation(B, test=np.arange(1, 13))
    B.setBinned(ref, [1.5, 2.5, 3.5, 4.5])
    assert np.array_equal(rel.model.interval, ref.model.interval) and rel.model.interval.flags["C_CONTIGUOUS"]
    assert " ord:5" in B.toStr(rel) and " intv:48" in B.toStr(rel) and " ord:" not in B.toStr(ref)
    B.setOrdinal(rel, n_levels=7, step=0.5, sample_edges=False)                    # more levels than occur; set again
    assert rel.model.ordinal == {"K": 7, "step": 0.5, "sample_edges": False} and len(rel.model.ordinal_edges) == 6
    B.setOrdinal(_relation(B, K=16))
    B.setOrdinal(_relation(B, K=4))


def test_setordinal_refusals(B):
    for K, pattern in ((3, "setBinned"), (2, "4 ... 16"), (17, "4 ... 16")):
        with pytest.raises(B.ArgumentError, match=pattern):
            B.setOrdinal(_relation(B, K=K))
    with pytest.raises(B.ArgumentError, match="setBinned"):
        B.setOrdinal(_relation(B), n_levels=3)
    for bad in (np.arange(60) % 5 + 0.5, np.arange(60) % 5 + 0.0, np.where(np.arange(60) == 7, np.nan, 2.0), np.where(np.arange(60) == 7, INF, 2.0)):
        with pytest.raises(B.ArgumentError, match="integers 1"):
            B.setOrdinal(_relation(B, values=bad), n_levels=5)
    with pytest.raises(B.ArgumentError, match="integers 1"):
        B.setOrdinal(_relation(B), n_levels=4)                                     # a 5 among four levels
    for bad in (4.5, True, float("nan"), INF, -INF, "5", [5]):
        with pytest.raises(B.ArgumentError, match="n_levels"):
            B.setOrdinal(_relation(B), n_levels=bad)
    for bad in (0.0, -1.0, 11.0, float("nan")):
        with pytest.raises(B.ArgumentError, match="step"):
            B.setOrdinal(_relation(B), step=bad)
    # exclusive with the other noise models, whichever comes first
    rel = _relation(B, values=np.arange(60) % 2)
    B.setProbit(rel)
    with pytest.raises(B.ArgumentError, match="setProbit"):
        B.setOrdinal(rel, n_levels=4)
    rel = _relation(B)
    B.setCensored(rel, np.zeros(60, dtype=np.int8))
    with pytest.raises(B.ArgumentError, match="setCensored"):
        B.setOrdinal(rel)
    rel = _relation(B)
    B.setBinned(rel, [2.5])
    with pytest.raises(B.ArgumentError, match="setOrdinal"):
        B.setOrdinal(rel)
    rel = _relation(B)
    B.setOrdinal(rel)
    with pytest.raises(B.ArgumentError):
        B.setProbit(rel)
    with pytest.raises(B.ArgumentError):
        B.setCensored(rel, np.zeros(60, dtype=np.int8))
    with pytest.raises(B.ArgumentError, match="setOrdinal"):
        B.setInterval(rel, rel.data.values - 0.5, rel.data.values + 0.5)
    with pytest.raises(B.ArgumentError, match="setOrdinal"):
        B.setBinned(rel, [1.5, 2.5, 3.5, 4.5])
    with pytest.raises(B.ArgumentError, match="assignToTest before"):           # the interval model's guard: the test split comes first
        B.assignToTest(rel, np.arange(1, 5))
    rel = _relation(B)
    rel.F = np.ones((60, 2))
    with pytest.raises(B.ArgumentError, match="features"):
        B.setOrdinal(rel)
    assert rel.model.ordinal is None and rel.model.interval is None


def test_settestordinal_and_what_drops_it(B):
    rel = _relation(B, test=np.arange(1, 13))
    with pytest.raises(B.ArgumentError, match="setOrdinal"):
        B.setTestOrdinal(rel)
    B.setOrdinal(rel)
    assert B.setTestOrdinal(rel) is None
    assert rel.model.test_ordinal.dtype == np.int8 and np.array_equal(rel.model.test_ordinal, rel.test_vec.values)
    assert rel.model.test_interval is None
    B.setTestBinned(rel, [1.5, 2.5, 3.5, 4.5])                                     # fixed test bins take the sampled ones' place
    assert rel.model.test_ordinal is None and rel.model.test_interval is not None
    B.setTestOrdinal(rel)
    assert rel.model.test_interval is None
    B.setTest(rel, {"u": [1, 2], "v": [1, 2], "y": [6.0, 2.0]})                    # a new test table drops the levels
    assert rel.model.test_ordinal is None
    with pytest.raises(B.ArgumentError, match="integers 1"):                       # ... and a 6 is no level of five
        B.setTestOrdinal(rel)
    B.setTest(rel, {"u": [1, 2], "v": [1, 2], "y": [2.5, 2.0]})
    with pytest.raises(B.ArgumentError, match="integers 1"):
        B.setTestOrdinal(rel)


def test_macau_signature_is_unchanged_and_rmse_train_is_refused(B):
    import inspect
    from bdf_amd.driver import macau
    params = list(inspect.signature(macau).parameters)
    assert params[-1] == "lpd" and "ordinal" not in params and len(params) == 24
    rel = _relation(B)
    B.setOrdinal(rel)
    with pytest.raises(B.ArgumentError, match="rmse_train"):
        macau(B.RelationData(rel), rmse_train=True, verbose=False)


# ---- the resource listing ---------------------------------------------------------------------------------------------------------
# (VGPRs, scratch bytes per lane, waves per SIMD) of the nine shapes <modes, vector width, row pieces> of k_ordinal_mass, as
# DESIGN.md section 16 prints them
MASS_KERNELS = {
    "14k_ordinal_massILi2ELi1ELi1EEEvNS_11OrdMassArgsE": (43, 0, 8),
    "14k_ordinal_massILi2ELi4ELi1EEEvNS_11OrdMassArgsE": (87, 0, 5),
    "14k_ordinal_massILi2ELi4ELi2EEEvNS_11OrdMassArgsE": (89, 0, 5),
    "14k_ordinal_massILi3ELi1ELi1EEEvNS_11OrdMassArgsE": (43, 0, 8),
    "14k_ordinal_massILi3ELi4ELi1EEEvNS_11OrdMassArgsE": (120, 0, 4),
    "14k_ordinal_massILi3ELi4ELi2EEEvNS_11OrdMassArgsE": (122, 0, 4),
    "14k_ordinal_massILi4ELi1ELi1EEEvNS_11OrdMassArgsE": (44, 0, 8),
    "14k_ordinal_massILi4ELi4ELi1EEEvNS_11OrdMassArgsE": (89, 0, 5),
    "14k_ordinal_massILi4ELi4ELi2EEEvNS_11OrdMassArgsE": (155, 0, 3),
}


def test_ordinal_kernels_use_no_scratch_and_only_the_reduction_and_table_lds():
    res = _resources("k_ordinal")
    shapes = {k: v for k, v in res.items() if "k_ordinal_massI" in k}
    assert shapes == MASS_KERNELS
    for k, v in res.items():                          # the nine shapes, propose, accept, bounds (and predict.h's unused final sum)
        assert v[1] == 0 and v[2] >= 2, (k, v)
    assert len(res) == 13
    text = open(os.path.join(ROOT, "bayesiandatafusion.jl_amd", "csrc", "k_ordinal.o.res")).read()
    lds = dict(zip(re.findall(r"Function Name: (\S+)", text), (int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", text))))
    for name, bytes_ in lds.items():
        # mass: 4 statistics x 4 waves of doubles + two tables of 17 doubles; propose: 16 normals; accept: 4 waves' sums; bounds: none
        want = 128 + 2 * 17 * 8 if "k_ordinal_mass" in name else 128 if ("propose" in name or "k_predict_final" in name) else 32 if "accept" in name else 0
        assert bytes_ == want, (name, bytes_)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## 16." in design
    for k, (vgprs, scratch, waves) in MASS_KERNELS.items():
        nm, vec, nc = re.search(r"ILi(\d)ELi(\d)ELi(\d)E", k).groups()
        assert re.search(rf"\|\s*{nm}\s*\|\s*{vec}\s*\|\s*{nc}\s*\|\s*{vgprs}\s*\|\s*{scratch}\s*\|\s*400\s*\|\s*{waves}\s*\|", design), k
