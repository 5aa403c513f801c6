"""Cells of new rows on the host (no GPU): setNewRows / setNewTest and everything they refuse, the closed-form
marginal of tests/newrows_restatement.py against 400,000 sampled factors of a new row, csrc/newrows.h compiled for the host against
the restated stream, the recorded quality figures against the computation, and the resource listing the build leaves for the
kernels of k_newrows.hip (no scratch)."""
import inspect
import math
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
import scipy.sparse as sp

import lpd_restatement as LR
import newrows_restatement as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the setters ----------------------------------------------------------------------------------------------------------------------
def _relation(B, values=None, n=60, feats=True, modes=2, seed=3):
    rng = np.random.default_rng(seed)
    dims = [9, 7, 4][:modes]
    ids = np.stack([rng.integers(1, d + 1, n) for d in dims], axis=1)
    ids = np.unique(ids, axis=0)
    y = rng.standard_normal(len(ids)) if values is None else np.resize(np.asarray(values, dtype=np.float64), len(ids))
    names = ["u", "v", "w"][:modes]
    ents = [B.Entity(nm) for nm in names]
    if feats:
        ents[0].F = rng.standard_normal((dims[0], 5))
    table = {nm: ids[:, k] for k, nm in enumerate(names)}
    table["y"] = y
    return B.Relation(table, "ratings", ents, alpha=2.0, dims=dims), ents


def _new_table(n_new=4, n_other=7, values=None):
    ids = np.array([[1, 1], [2, 7], [n_new, 3], [1, 2]])
    vals = np.array([0.5, float("nan"), -1.0, 2.0]) if values is None else np.asarray(values, dtype=np.float64)
    return {"u": ids[:, 0], "v": ids[:, 1], "y": vals}


def test_setters_round_trip_and_clear(B):
    rel, (u, v) = _relation(B)
    assert u.new_rows is None and rel.model.new_test is None and B.Entity("x").new_rows is None and B.RelationModel().new_test is None
    Fn = np.arange(20.0).reshape(4, 5)
    assert B.setNewRows(u, Fn) is None and u.new_rows is Fn
    for other in (sp.csr_matrix(Fn), B.sparse_csr(sp.csr_matrix(Fn)), B.SparseBinMatrix(4, 5, [1, 2, 4], [1, 5, 3])):
        B.setNewRows(u, other)
        assert u.new_rows is other
    B.setNewRows(u, Fn)
    assert B.setNewTest(rel, u, _new_table()) is None
    m = rel.model.new_test
    assert m["mode"] == 1 and m["ids"].dtype == np.int64 and m["ids"].shape == (4, 2) and np.isnan(m["values"][1]) and m["values"][0] == 0.5
    B.setNewTest(rel, u, (np.array([[1.0, 2.0]]), np.array([3.0])))            # ids as whole floats, a table as (ids, values)
    assert rel.model.new_test["ids"].tolist() == [[1, 2]]
    from bdf_amd.relation_data import check_new_rows
    assert check_new_rows(B.RelationData(rel)) is rel
    B.setNewTest(rel, u, None)
    assert rel.model.new_test is None and check_new_rows(B.RelationData(rel)) is None
    B.setNewRows(u, None)
    assert u.new_rows is None
    # the entity in the relation's second column: the new row's id is the second one
    rel2, (a, b) = _relation(B, feats=False)
    b.F = np.ones((7, 3))
    B.setNewRows(b, np.ones((2, 3)))
    B.setNewTest(rel2, b, {"u": [9, 1], "v": [2, 1], "y": [0.0, 1.0]})
    assert rel2.model.new_test["mode"] == 2


def test_setnewrows_refusals(B):
    rel, (u, v) = _relation(B)
    with pytest.raises(B.ArgumentError, match="takes an Entity"):
        B.setNewRows(rel, np.ones((2, 5)))
    with pytest.raises(B.ArgumentError, match="has no features"):
        B.setNewRows(v, np.ones((2, 5)))
    with pytest.raises(B.ArgumentError, match="has 4 columns but the entity's features have 5"):
        B.setNewRows(u, np.ones((2, 4)))
    with pytest.raises(B.ArgumentError, match="F_new is empty"):
        B.setNewRows(u, np.ones((0, 5)))
    assert u.new_rows is None                                        # a refused call changes nothing
    plain, (a, b) = _relation(B, feats=False)
    B.setSpikeAndSlab(a)
    a.F = np.ones((9, 5))                                            # (behind the setter's back: the setter itself refuses features)
    with pytest.raises(B.ArgumentError, match="spike-and-slab"):
        B.setNewRows(a, np.ones((2, 5)))


def test_setnewtest_refusals(B):
    rel, (u, v) = _relation(B)
    with pytest.raises(B.ArgumentError, match="call setNewRows"):
        B.setNewTest(rel, u, _new_table())                          # setNewTest without setNewRows
    B.setNewRows(u, np.ones((4, 5)))
    with pytest.raises(B.ArgumentError, match="takes an Entity"):
        B.setNewTest(rel, "u", _new_table())
    with pytest.raises(B.ArgumentError, match="has no entity"):
        B.setNewTest(rel, B.Entity("z"), _new_table())
    with pytest.raises(B.ArgumentError, match="has no new rows"):
        B.setNewTest(rel, v, _new_table())
    for bad, what in (({"u": [5], "v": [1], "y": [0.0]}, "outside 1 ... 4, the rows of F_new"), ({"u": [0], "v": [1], "y": [0.0]}, "outside 1 ... 4"),
                      ({"u": [1], "v": [8], "y": [0.0]}, "outside 1 ... 7"), ({"u": [1], "v": [0], "y": [0.0]}, "outside 1 ... 7"),
                      ({"u": [1.5], "v": [1], "y": [0.0]}, "must be integers"), ({"u": [1], "v": [1], "y": [float("inf")]}, "must be finite"),
                      ({"u": [1], "y": [0.0]}, "two id columns")):
        with pytest.raises(B.ArgumentError, match=what):
            B.setNewTest(rel, u, bad)
    assert rel.model.new_test is None
    # three modes
    r3, ents = _relation(B, modes=3)
    B.setNewRows(ents[0], np.ones((4, 5)))
    with pytest.raises(B.ArgumentError, match="has 3 modes"):
        B.setNewTest(r3, ents[0], {"u": [1], "v": [1], "w": [1], "y": [0.0]})
    # relation-level features
    rf, (a, b) = _relation(B)
    B.setNewRows(a, np.ones((4, 5)))
    rf.F = np.ones((rf.data.nnz(), 2))
    with pytest.raises(B.ArgumentError, match="relation-level side information"):
        B.setNewTest(rf, a, _new_table())
    # the noise models without a closed form, or whose new cell's weight is unknown
    def fresh(values=None):
        r, (a, b) = _relation(B, values=values)
        B.setNewRows(a, np.ones((4, 5)))
        return r, a

    r, a = fresh(values=[0.0, 1.0])
    B.setLogit(r)
    with pytest.raises(B.ArgumentError, match=r"logit noise model \(setLogit\): the marginal"):
        B.setNewTest(r, a, _new_table())
    r, a = fresh(values=[0.0, 3.0, 1.0])
    B.setCounts(r, 2)
    with pytest.raises(B.ArgumentError, match=r"count noise model \(setCounts\): the marginal"):
        B.setNewTest(r, a, _new_table())
    r, a = fresh()
    B.setRobust(r)
    with pytest.raises(B.ArgumentError, match=r"robust noise model \(setRobust\)"):
        B.setNewTest(r, a, _new_table())
    r, a = fresh()
    B.setWeights(r, np.ones(r.data.nnz()))
    with pytest.raises(B.ArgumentError, match=r"observation weights \(setWeights\): the weight of a new cell is unknown"):
        B.setNewTest(r, a, _new_table())
    r, a = fresh()
    B.setEntityNoise(r, a)
    with pytest.raises(B.ArgumentError, match=r"noise precision per row \(setEntityNoise\)"):
        B.setNewTest(r, a, _new_table())
    r, a = fresh(values=[1.0, 2.0, 3.0, 4.0])
    B.setOrdinal(r)
    with pytest.raises(B.ArgumentError, match=r"ordinal noise model \(setOrdinal\)"):
        B.setNewTest(r, a, _new_table())
    # probit: values 0 / 1 or NaN
    r, a = fresh(values=[0.0, 1.0])
    B.setProbit(r)
    with pytest.raises(B.ArgumentError, match="must be 0, 1 or NaN"):
        B.setNewTest(r, a, _new_table())
    B.setNewTest(r, a, _new_table(values=[1.0, float("nan"), 0.0, 1.0]))
    assert r.model.new_test is not None
    # allowed: censored, interval / binned, background, a sampled alpha
    for setter in (lambda r: B.setCensored(r, np.zeros(r.data.nnz(), dtype=np.int8)), lambda r: B.setBinned(r, [-0.5, 0.5]),
                   lambda r: B.setBackground(r, 0.1), lambda r: setattr(r.model, "alpha_sample", True)):
        r, a = fresh()
        setter(r)
        B.setNewTest(r, a, _new_table())
        assert r.model.new_test["mode"] == 1


def test_macau_time_checks(B):
    """what is looked at again when macau() runs: a relation that is not the first, more than one rank, a model or features changed
    behind the setters' backs"""
    from bdf_amd.relation_data import check_new_rows
    rel, (u, v) = _relation(B)
    B.setNewRows(u, np.ones((4, 5)))
    B.setNewTest(rel, u, _new_table())
    rd = B.RelationData(rel)
    assert check_new_rows(rd) is rel
    with pytest.raises(B.ArgumentError, match="one rank only"):
        check_new_rows(rd, world=2)
    other, _ = _relation(B, feats=False, seed=4)
    second = B.Relation({"u": [1, 2], "v": [1, 2], "y": [0.0, 1.0]}, "second", [u, v], dims=[9, 7])
    second.model.new_test = dict(rel.model.new_test)
    rd2 = B.RelationData(rel)
    B.addRelation(rd2, second)
    with pytest.raises(B.ArgumentError, match="is not the first relation"):
        check_new_rows(rd2)
    B.setNewRows(u, None)
    with pytest.raises(B.ArgumentError, match="call setNewRows"):
        check_new_rows(rd)
    B.setNewRows(u, np.ones((3, 5)))                                # fewer new rows than the table addresses
    with pytest.raises(B.ArgumentError, match="outside 1 ... 3"):
        check_new_rows(rd)
    B.setNewRows(u, np.ones((4, 5)))
    B.setRobust(rel)
    with pytest.raises(B.ArgumentError, match="setRobust"):
        check_new_rows(rd)

    class TwoRanks:                    # what an engine built with shard=(rank, 2) says of itself
        world, D = 2, 2

    rel, (u, v) = _relation(B)
    B.setNewRows(u, np.ones((4, 5)))
    B.setNewTest(rel, u, _new_table())
    from bdf_amd.driver import macau
    with pytest.raises(B.ArgumentError, match="one rank only"):
        macau(B.RelationData(rel), num_latent=2, burnin=1, psamples=2, verbose=False, engine=TwoRanks(), reset_model=False)


def test_macau_signature_is_untouched():
    from bdf_amd.driver import macau
    params = list(inspect.signature(macau).parameters.values())
    assert len(params) == 24 and params[-1].name == "lpd" and params[-1].default is False


# ---- the marginalisation ----------------------------------------------------------------------------------------------------------------
def test_the_closed_form_is_the_marginal_over_the_new_rows_factor():
    """For one fixed draw (mu, Lambda, beta, V, alpha) and six cells: 400,000 factors u* ~ N(uhat, Lambda^-1) (seeded).  The mean and
    the variance of mean_value + u* . v over them against the restatement's m and q, the variance of a value with its noise against
    q + 1 / alpha, and the share of z = u* . v + eps > 0 against the probit probability Phi(m / sqrt(1 + q)): each within four
    Monte-Carlo standard errors (of a mean: sd / sqrt n; of a variance of Gaussian values: var sqrt(2 / (n - 1)); of a share:
    sqrt(p (1 - p) / n))"""
    rng = np.random.default_rng(11)
    D, numF, M, n = 5, 4, 6, 400_000
    A = rng.standard_normal((D, D))
    Lam = A @ A.T / D + np.eye(D)
    mu, beta, V = rng.standard_normal(D) * 0.3, rng.standard_normal((numF, D)) * 0.5, rng.standard_normal((M, D))
    F = rng.standard_normal((2, numF))
    alpha, mean = 3.0, 0.25
    uh = NR.uhat(mu, beta, F)
    assert np.allclose(uh[1], mu + beta.T @ F[1], rtol=1e-14)
    q = NR.quad(Lam, V)
    assert np.allclose(q, [V[j] @ np.linalg.inv(Lam) @ V[j] for j in range(M)], rtol=1e-12)
    ids = np.array([[1, 1], [1, 4], [2, 2], [2, 6], [1, 3], [2, 5]])
    m, qc = NR.cells(ids, uh, V, q, mean)
    Lc = np.linalg.cholesky(np.linalg.inv(Lam))
    worst = 0.0
    for k, (i, j) in enumerate(ids - 1):
        u = uh[i][None, :] + rng.standard_normal((n, D)) @ Lc.T
        f = mean + u @ V[j]
        y = f + rng.standard_normal(n) / math.sqrt(alpha)
        z = (f - mean) + rng.standard_normal(n)                     # the probit latent is not centred: mean_value = 0 there
        p_ref = float(NR.predict(True, m[k] - mean, qc[k]))
        errs = (abs(f.mean() - m[k]) / math.sqrt(qc[k] / n), abs(f.var(ddof=1) - qc[k]) / (qc[k] * math.sqrt(2.0 / (n - 1))),
                abs(y.mean() - float(NR.predict(False, m[k], qc[k]))) / math.sqrt((qc[k] + 1.0 / alpha) / n),
                abs(y.var(ddof=1) - (qc[k] + 1.0 / alpha)) / ((qc[k] + 1.0 / alpha) * math.sqrt(2.0 / (n - 1))),
                abs((z > 0).mean() - p_ref) / math.sqrt(p_ref * (1.0 - p_ref) / n))
        worst = max(worst, *errs)
        assert max(errs) <= 4.0, (k, errs)
        # the log-likelihood is the log density of that Gaussian, and of that Bernoulli
        yv = 0.7
        want = -0.5 * math.log(2.0 * math.pi * (qc[k] + 1.0 / alpha)) - 0.5 * (yv - m[k]) ** 2 / (qc[k] + 1.0 / alpha)
        assert abs(float(NR.loglik(False, np.array([yv]), m[k:k + 1], qc[k:k + 1], alpha)[0]) - want) <= 1e-12 * max(1.0, abs(want))
        for yb, pb in ((1.0, p_ref), (0.0, 1.0 - p_ref)):
            got = float(NR.loglik(True, np.array([yb]), m[k:k + 1] - mean, qc[k:k + 1], alpha)[0])
            assert abs(got - math.log(pb)) <= 1e-12 * max(1.0, abs(math.log(pb)))
    print(f"marginal against 400,000 sampled factors: worst deviation {worst:.2f} Monte-Carlo standard errors (asserted: 4)")
    assert np.isnan(NR.loglik(False, np.array([np.nan]), m[:1], qc[:1], alpha)[0])


def test_stream_is_the_mean_the_sample_variance_and_logsumexp():
    from scipy.special import logsumexp
    rng = np.random.default_rng(5)
    S, n = 30, 200
    p, q, l = rng.standard_normal((S, n)) * 3.0 + 100.0, rng.random((S, n)), rng.uniform(-900.0, -1.0, (S, n))
    l[:, 7] = np.nan                                                # a cell without a value
    p[:, 3] = 2.5                                                   # equal draws: M2 exactly 0
    st = NR.Stream()
    avg, lpd = st.update(p[4], q[4], l[4], 0)
    assert np.array_equal(avg, p[4]) and st.draws == 0 and st.mean is None
    for s in range(S):
        avg, lpd = st.update(p[s], q[s], l[s], 1 if s == 0 else 2)
        assert np.allclose(avg, p[:s + 1].mean(axis=0), rtol=1e-13) and st.M2[3] == 0.0
        ok = ~np.isnan(l[0])
        assert np.allclose(lpd[ok], logsumexp(l[:s + 1, ok], axis=0) - math.log(s + 1), rtol=1e-12) and np.isnan(lpd[7])
        if s >= 1:
            want = np.sqrt(p[:s + 1].var(axis=0, ddof=1) + q[:s + 1].mean(axis=0))
            assert np.allclose(st.stdev(False), want, rtol=1e-10) and np.allclose(st.stdev(True), p[:s + 1].std(axis=0, ddof=1), rtol=1e-8, atol=1e-12)
        else:
            assert np.isnan(st.stdev(False)).all()


def test_header_and_restatement_state_the_same_stream():
    """csrc/newrows.h, the text the kernel folds a draw in with, compiled for the host: 30 draws of 200 cells through
    bdf_newrows_predict / _loglik / _start / _fold / _stdev against the restated stream after every draw, both links: 1e-12 relative to
    max(1, |value|)"""
    cxx = [shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")]
    if cxx[0] is None:
        cxx = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "c++"]
    src = r'''
        #include <cstdio>
        #include <cmath>
        #include <vector>
        #include "newrows.h"
        int main() { int S, n, link; double alpha; if (scanf("%d %d %d %lf", &S, &n, &link, &alpha) != 4) return 1;
                     std::vector<bdf_newrows_cell> c(n);
                     for (int s = 0; s < S; s++) for (int t = 0; t < n; t++) { double y, m, q; if (scanf("%lf %lf %lf", &y, &m, &q) != 3) return 1;
                         const bool scored = y == y;
                         const double p = bdf_newrows_predict(link, m, q);
                         double l = 0.0, lpd;
                         if (scored) l = bdf_newrows_loglik(link, y, m, q, alpha);
                         lpd = l;
                         if (s == 0) bdf_newrows_start(p, q, scored, l, c[t]); else lpd = bdf_newrows_fold(p, q, scored, l, s + 1.0, log(s + 1.0), c[t]);
                         printf("%.17g %.17g %.17g %.17g %.17g\n", c[t].mean, c[t].M2, c[t].sq, scored ? lpd : NAN, bdf_newrows_stdev(link, c[t].M2, c[t].sq, s + 1.0)); }
                     return 0; }
    '''
    rng = np.random.default_rng(9)
    S, n, alpha = 30, 200, 2.5
    m, q = rng.standard_normal((S, n)) * 4.0, rng.random((S, n)) * 3.0
    m[:, 0], q[:, 0] = 90.0, 0.21                                   # the probit map's far tail for y = 0: Phi(-81.8)
    worst = 0.0
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "t.cpp"), "w").write(src)
        subprocess.run(cxx + ["-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "bayesiandatafusion.jl_amd", "csrc"), os.path.join(td, "t.cpp"),
                        "-o", os.path.join(td, "t")], check=True)
        for link in (0, 1):
            y = (rng.random(n) < 0.5).astype(np.float64) if link else rng.standard_normal(n)
            y[0], y[5] = 0.0, np.nan
            text = "%d %d %d %.17g\n" % (S, n, link, alpha) + "".join("%s %.17g %.17g\n" % ("nan" if np.isnan(y[t]) else "%.17g" % y[t], m[s, t], q[s, t])
                                                                       for s in range(S) for t in range(n))
            out = subprocess.run([os.path.join(td, "t")], input=text, capture_output=True, text=True, check=True).stdout
            got = np.array([float(t) for t in out.split()]).reshape(S, n, 5)
            st = NR.Stream()
            for s in range(S):
                avg, lpd = st.update(NR.predict(link, m[s], q[s]), q[s], NR.loglik(link, y, m[s], q[s], alpha), 1 if s == 0 else 2)
                for k, ref in enumerate((st.mean, st.M2, st.sq, lpd, st.stdev(link))):
                    assert np.array_equal(np.isnan(got[s, :, k]), np.isnan(ref)), (link, s, k)
                    ok = ~np.isnan(ref)
                    e = (np.abs(got[s, ok, k] - ref[ok]) / np.maximum(1.0, np.abs(ref[ok]))).max() if ok.any() else 0.0
                    worst = max(worst, e)
                    assert e <= 1e-12, (link, s, k, e)
            assert np.isnan(got[:, 5, 3]).all() and np.isfinite(got[:, 0, 3]).all() and (link == 0 or got[-1, 0, 3] < -900.0)
    print(f"newrows.h against the restatement: worst error relative to max(1, |value|) {worst:.2e}")


# ---- the quality record ---------------------------------------------------------------------------------------------------------------
def test_recorded_quality_figures_are_what_the_restatement_computes():
    """the first of the five recorded CPU chains recomputed: its ratio (cold RMSE) / (RMSE of predicting mean_value) and its coverage
    of pred +- 1.645 sqrt(stdev^2 + 1 / alpha); and the planted signal is strong: every recorded ratio is well below 0.8"""
    sh = dict(NR.QUALITY_SHAPE)
    Ft, Fn, train, new = NR.planted(**sh)
    g = NR.gibbs(Ft, train, Fn, new, sh["M"], sh["D"], NR.QUALITY_ALPHA, *NR.QUALITY_ITERS, NR.QUALITY_SEEDS[0])
    assert abs(g["ratio"] - NR.QUALITY_CPU_RATIOS[0]) <= 5e-6 and abs(g["coverage"] - NR.QUALITY_CPU_COVERAGE[0]) <= 5e-6
    assert len(NR.QUALITY_CPU_RATIOS) == len(NR.QUALITY_CPU_COVERAGE) == len(NR.QUALITY_SEEDS) == 5
    assert max(NR.QUALITY_CPU_RATIOS) < 0.8 and 0.85 < min(NR.QUALITY_CPU_COVERAGE) and max(NR.QUALITY_CPU_COVERAGE) < 0.95


# ---- the resource listing ---------------------------------------------------------------------------------------------------------
def _resources(unit):
    path = os.path.join(ROOT, "bayesiandatafusion.jl_amd", "csrc", unit + ".o.res")
    assert os.path.exists(path), "no csrc/%s.o.res: build with __graft_entry__.build() (make)" % unit
    res, name = {}, None
    for line in open(path):
        mt = re.search(r"remark: \s*(Function Name|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
        if not mt:
            continue
        if mt.group(1) == "Function Name":
            name = mt.group(2).replace("_ZN12_GLOBAL__N_1", "")
            res[name] = {}
        elif name is not None:
            res[name][mt.group(1).split(" ")[0]] = int(mt.group(2))
    return res


def test_newrows_kernels_use_no_scratch():
    res = _resources("k_newrows")
    quad = {k: v for k, v in res.items() if "k_newrows_quadI" in k}
    update = {k: v for k, v in res.items() if "k_newrows_updateI" in k}
    assert len(quad) == 3 and len(update) == 3                      # DP = 16, 32, 64; <vector width, row pieces> = <1, 1>, <4, 1>, <4, 2>
    assert sum("k_newrows_prep" in k for k in res) == 1 and sum("k_newrows_final" in k for k in res) == 1 and sum("k_newrows_read" in k for k in res) == 1
    for k, v in res.items():
        assert v["ScratchSize"] == 0, (k, v)
    for k, v in update.items():
        assert v["Occupancy"] >= 4 and v["LDS"] == 256, (k, v)       # 8 statistics x 4 waves of doubles, nothing else
    for k, v in quad.items():
        dp = int(re.search(r"quadILi(\d+)E", k).group(1))
        assert v["LDS"] == dp * (dp + 2) * 8 and v["Occupancy"] >= 2, (k, v)       # W with its padded leading dimension
