"""WAIC on the training cells on the host (no GPU): the restated stream of tests/waic_restatement.py against scipy's logsumexp and
numpy's variance, Jensen's inequality between its two halves, csrc/waic.h compiled for the host against it, the table that says what kind of record a training row is, setWaic and
what macau() refuses with it, the recorded quality gaps against the computation, and the resource listing the build leaves for
k_waic."""
import inspect
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
from scipy.special import logsumexp

import waic_restatement as WR
from test_probit_host import _resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.inf


# ---- the stream -----------------------------------------------------------------------------------------------------------------------
def _draws():
    """40 draws whose log-likelihoods span -2,000 ... -1 for each of 300 cells; cell 5 has every draw equal, cells 0 .. 4 the whole
    span, cell 6 draws 1e-9 apart"""
    rng = np.random.default_rng(3)
    S, n = 40, 300
    l = rng.uniform(-2000.0, -1.0, (S, n))
    l[0, :5], l[-1, :5] = -2000.0, -1.0
    l[:, 5] = -700.0
    l[:, 6] = np.linspace(-1.0 - 1e-9, -1.0, S)
    return l


def _close(got, want, tol=1e-12):
    return np.all(np.abs(got - want) <= tol * np.maximum(1.0, np.abs(want)))


def test_stream_matches_logsumexp_and_the_sample_variance():
    """after every draw: lppd against scipy.special.logsumexp - log S and V against numpy.var(ddof=1), both to 1e-12 max(1, |value|);
    V exactly 0 after one draw and for the cell whose draws are all equal; burn-in draws leave no trace; and Jensen's inequality,
    lppd >= the Welford mean, in every cell after every draw -- it ties the two halves of the state to each other"""
    l = _draws()
    S = len(l)
    rng = np.random.default_rng(4)
    worst_l = worst_v = 0.0
    for order in (np.arange(S), np.arange(S)[::-1], np.argsort(l[:, 0]), rng.permutation(S)):
        st = WR.Stream()
        lp, V = st.update(l[3] - 5.0, 0)
        assert np.array_equal(lp, l[3] - 5.0) and not V.any() and st.draws == 0 and st.M is None and st.M2 is None
        for k, s in enumerate(order):
            lp, V = st.update(l[s], 1 if k == 0 else 2)
            seen = l[order[:k + 1]]
            want_l = logsumexp(seen, axis=0) - np.log(k + 1)
            want_v = np.var(seen, axis=0, ddof=1) if k >= 1 else np.zeros(l.shape[1])
            assert _close(lp, want_l) and _close(V, want_v), (k, np.abs(lp - want_l).max(), np.abs(V - want_v).max())
            worst_l = max(worst_l, (np.abs(lp - want_l) / np.maximum(1.0, np.abs(want_l))).max())
            worst_v = max(worst_v, (np.abs(V - want_v) / np.maximum(1.0, np.abs(want_v))).max())
            if k == 0:
                assert not V.any()                                  # one draw: exactly 0
            assert V[5] == 0.0 and st.M2[5] == 0.0                  # equal draws: exactly 0
            assert np.all(V >= 0.0)
            assert np.all(lp >= st.mean - 1e-12 * np.maximum(1.0, np.abs(st.mean)))          # Jensen
        assert st.draws == S
    print(f"stream: worst relative error of lppd {worst_l:.2e}, of V {worst_v:.2e}")
    st.update(l[7], 1)                                              # a first draw starts over
    assert st.draws == 1 and np.array_equal(st.lppd(), l[7]) and not st.V().any()


def test_stream_of_equal_draws():
    l = np.tile(np.array([-1.0, -3.25, -700.0, -1999.5, 0.0, 2.5]), (40, 1))
    st = WR.Stream()
    for k in range(40):
        lp, V = st.update(l[k], 1 if k == 0 else 2)
        assert _close(lp, logsumexp(l[:k + 1], axis=0) - np.log(k + 1)) and not V.any() and np.array_equal(st.mean, l[0])
        assert _close(V, np.var(l[:k + 1], axis=0, ddof=1) if k else 0.0)


def test_header_and_restatement_state_the_same_stream():
    """csrc/waic.h, the text the kernel folds a draw in with, compiled for the host (as test_lpd_host.py compiles lpd.h): 40 draws of
    300 cells through bdf_waic_start and bdf_waic_fold against the restated stream after every draw.  The same operations in the
    same order on two exp / log implementations: 1e-12 relative to max(1, |value|) for lppd and V, V exactly 0 for equal draws"""
    cxx = [shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")]
    if cxx[0] is None:
        cxx = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "c++"]
    src = r'''
        #include <cstdio>
        #include <cmath>
        #include <vector>
        #include "waic.h"
        int main() { int S, n; if (scanf("%d %d", &S, &n) != 2) return 1;
                     std::vector<bdf_waic_cell> c(n);
                     for (int s = 0; s < S; s++) for (int t = 0; t < n; t++) { double l, lppd, V = 0.0; if (scanf("%lf", &l) != 1) return 1;
                         lppd = l; if (s == 0) bdf_waic_start(l, c[t]); else bdf_waic_fold(l, s + 1.0, log(s + 1.0), c[t], lppd, V);
                         printf("%.17g %.17g %.17g\n", lppd, V, c[t].mu); }
                     return 0; }
    '''
    l = _draws()
    S, n = l.shape
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "t.cpp"), "w").write(src)
        subprocess.run(cxx + ["-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "bayesiandatafusion.jl_amd", "csrc"), os.path.join(td, "t.cpp"),
                        "-o", os.path.join(td, "t")], check=True)
        text = "%d %d\n" % (S, n) + "".join("%.17g\n" % v for v in l.ravel())
        out = subprocess.run([os.path.join(td, "t")], input=text, capture_output=True, text=True, check=True).stdout
    got = np.array([float(t) for t in out.split()]).reshape(S, n, 3)
    st = WR.Stream()
    worst = 0.0
    for s in range(S):
        lp, V = st.update(l[s], 1 if s == 0 else 2)
        assert _close(got[s, :, 0], lp) and _close(got[s, :, 1], V) and _close(got[s, :, 2], st.mean)
        worst = max(worst, (np.abs(got[s, :, 0] - lp) / np.maximum(1.0, np.abs(lp))).max(), (np.abs(got[s, :, 1] - V) / np.maximum(1.0, np.abs(V))).max())
        assert got[s, 5, 1] == 0.0
    print(f"waic.h against the restatement: worst error relative to max(1, |value|) {worst:.2e}")


def test_summary_is_the_definition():
    rng = np.random.default_rng(8)
    lppd, V = -rng.uniform(0.5, 3.0, 500), rng.uniform(0.0, 0.8, 500)
    s = WR.summary(lppd, V)
    e = lppd - V
    assert abs(s["lppd"] - lppd.sum()) <= 1e-10 and abs(s["p_waic"] - V.sum()) <= 1e-10 and abs(s["elpd"] - e.sum()) <= 1e-10
    assert s["waic"] == -2.0 * s["elpd"] and s["n"] == 500 and s["n_high"] == int((V > 0.4).sum()) and 0 < s["n_high"] < 500
    assert abs(s["se"] - np.sqrt(500 * np.var(e))) <= 1e-10
    # shifted by 1e8 the squares about the mean keep their digits (a difference of two sums of squares would keep none)
    assert abs(WR.summary(lppd - 1e8, V)["se"] - s["se"]) <= 1e-6


# ---- what kind of record a training row is ------------------------------------------------------------------------------------------
def _relation(B, values=None, n=40, alpha=2.0):
    rng = np.random.default_rng(3)
    ids = np.stack([rng.integers(1, 9, n), rng.integers(1, 7, n)], axis=1)
    y = rng.standard_normal(n) if values is None else np.asarray(values, dtype=np.float64)
    return B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "ratings", [B.Entity("u"), B.Entity("v")], alpha=alpha, dims=[8, 6])


def test_the_kind_of_record_of_every_noise_model(B):
    from bdf_amd.relation_data import _ordinal_bounds, _waic_bounds
    rel = _relation(B)
    y = np.asarray(rel.data.values)
    assert _waic_bounds(rel) is None and WR.train_bounds("gauss", y) is None                       # Gaussian: the density
    pro = _relation(B, values=(y > 0).astype(float))
    B.setProbit(pro)
    assert _waic_bounds(pro) is None and WR.train_bounds("probit", pro.data.values) is None        # probit: the pairs' link
    # censored: an unflagged, a right- and a left-censored row
    c = np.zeros(40, dtype=np.int8)
    c[1::3], c[2::3] = 1, -1
    cen = _relation(B)
    B.setCensored(cen, c)
    b = _waic_bounds(cen)
    assert b.dtype == np.float64 and b.shape == (40, 2) and b.flags["C_CONTIGUOUS"]
    assert np.array_equal(b[0], [y[0], y[0]]) and np.array_equal(b[1], [y[1], INF]) and np.array_equal(b[2], [-INF, y[2]])
    assert np.array_equal(b, WR.train_bounds("censored", y, censor=c))
    # interval: as it stands, with an exact row, one-sided rows and the row that says nothing
    lo, hi = y - 0.3, y + 0.6
    lo[0], hi[0] = y[0], y[0]
    hi[1], lo[2] = INF, -INF
    lo[3], hi[3] = -INF, INF
    itv = _relation(B)
    B.setInterval(itv, lo, hi)
    b = _waic_bounds(itv)
    assert np.array_equal(b, np.stack([lo, hi], axis=1)) and np.array_equal(b, WR.train_bounds("interval", y, interval=itv.model.interval))
    assert b[0, 0] == b[0, 1] and np.array_equal(b[3], [-INF, INF])
    binned = _relation(B)
    B.setBinned(binned, [-0.5, 0.5])
    assert np.array_equal(_waic_bounds(binned), binned.model.interval) and np.isinf(_waic_bounds(binned)).any()
    # ordinal: the levels' bins between the edges k + 1/2, fixed or where every chain starts
    lev = np.random.default_rng(5).integers(1, 6, 40).astype(float)
    lev[:5] = [1, 2, 3, 4, 5]
    for sample_edges in (False, True):
        o = _relation(B, values=lev)
        B.setOrdinal(o, sample_edges=sample_edges)
        b = _waic_bounds(o)
        assert np.array_equal(b, _ordinal_bounds(o.model.ordinal_codes, np.arange(1, 5) + 0.5))
        assert np.array_equal(b, WR.train_bounds("ordinal", lev, codes=lev, edges=np.arange(1, 5) + 0.5))
        assert np.array_equal(b[:5], [[-INF, 1.5], [1.5, 2.5], [2.5, 3.5], [3.5, 4.5], [4.5, INF]])
    # this draw's edges
    b = WR.train_bounds("ordinal", lev, codes=lev, edges=[1.5, 1.9, 3.1, 4.5])
    assert np.array_equal(b[:5], [[-INF, 1.5], [1.5, 1.9], [1.9, 3.1], [3.1, 4.5], [4.5, INF]])
    # the relation's own checks run first: flags changed behind the setter's back are looked at again
    cen.model.censor = np.full(40, 2, dtype=np.int8)
    with pytest.raises(B.ArgumentError):
        _waic_bounds(cen)
    itv.model.interval = np.zeros((39, 2))
    with pytest.raises(B.ArgumentError):
        _waic_bounds(itv)


# ---- setWaic and the driver's refusals -----------------------------------------------------------------------------------------------
def test_setwaic_sets_the_model_and_refuses_what_is_no_switch(B):
    rel = _relation(B)
    assert rel.model.waic is None and B.RelationModel().waic is None
    assert B.setWaic(rel) is None and rel.model.waic == {"pointwise": False}
    B.setWaic(rel, pointwise=True)
    assert rel.model.waic == {"pointwise": True}
    B.setWaic(rel, on=False)
    assert rel.model.waic is None
    B.setWaic(rel, True, True)
    for bad in (dict(on=1), dict(on="yes"), dict(on=None), dict(pointwise=1), dict(pointwise="all"), dict(on=False, pointwise=True)):
        with pytest.raises(B.ArgumentError, match="setWaic"):
            B.setWaic(rel, **bad)
    assert rel.model.waic == {"pointwise": True}                    # a refused call changes nothing
    assert rel.model.alpha == 2.0 and rel.model.interval is None and rel.model.censor is None


def test_macau_refuses_waic_with_fewer_than_two_draws_and_with_more_than_one_rank(B):
    from bdf_amd.driver import macau
    rel = _relation(B)
    B.setWaic(rel)
    rd = B.RelationData(rel)
    for psamples in (0, 1):
        with pytest.raises(B.ArgumentError, match="psamples"):
            macau(rd, num_latent=2, burnin=1, psamples=psamples, verbose=False)

    class TwoRanks:                    # what an engine built with shard=(rank, 2) says of itself
        world, D = 2, 2

    with pytest.raises(B.ArgumentError, match="more than one rank"):
        macau(rd, num_latent=2, burnin=1, psamples=2, verbose=False, engine=TwoRanks(), reset_model=False)


def test_macau_signature_is_untouched():
    from bdf_amd.driver import macau
    params = list(inspect.signature(macau).parameters.values())
    assert len(params) == 24 and params[-1].name == "lpd" and params[-1].default is False


# ---- the quality record ---------------------------------------------------------------------------------------------------------------
def test_recorded_quality_gaps_are_what_the_restatement_computes():
    """the gaps (D = 3) - (D = 1) of the elpd per training cell and of the held-out LPD on the planted data, seed 2 of the three
    recorded ones, recomputed; all three records agree in sign, and most cells have V < 0.4"""
    e3, l3, h3 = WR.quality_fit(3, WR.QUALITY_SEEDS[0])
    e1, l1, h1 = WR.quality_fit(1, WR.QUALITY_SEEDS[0])
    assert abs((e3 - e1) - WR.QUALITY_ELPD_GAPS[0]) <= 5e-5 and abs((l3 - l1) - WR.QUALITY_LPD_GAPS[0]) <= 5e-5
    assert min(WR.QUALITY_ELPD_GAPS) > 0.0 and min(WR.QUALITY_LPD_GAPS) > 0.0
    assert h3 < 0.5 and h1 < 0.5


# ---- the resource listing ---------------------------------------------------------------------------------------------------------
# (VGPRs, scratch bytes per lane, waves per SIMD) of the nine shapes <modes, vector width, row pieces> of k_waic, as DESIGN.md
# section 17 prints them
WAIC_KERNELS = {
    "6k_waicILi2ELi1ELi1EEEvNS_8WaicArgsE": (41, 0, 7),
    "6k_waicILi2ELi4ELi1EEEvNS_8WaicArgsE": (89, 0, 5),
    "6k_waicILi2ELi4ELi2EEEvNS_8WaicArgsE": (91, 0, 5),
    "6k_waicILi3ELi1ELi1EEEvNS_8WaicArgsE": (42, 0, 7),
    "6k_waicILi3ELi4ELi1EEEvNS_8WaicArgsE": (122, 0, 4),
    "6k_waicILi3ELi4ELi2EEEvNS_8WaicArgsE": (124, 0, 4),
    "6k_waicILi4ELi1ELi1EEEvNS_8WaicArgsE": (46, 0, 7),
    "6k_waicILi4ELi4ELi1EEEvNS_8WaicArgsE": (91, 0, 5),
    "6k_waicILi4ELi4ELi2EEEvNS_8WaicArgsE": (162, 0, 3),
}


def test_waic_kernels_use_no_scratch_only_the_reduction_lds_and_keep_k_lpd_s_occupancy():
    res = _resources("k_waic")
    shapes = {k: v for k, v in res.items() if "k_waicI" in k}
    assert shapes == WAIC_KERNELS
    lpd = {re.search(r"ILi\dELi\dELi\dE", k).group(0): v for k, v in _resources("k_lpd").items() if "k_lpdI" in k}
    assert len(lpd) == 9
    for k, (vgprs, scratch, waves) in shapes.items():
        assert scratch == 0, k
        assert waves >= lpd[re.search(r"ILi\dELi\dELi\dE", k).group(0)][2] - 1, (k, waves)
    for k, v in res.items():                                        # the nine shapes, the read-out and the fixed-order sum
        assert v[1] == 0 and v[2] >= 2, (k, v)
    assert len(res) == 11
    text = open(os.path.join(ROOT, "bayesiandatafusion.jl_amd", "csrc", "k_waic.o.res")).read()
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", text)]
    assert lds == [128] * 11                                        # 4 statistics x 4 waves of doubles, nothing else
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("## 17."):]
    for k, (vgprs, scratch, waves) in WAIC_KERNELS.items():
        nm, vec, nc = re.search(r"ILi(\d)ELi(\d)ELi(\d)E", k).groups()
        assert re.search(rf"\|\s*{nm}\s*\|\s*{vec}\s*\|\s*{nc}\s*\|\s*{vgprs}\s*\|\s*{scratch}\s*\|\s*128\s*\|\s*{waves}\s*\|", section), k
