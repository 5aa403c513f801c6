"""The held-out log predictive density on the host (no GPU): the restated maps of tests/lpd_restatement.py against a 50-digit
evaluation, csrc/lpd.h compiled for the host against the restatement, the maps' finiteness far out, the streaming log-sum-exp against
scipy's logsumexp, setTestInterval / setTestBinned and what they guard, and the resource listing the build leaves for k_lpd."""
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
from scipy.special import logsumexp

import lpd_restatement as LR
from test_probit_host import _resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.inf
ALPHAS = (0.04, 5.0, 900.0)


# ---- the restated maps against 50 digits ------------------------------------------------------------------------------------------
def _mpf(x):
    from mpmath import mp, mpf
    return mpf(float(x)) if np.isfinite(x) else (mp.inf if x > 0 else -mp.inf)


def _exact_log_phi(x):
    from mpmath import mp
    with mp.workdps(50):
        return float(mp.log(mp.ncdf(_mpf(x))))


def _exact_log_mass(a, b):
    """log(Phi(b) - Phi(a)) from the doubles as they are; taken in the lower tail, where 50 digits hold the difference"""
    from mpmath import mp
    with mp.workdps(50):
        a, b = _mpf(a), _mpf(b)
        if a + b > 0:
            a, b = -b, -a
        return float(mp.log(mp.ncdf(b) - mp.ncdf(a)))


def test_maps_match_a_50_digit_evaluation():
    """The grids: log Phi on 3,000 points of [-60, 10] and the switch points 0 and -37 with their neighbours; the log mass with the
    standardised lower bound uniform in [-50, 50], 1,500 points each, for two-sided intervals of width 1e-3 ... 16 (log-uniform),
    for one-sided intervals on either side, and for narrow ones of width 1e-6 ... 1e-3.  Measured (absolute, printed with -s):
    log Phi 2.3e-13 (5.4e-16 relative to |log Phi|: half an ulp of a number of size 1,800), two-sided 4.3e-12, one-sided 2.3e-13,
    narrow 4.4e-9 -- the last is the cancellation in Phi(b) - Phi(a) of an interval a millionth of a standard deviation wide near
    the centre (the difference is 4e-7 of two numbers good to 1e-16), which belongs to the form itself; deep in the tail, where
    the difference of the two logarithms is formed analytically, the narrow intervals are good to 1e-12.  The bounds are ten times
    the measured figures."""
    below, above = np.nextafter(-37.0, -INF), np.nextafter(-37.0, 0.0)
    xs = np.concatenate([np.linspace(-60.0, 10.0, 3000), [-37.0, below, above, 0.0, -0.0, np.nextafter(0.0, -1.0), 1e-300]])
    got = LR.log_phi(xs)
    ex = np.array([_exact_log_phi(x) for x in xs])
    e_abs, e_rel = np.abs(got - ex).max(), (np.abs(got - ex) / np.maximum(1.0, np.abs(ex))).max()
    print(f"log Phi: worst absolute error {e_abs:.2e}, relative to max(1, |log Phi|) {e_rel:.2e}")
    assert e_abs <= 2.3e-12 and e_rel <= 5.5e-15
    rng = np.random.default_rng(1)
    worst = {}
    for name, (w_lo, w_hi) in (("two-sided", (-3.0, np.log10(16.0))), ("narrow", (-6.0, -3.0))):
        a, w = rng.uniform(-50.0, 50.0, 1500), 10.0 ** rng.uniform(w_lo, w_hi, 1500)
        got = LR.lpd_mass(0.0, a, a + w, 1.0)
        assert np.all(np.isfinite(got)) and np.all(got < 0.0)
        worst[name] = max(abs(g - _exact_log_mass(x, x + y)) for g, x, y in zip(got, a, w))
        if name == "narrow":          # where both logarithms are asymptotic the narrow intervals lose nothing
            deep = a + w <= -37.0
            deep |= a >= 37.0
            worst["narrow, beyond 37 sd"] = max(abs(g - _exact_log_mass(x, x + y)) for g, x, y in zip(got[deep], a[deep], w[deep]))
    a = rng.uniform(-50.0, 50.0, 1500)
    right, left = LR.lpd_mass(0.0, a, INF, 1.0), LR.lpd_mass(0.0, -INF, a, 1.0)
    worst["one-sided"] = max(max(abs(g - _exact_log_mass(x, INF)) for g, x in zip(right, a)),
                             max(abs(g - _exact_log_mass(-INF, x)) for g, x in zip(left, a)))
    print("log mass, worst absolute error: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert worst["two-sided"] <= 4.4e-11 and worst["one-sided"] <= 2.3e-12 and worst["narrow"] <= 4.4e-8
    assert worst["narrow, beyond 37 sd"] <= 1e-11
    assert float(LR.lpd_mass(0.3, -INF, INF, 2.0)) == 0.0              # the row that says nothing has mass 1
    # the density and the 0/1 map are what they say
    from mpmath import mp, mpf
    with mp.workdps(50):
        for y, m, al in ((0.3, -1.2, 0.04), (5.0, 4.0, 900.0), (-40.0, 0.5, 5.0)):
            ex = mp.log(mpf(al) / (2 * mp.pi)) / 2 - mpf(al) * (mpf(y) - mpf(m)) ** 2 / 2
            assert abs(float(LR.lpd_gauss(y, m, al)) - float(ex)) <= 1e-15 * max(1.0, abs(float(ex))) * 4
    assert np.array_equal(LR.lpd_probit([1.0, 0.0, 1.0], [0.7, 0.7, -45.0]), LR.log_phi([0.7, -0.7, -45.0]))


# ---- the header against the restatement -------------------------------------------------------------------------------------------
def _compile_and_run(lines):
    """csrc/lpd.h compiled for the host where a C++ compiler is at hand (csrc/Makefile's, as a host compiler, when there is no
    other); lines of "kind y m lo hi alpha" -> the values the header's maps give (kind 0 density, 1 probit, 2 mass, 3 log Phi(m))"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cxx = [shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")]
    if cxx[0] is None:
        cxx = [hipcc, "-x", "c++"]
    src = r'''
        #include <cstdio>
        #include "lpd.h"
        int main() { int k; double y, m, lo, hi, al; while (scanf("%d %lf %lf %lf %lf %lf", &k, &y, &m, &lo, &hi, &al) == 6)
                         printf("%.17g\n", k == 0 ? bdf_lpd_gauss(y, m, al) : k == 1 ? bdf_lpd_probit(y, m) : k == 2 ? bdf_lpd_mass(m, lo, hi, al)
                                                                                                              : bdf_log_phi(m)); return 0; }
    '''
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "t.cpp"), "w").write(src)
        subprocess.run(cxx + ["-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "bayesiandatafusion.jl_amd", "csrc"), os.path.join(td, "t.cpp"),
                        "-o", os.path.join(td, "t")], check=True)
        text = "".join("%d %.17g %.17g %.17g %.17g %.17g\n" % t for t in lines)
        out = subprocess.run([os.path.join(td, "t")], input=text, capture_output=True, text=True, check=True).stdout
    return np.array([float(t) for t in out.split()])


def test_header_and_restatement_state_the_same_maps():
    """4,000 points, the predictive mean out to 45 standard deviations from the record on either side, widths from 1e-3 standard
    deviations, alpha in {0.04, 5, 900}: 1,000 each of the density, the 0/1 map, the mass (an eighth each right-open and left-open,
    some (-inf, +inf)) and log Phi itself.  The same formulas on two erfc implementations: 1e-12 relative to max(1, |l|)."""
    rng = np.random.default_rng(2)
    n = 1000
    alpha = np.repeat(ALPHAS, n // 3 + 1)[:n]
    ra = np.sqrt(alpha)
    m = rng.standard_normal(n)
    a, w = rng.uniform(-45.0, 45.0, n), 10.0 ** rng.uniform(-3.0, 2.0, n)
    a[::3] = rng.uniform(-8.0, 8.0, len(a[::3]))
    lo, hi = m + a / ra, m + (a + w) / ra
    lo[5::8], hi[7::8] = -INF, INF
    lo[11::50], hi[11::50] = -INF, INF
    y = m + a / ra
    x = np.concatenate([rng.uniform(-45.0, 45.0, n - 8), [-37.0, np.nextafter(-37.0, 0.0), np.nextafter(-37.0, -INF), 0.0, -0.0, 8.3, -38.2, 37.0]])
    lines = [(0, y[k], m[k], 0.0, 0.0, alpha[k]) for k in range(n)] + [(1, float(k & 1), x[k], 0.0, 0.0, 1.0) for k in range(n)]
    lines += [(2, 0.0, m[k], lo[k], hi[k], alpha[k]) for k in range(n)] + [(3, 0.0, x[k], 0.0, 0.0, 1.0) for k in range(n)]
    got = _compile_and_run(lines)
    ref = np.concatenate([LR.lpd_gauss(y, m, alpha), LR.lpd_probit((np.arange(n) & 1).astype(float), x), LR.lpd_mass(m, lo, hi, alpha), LR.log_phi(x)])
    assert len(got) == 4 * n and np.all(np.isfinite(got)) and np.all(np.isfinite(ref))
    err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    print(f"lpd.h against the restatement: worst error relative to max(1, |l|) {err.max():.2e} (density {err[:n].max():.1e}, 0/1 "
          f"{err[n:2 * n].max():.1e}, mass {err[2 * n:3 * n].max():.1e}, log Phi {err[3 * n:].max():.1e})")
    assert err.max() <= 1e-12


def test_maps_are_finite_everywhere():
    """standardised bounds out to +-50 (and +-1e4 for the one-sided and the 0/1 map), widths 1e-6 ... inf, alpha in {0.04, 5, 900},
    the restatement and the header: no -inf, no NaN, and never a positive log of a probability"""
    a = np.linspace(-50.0, 50.0, 401)
    lines = []
    for alpha in ALPHAS:
        ra = np.sqrt(alpha)
        for w in (1e-6, 1e-3, 0.3, 4.0, 60.0, INF):
            for m in (0.0, -3.25):
                lo, hi = m + a / ra, m + (a + w) / ra
                for lo_, hi_ in ((lo, hi), (np.full_like(lo, -INF), hi)):
                    got = LR.lpd_mass(m, lo_, hi_, alpha)
                    assert np.all(np.isfinite(got)) and np.all(got <= 0.0), (alpha, w, m)
                    lines += [(2, 0.0, m, lo_[k], hi_[k], alpha) for k in range(0, len(a), 8)]
    far = np.array([-1e4, -50.0, -38.6, -37.0, 0.0, 37.0, 50.0, 1e4])
    assert np.all(np.isfinite(LR.log_phi(far))) and np.all(LR.log_phi(far) <= 0.0)
    assert np.all(np.isfinite(LR.lpd_mass(0.0, far, INF, 1.0))) and np.all(np.isfinite(LR.lpd_mass(0.0, -INF, far, 1.0)))
    lines += [(3, 0.0, t, 0.0, 0.0, 1.0) for t in far] + [(1, 1.0, t, 0.0, 0.0, 1.0) for t in far] + [(2, 0.0, 0.0, -INF, INF, 5.0)]
    got = _compile_and_run(lines)
    assert len(got) == len(lines) and np.all(np.isfinite(got)) and np.all(got <= 0.0)
    assert got[-1] == 0.0


# ---- the streaming log-sum-exp ------------------------------------------------------------------------------------------------------
def test_streaming_logsumexp_matches_scipy_in_any_order():
    """40 draws whose log-likelihoods span -2,000 ... -1 for each of 300 cells; the stream in five orders (as drawn, reversed,
    ascending, descending, shuffled) against log(mean(exp(l))) from scipy.special.logsumexp, to 1e-12; burn-in draws before the
    first posterior one leave no trace"""
    rng = np.random.default_rng(3)
    S, n = 40, 300
    l = rng.uniform(-2000.0, -1.0, (S, n))
    l[0, :5], l[-1, :5] = -2000.0, -1.0                              # the whole span in one cell
    l[:, 5] = -700.0                                                 # every draw the same
    l[:, 6] = np.linspace(-1.0 - 1e-9, -1.0, S)                      # every draw counts
    ref = logsumexp(l, axis=0) - np.log(S)
    orders = [np.arange(S), np.arange(S)[::-1], np.argsort(l[:, 0]), np.argsort(-l[:, 0]), rng.permutation(S)]
    for order in orders:
        st = LR.Stream()
        assert np.array_equal(st.update(l[3] - 5.0, 0), l[3] - 5.0) and st.draws == 0 and st.M is None       # burn-in: no state
        for k, s in enumerate(order):
            lpd = st.update(l[s], 1 if k == 0 else 2)
            assert np.abs(lpd - (logsumexp(l[order[:k + 1]], axis=0) - np.log(k + 1))).max() <= 1e-12
        assert st.draws == S and np.abs(st.lpd() - ref).max() <= 1e-12
    assert np.abs(ref[5] + 700.0) <= 1e-12 and np.all(ref <= l.max(axis=0)) and np.all(ref >= l.max(axis=0) - np.log(S))
    st.update(l[7], 1)                                               # a first draw starts over
    assert st.draws == 1 and np.array_equal(st.lpd(), l[7])


# ---- the setters ----------------------------------------------------------------------------------------------------------------------
def _relation(B, n=40, test=None, values=None, alpha=2.0):
    rng = np.random.default_rng(3)
    ids = np.stack([rng.integers(1, 9, n), rng.integers(1, 7, n)], axis=1)
    y = rng.standard_normal(n) if values is None else np.asarray(values, dtype=np.float64)
    rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "ratings", [B.Entity("u"), B.Entity("v")], alpha=alpha, dims=[8, 6])
    if test is not None:
        B.assignToTest(rel, test)
    return rel


def _test_bounds(rel, seed=5):
    rng = np.random.default_rng(seed)
    y = np.asarray(rel.test_vec.values)
    pick = rng.random(len(y))
    lo = np.where(pick < 0.6, y - rng.uniform(0.1, 1.0, len(y)), y)
    hi = np.where(pick < 0.6, y + rng.uniform(0.1, 1.0, len(y)), y)
    lo[(pick >= 0.3) & (pick < 0.4)] = -INF
    hi[(pick >= 0.4) & (pick < 0.5)] = INF
    return lo, hi


def test_settestinterval_stores_one_float64_array_per_test_row(B):
    assert _relation(B).model.test_interval is None and B.RelationModel().test_interval is None
    rel = _relation(B, test=np.arange(1, 13))
    lo, hi = _test_bounds(rel)
    assert B.setTestInterval(rel, lo, hi) is None
    b = rel.model.test_interval
    assert b.dtype == np.float64 and b.shape == (12, 2) and b.flags["C_CONTIGUOUS"]
    assert np.array_equal(b[:, 0], lo) and np.array_equal(b[:, 1], hi) and np.isinf(b).any() and np.any(lo == hi)
    assert rel.model.interval is None and rel.model.alpha == 2.0                  # the training side is left alone
    y = np.asarray(rel.test_vec.values)
    B.setTestInterval(rel, list(y), list(y))                                       # lists work; lower = upper: every cell exact
    assert np.array_equal(rel.model.test_interval, np.stack([y, y], axis=1))
    B.setTestInterval(rel, y, np.full(12, INF))                                    # a censored test record: one infinite bound
    B.setTestInterval(rel, np.full(12, -INF), np.full(12, INF))
    B.setInterval(rel, rel.data.values, rel.data.values)                           # training bounds beside test bounds
    assert len(rel.model.interval) == 28 and len(rel.model.test_interval) == 12
    rel.model.alpha_sample = True
    B.setTestInterval(rel, lo, hi)


def test_settestinterval_refuses_nan_a_wrong_length_crossed_bounds_a_value_outside_and_probit(B):
    rel = _relation(B, test=np.arange(1, 13))
    lo, hi = _test_bounds(rel)
    y = np.asarray(rel.test_vec.values)

    def changed(a, k, v):
        a = a.copy()
        a[k] = v
        return a

    for bad_lo, bad_hi in ((changed(lo, 3, np.nan), hi), (lo, changed(hi, 4, np.nan)), (lo[:-1], hi[:-1]), (np.append(lo, 0.0), np.append(hi, 1.0)),
                           (lo, hi[:-1]), (lo.reshape(-1, 1), hi.reshape(-1, 1)), (changed(lo, 0, y[0] + 2.0), changed(hi, 0, y[0] + 1.0)),
                           (changed(lo, 7, y[7] + 0.5), changed(hi, 7, y[7] + 1.5)), (changed(lo, 8, y[8] - 1.5), changed(hi, 8, y[8] - 0.5)),
                           (changed(lo, 9, INF), changed(hi, 9, INF)), (changed(lo, 9, -INF), changed(hi, 9, -INF)),
                           (np.zeros(28), np.ones(28)), (["a"] * 12, hi)):                       # (28: the training rows' count)
        with pytest.raises(B.ArgumentError):
            B.setTestInterval(rel, bad_lo, bad_hi)
    assert rel.model.test_interval is None
    B.setTestInterval(rel, changed(lo, 2, y[2]), changed(hi, 2, y[2] + 1.0))      # the value may sit on a bound
    B.setTestInterval(rel, changed(lo, 2, y[2] - 1.0), changed(hi, 2, y[2]))
    with pytest.raises(B.ArgumentError):                                           # no test rows: only empty bounds fit
        B.setTestInterval(_relation(B), lo, hi)
    vals = (np.arange(40) % 2).astype(np.float64)
    rel = _relation(B, test=np.arange(1, 13), values=vals)
    B.setProbit(rel)
    t = np.asarray(rel.test_vec.values)
    with pytest.raises(B.ArgumentError, match="setProbit"):
        B.setTestInterval(rel, t - 0.5, t + 0.5)
    with pytest.raises(B.ArgumentError, match="setProbit"):
        B.setTestBinned(rel, [0.5])
    assert rel.model.test_interval is None


def test_settestbinned_follows_setbinned_edge_rule(B):
    import interval_restatement as IR
    below = np.nextafter(2.5, -INF)
    vals = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 1.5, below, 2.5, 4.5, -7.0, 99.0, 1.4999])
    rel = _relation(B, values=np.arange(40) % 5 + 1.0)
    B.setTest(rel, {"u": np.arange(12) % 8 + 1, "v": np.arange(12) % 6 + 1, "y": vals[:12]})
    assert B.setTestBinned(rel, [1.5, 2.5, 3.5, 4.5]) is None
    expect = np.array([[-INF, 1.5], [1.5, 2.5], [2.5, 3.5], [3.5, 4.5], [4.5, INF], [1.5, 2.5], [1.5, 2.5], [2.5, 3.5], [4.5, INF],
                       [-INF, 1.5], [4.5, INF], [-INF, 1.5]])
    assert np.array_equal(rel.test_vec.values, vals)                               # setTest keeps the table's order
    assert np.array_equal(rel.model.test_interval, expect)                        # exactly: e_j <= v < e_{j+1}
    assert np.array_equal(rel.model.test_interval, IR.bin_bounds(rel.test_vec.values, [1.5, 2.5, 3.5, 4.5]))
    B.setBinned(rel, [1.5, 2.5, 3.5, 4.5])                                         # the same rule on the training side
    assert np.array_equal(rel.model.interval, IR.bin_bounds(rel.data.values, [1.5, 2.5, 3.5, 4.5]))
    B.setTestBinned(rel, [3.0])                                                    # one interior edge: two open bins
    assert np.array_equal(rel.model.test_interval[:, 0], np.where(vals >= 3.0, 3.0, -INF))
    for bad in ([], [1.0, 1.0], [2.0, 1.0], [1.0, np.nan], [-INF, 0.0], [0.0, INF], [[0.0, 1.0]]):
        with pytest.raises(B.ArgumentError):
            B.setTestBinned(rel, bad)
    assert rel.model.test_interval.shape == (12, 2)


def test_settest_and_assigntotest_drop_the_test_bounds(B):
    rel = _relation(B, test=np.arange(1, 13))
    B.setTestInterval(rel, *_test_bounds(rel))
    B.setTest(rel, {"u": [1, 2, 3], "v": [1, 1, 2], "y": [0.1, 1.0, -1.0]})       # a new test table: the old bounds say nothing about it
    assert rel.model.test_interval is None and len(rel.test_vec) == 3
    B.setTestInterval(rel, [0.0, 1.0, -INF], [0.5, 1.0, INF])
    B.assignToTest(rel, np.arange(1, 6))
    assert rel.model.test_interval is None and len(rel.test_vec) == 5
    B.setTestBinned(rel, [0.0])
    assert rel.model.test_interval.shape == (5, 2)


def test_the_bounds_are_looked_at_again_when_they_are_used(B):
    from bdf_amd.relation_data import check_test_interval
    rel = _relation(B, test=np.arange(1, 13))
    lo, hi = _test_bounds(rel)
    B.setTestInterval(rel, lo, hi)
    keep = rel.model.test_interval
    check_test_interval(rel)
    assert np.array_equal(rel.model.test_interval, keep)
    for wrong in (keep[:-1], keep[:, 0], keep[:, ::-1] + np.array([1.0, -1.0])):
        rel.model.test_interval = wrong
        with pytest.raises(B.ArgumentError):
            check_test_interval(rel)
    rel.model.test_interval = keep.copy()
    rel.model.test_interval[3, 1] = np.nan
    with pytest.raises(B.ArgumentError):
        check_test_interval(rel)


def test_macau_has_the_lpd_keyword_last(B):
    import inspect
    from bdf_amd.driver import macau
    params = list(inspect.signature(macau).parameters.values())
    assert params[-1].name == "lpd" and params[-1].default is False


# ---- the resource listing ---------------------------------------------------------------------------------------------------------
# (VGPRs, scratch bytes per lane, waves per SIMD) of the nine shapes <modes, vector width, row pieces> of k_lpd, as DESIGN.md
# section 15 prints them
LPD_KERNELS = {
    "5k_lpdILi2ELi1ELi1EEEvNS_7LpdArgsE": (46, 0, 7),
    "5k_lpdILi2ELi4ELi1EEEvNS_7LpdArgsE": (94, 0, 5),
    "5k_lpdILi2ELi4ELi2EEEvNS_7LpdArgsE": (96, 0, 5),
    "5k_lpdILi3ELi1ELi1EEEvNS_7LpdArgsE": (46, 0, 7),
    "5k_lpdILi3ELi4ELi1EEEvNS_7LpdArgsE": (127, 0, 4),
    "5k_lpdILi3ELi4ELi2EEEvNS_7LpdArgsE": (129, 0, 3),
    "5k_lpdILi4ELi1ELi1EEEvNS_7LpdArgsE": (52, 0, 7),
    "5k_lpdILi4ELi4ELi1EEEvNS_7LpdArgsE": (96, 0, 5),
    "5k_lpdILi4ELi4ELi2EEEvNS_7LpdArgsE": (162, 0, 3),
}


def test_lpd_kernels_use_no_scratch_and_only_the_reduction_lds():
    res = _resources("k_lpd")
    shapes = {k: v for k, v in res.items() if "k_lpdI" in k}
    assert shapes == LPD_KERNELS
    for k, v in res.items():                                        # the nine shapes, the read-out and the fixed-order sum
        assert v[1] == 0 and v[2] >= 2, (k, v)
    assert len(res) == 11
    path = os.path.join(ROOT, "bayesiandatafusion.jl_amd", "csrc", "k_lpd.o.res")
    text = open(path).read()
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", text)]
    assert sorted(lds) == [0] + [128] * 10                          # 4 statistics x 4 waves of doubles, nothing else
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for k, (vgprs, scratch, waves) in LPD_KERNELS.items():
        nm, vec, nc = re.search(r"ILi(\d)ELi(\d)ELi(\d)E", k).groups()
        assert re.search(rf"\|\s*{nm}\s*\|\s*{vec}\s*\|\s*{nc}\s*\|\s*{vgprs}\s*\|\s*{scratch}\s*\|\s*128\s*\|\s*{waves}\s*\|", design), k
