"""The interval-censored noise model on the host (no GPU): setInterval / setBinned and what they guard, the restated draw map of
tests/interval_restatement.py against a 40-digit inversion and scipy's truncated-normal mean, its Philox uniforms against the
oracle, and the resource listing the build leaves for the new kernels."""
import os
import re

import numpy as np
import pytest
from scipy.stats import truncnorm

import interval_restatement as IR
from test_probit_host import _resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.inf


def _relation(B, n=40, test=None, alpha=2.0, values=None):
    rng = np.random.default_rng(3)
    ids = np.stack([rng.integers(1, 9, n), rng.integers(1, 7, n)], axis=1)
    y = rng.standard_normal(n) if values is None else np.asarray(values, dtype=np.float64)
    rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "ratings", [B.Entity("u"), B.Entity("v")], alpha=alpha, dims=[8, 6])
    if test is not None:
        B.assignToTest(rel, test)
    return rel


def _bounds(rel, seed=5):
    """legal bounds around the relation's training values: a third two-sided, some open on one side or both, the rest exact"""
    rng = np.random.default_rng(seed)
    y = np.asarray(rel.data.values)
    pick = rng.random(len(y))
    lo = np.where(pick < 0.5, y - rng.uniform(0.1, 1.0, len(y)), y)
    hi = np.where(pick < 0.5, y + rng.uniform(0.1, 1.0, len(y)), y)
    lo[(pick >= 0.3) & (pick < 0.4)] = -INF
    hi[(pick >= 0.4) & (pick < 0.5)] = INF
    lo[pick >= 0.9], hi[pick >= 0.9] = -INF, INF
    return lo, hi


# ---- setInterval --------------------------------------------------------------------------------------------------------------
def test_default_has_no_bounds(B):
    assert _relation(B).model.interval is None and B.RelationModel().interval is None


def test_setinterval_stores_one_float64_array_and_resets_the_device_state(B):
    rel = _relation(B, test=np.arange(1, 11))
    rel._dev = object()
    lo, hi = _bounds(rel)
    assert B.setInterval(rel, lo, hi) is None
    b = rel.model.interval
    assert b.dtype == np.float64 and b.shape == (30, 2) and b.flags["C_CONTIGUOUS"] and rel._dev is None
    assert np.array_equal(b[:, 0], lo) and np.array_equal(b[:, 1], hi)
    assert np.isinf(b).any() and np.any((b[:, 0] == -INF) & (b[:, 1] == INF))      # open sides and "says nothing" rows are legal
    assert rel.model.alpha == 2.0 and rel.model.alpha_sample is False and rel.model.probit is False and rel.model.censor is None
    y = np.asarray(rel.data.values)
    B.setInterval(rel, list(y), list(y))                           # lists work; the bounds are replaced: every row exact
    assert np.array_equal(rel.model.interval, np.stack([y, y], axis=1))
    B.setPrecision(rel, 3.0)                                       # the precision stays a parameter
    rel.model.alpha_sample = True
    assert rel.model.alpha == 3.0 and rel.model.interval is not None


def test_setinterval_refuses_nan_a_wrong_length_crossed_bounds_and_a_value_outside(B):
    rel = _relation(B, test=np.arange(1, 11))
    lo, hi = _bounds(rel)
    y = np.asarray(rel.data.values)

    def changed(a, k, v):
        a = a.copy()
        a[k] = v
        return a

    for bad_lo, bad_hi in ((changed(lo, 3, np.nan), hi), (lo, changed(hi, 4, np.nan)), (lo[:-1], hi[:-1]), (np.append(lo, 0.0), np.append(hi, 1.0)),
                           (lo, hi[:-1]), (lo.reshape(-1, 1), hi.reshape(-1, 1)), (changed(lo, 0, y[0] + 2.0), changed(hi, 0, y[0] + 1.0)),
                           (changed(lo, 7, y[7] + 0.5), changed(hi, 7, y[7] + 1.5)), (changed(lo, 8, y[8] - 1.5), changed(hi, 8, y[8] - 0.5)),
                           (changed(lo, 9, INF), changed(hi, 9, INF)), (changed(lo, 9, -INF), changed(hi, 9, -INF))):
        with pytest.raises(B.ArgumentError):
            B.setInterval(rel, bad_lo, bad_hi)
    assert rel.model.interval is None
    B.setInterval(rel, changed(lo, 2, y[2]), changed(hi, 2, y[2] + 1.0))      # the value may sit on a bound
    B.setInterval(rel, changed(lo, 2, y[2] - 1.0), changed(hi, 2, y[2]))


def test_order_relative_to_the_test_split(B):
    rel = _relation(B)
    B.setInterval(rel, *_bounds(rel))
    with pytest.raises(B.ArgumentError, match="assignToTest before setInterval"):
        B.assignToTest(rel, np.arange(1, 11))
    assert rel.data.nnz() == 40 and len(rel.test_vec) == 0         # nothing was split off
    B.setTest(rel, {"u": [1, 2, 3], "v": [1, 1, 2], "y": [0.1, 1.0, -1.0]})     # setTest leaves the training rows alone
    assert len(rel.test_vec) == 3 and len(rel.model.interval) == 40
    rel2 = _relation(B)
    B.setTest(rel2, {"u": [1, 2, 3], "v": [1, 1, 2], "y": [0.1, 1.0, -1.0]})
    B.setInterval(rel2, *_bounds(rel2))
    assert len(rel2.model.interval) == 40
    rel3 = _relation(B, test=np.arange(1, 11))                     # the documented order
    B.setInterval(rel3, *_bounds(rel3))
    rel4 = _relation(B, values=np.arange(40) % 5 + 1.0)
    B.setBinned(rel4, [1.5, 2.5, 3.5, 4.5])
    with pytest.raises(B.ArgumentError, match="assignToTest before"):
        B.assignToTest(rel4, 5)


# ---- setBinned ----------------------------------------------------------------------------------------------------------------
def test_setbinned_gives_every_row_its_bin_and_an_edge_belongs_to_the_bin_above(B):
    below = np.nextafter(2.5, -INF)
    vals = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 1.5, below, 2.5, 4.5, -7.0, 99.0, 1.4999])
    rel = _relation(B, n=len(vals), values=vals)
    rel._dev = object()
    assert B.setBinned(rel, [1.5, 2.5, 3.5, 4.5]) is None and rel._dev is None
    expect = np.array([[-INF, 1.5], [1.5, 2.5], [2.5, 3.5], [3.5, 4.5], [4.5, INF], [1.5, 2.5], [1.5, 2.5], [2.5, 3.5], [4.5, INF],
                       [-INF, 1.5], [4.5, INF], [-INF, 1.5]])
    order = [int(np.flatnonzero(vals == v)[0]) for v in rel.data.values]       # the relation keeps its own row order
    assert np.array_equal(rel.model.interval, expect[order])                  # exactly: e_j <= v < e_{j+1}
    assert np.array_equal(rel.model.interval, IR.bin_bounds(rel.data.values, [1.5, 2.5, 3.5, 4.5]))
    B.setBinned(rel, [3.0])                                        # one interior edge: two open bins
    assert np.array_equal(rel.model.interval[:, 0], np.where(np.asarray(rel.data.values) >= 3.0, 3.0, -INF))
    assert np.array_equal(rel.model.interval[:, 1], np.where(np.asarray(rel.data.values) >= 3.0, INF, 3.0))
    assert B.toStr(rel) == "rati[α=2.0 intv:12]"


def test_setbinned_refuses_edges_that_are_not_finite_and_strictly_increasing(B):
    rel = _relation(B)
    for bad in ([], [1.0, 1.0], [2.0, 1.0], [1.0, np.nan], [-INF, 0.0], [0.0, INF], [[0.0, 1.0]]):
        with pytest.raises(B.ArgumentError):
            B.setBinned(rel, bad)
    assert rel.model.interval is None


# ---- what excludes what ---------------------------------------------------------------------------------------------------------
def test_interval_censoring_probit_and_features_exclude_each_other(B):
    rel = _relation(B)
    rel.F = np.ones((40, 2))
    with pytest.raises(B.ArgumentError, match="features"):
        B.setInterval(rel, *_bounds(rel))
    vals = (np.arange(40) % 2).astype(np.float64)

    def binary():
        return _relation(B, values=vals)

    rel = binary()
    B.setProbit(rel)
    with pytest.raises(B.ArgumentError, match=r"(?s)setProbit.*setInterval|setInterval.*setProbit"):
        B.setInterval(rel, vals - 0.5, vals + 0.5)
    with pytest.raises(B.ArgumentError):
        B.setBinned(rel, [0.5])
    assert rel.model.interval is None
    rel = binary()
    B.setInterval(rel, vals - 0.5, vals + 0.5)
    with pytest.raises(B.ArgumentError, match=r"(?s)setProbit.*setInterval|setInterval.*setProbit"):
        B.setProbit(rel)
    assert rel.model.probit is False
    with pytest.raises(B.ArgumentError, match=r"(?s)setCensored.*setInterval|setInterval.*setCensored"):
        B.setCensored(rel, np.zeros(40, dtype=int))
    assert rel.model.censor is None
    rel = binary()
    B.setCensored(rel, np.zeros(40, dtype=int))
    with pytest.raises(B.ArgumentError, match=r"(?s)setCensored.*setInterval|setInterval.*setCensored"):
        B.setInterval(rel, vals - 0.5, vals + 0.5)
    assert rel.model.interval is None


def test_samplers_refuse_what_the_interval_model_does_not_cover(B):
    rel = _relation(B, test=np.arange(1, 6))
    B.setInterval(rel, *_bounds(rel))
    rd = B.RelationData(rel)
    with pytest.raises(B.ArgumentError):
        B.bpmf_vb(rd, num_latent=4, verbose=False, niter=1)
    with pytest.raises(B.ArgumentError):
        B.macau_hmc(rd, num_latent=4, verbose=False, burnin=1, psamples=1)
    with pytest.raises(B.ArgumentError):
        B.GibbsEngine(rd, 4, shard=(0, 2))
    with pytest.raises(B.ArgumentError):
        B.macau(rd, num_latent=4, burnin=1, psamples=1, verbose=False, rmse_train=True)
    # changed behind setInterval's back: the engine looks again (check_interval)
    from bdf_amd.relation_data import check_interval
    keep = rel.model.interval
    rel.model.interval = keep[:-1]
    with pytest.raises(B.ArgumentError):
        B.GibbsEngine(rd, 4)
    for k, v in ((0, np.nan), (1, np.nan)):
        rel.model.interval = keep.copy()
        rel.model.interval[3, k] = v
        with pytest.raises(B.ArgumentError):
            check_interval(rel)
    rel.model.interval = keep[:, ::-1] + np.array([1.0, -1.0])       # lower above upper
    with pytest.raises(B.ArgumentError):
        check_interval(rel)
    rel.model.interval = keep[:, 0]                                 # not (n, 2)
    with pytest.raises(B.ArgumentError):
        check_interval(rel)
    rel.model.interval = keep
    rel.F = np.ones((35, 2))
    with pytest.raises(B.ArgumentError):
        B.GibbsEngine(rd, 4)
    rel.F = None
    rel.model.probit = True
    with pytest.raises(B.ArgumentError):
        check_interval(rel)
    rel.model.probit = False
    rel.model.censor = np.zeros(35, dtype=np.int8)
    with pytest.raises(B.ArgumentError):
        check_interval(rel)
    rel.model.censor = None
    check_interval(rel)
    assert np.array_equal(rel.model.interval, keep)


def test_tostr_counts_the_bounded_rows_and_leaves_the_others_alone(B):
    rel = _relation(B, alpha=2.0)
    assert B.toStr(rel) == "rati[α=2.0]"
    y = np.asarray(rel.data.values)
    lo, hi = y.copy(), y.copy()
    lo[:7], hi[7:12], lo[12], hi[12] = y[:7] - 1.0, INF, -INF, INF
    B.setInterval(rel, lo, hi)
    assert B.toStr(rel) == "rati[α=2.0 intv:13]"
    B.setInterval(rel, y, y)
    assert B.toStr(rel) == "rati[α=2.0 intv:0]"


# ---- the restated map ---------------------------------------------------------------------------------------------------------
def test_purpose_number_matches_the_header(B):
    h = open(os.path.join(ROOT, "include", "bdf.h")).read()
    assert re.search(r"#define BDF_P_INTERVAL\s+14\b", h)
    from bdf_amd import _lib
    assert _lib.P_INTERVAL == IR.P_INTERVAL == 14


def test_uniforms_are_the_library_stream(O):
    for seed, sweep, tag in ((42, 1, 1), (0xDEADBEEF12345, 7, 3)):
        u = IR.uniforms(seed, sweep, tag, 50)
        for k in (0, 1, 17, 49):
            o = O.draw(seed, sweep, IR.P_INTERVAL, 0x800000 | tag, k, 0)
            x = (int(o[1]) << 32) | int(o[0])
            assert u[k] == ((x >> 11) + 0.5) * 2.0 ** -53
    import censored_restatement as CR
    assert not np.array_equal(IR.uniforms(1, 1, 1, 8), CR.uniforms(1, 1, 1, 8))         # a stream of its own


def _exact_quantile(m, lo, hi, alpha, u):
    """the quantile at u of N(m, 1 / alpha) on [lo, hi] from the doubles as they are, in 40-digit arithmetic: Newton's iteration on
    the tail probability that is at most 1/2 (Phi(x) = p below the median, Phi(-x) = 1 - p above it) from the double estimate"""
    from mpmath import mp, mpf
    from scipy.special import ndtri
    with mp.workdps(40):
        m, lo, hi, alpha, u = (mpf(float(t)) for t in (m, lo, hi, alpha, u))
        ra = mp.sqrt(alpha)
        a, b = (lo - m) * ra, (hi - m) * ra
        Pa, Pb = mp.ncdf(a), mp.ncdf(b)
        p, q = Pa + u * (Pb - Pa), mp.ncdf(-b) + (1 - u) * (Pb - Pa)
        t = min(p, q)
        x = mpf(float(ndtri(float(t))))
        for _ in range(8):                         # quadratic from a start good to 1e-15: far more than enough
            x -= (mp.ncdf(x) - t) / mp.npdf(x)
        return m + (x if p <= q else -x) / ra


def test_draw_z_matches_a_40_digit_inversion():
    """Standardised lower bounds a in [-8, 8], widths 1e-3 ... 16 (log-uniform), alpha in {0.04, 5, 900}, m standard normal, 100
    points per alpha; per point a random u, a small one (which a wide interval above m turns into the far tail of the reflected
    map), u = 2^-54 (the smallest uniform of the stream) and u = 1.0 (its largest, after rounding), where the answer is the bound.
    Measured: worst |z - exact| sqrt(alpha) = 6.5e-15 standard deviations, at alpha = 900, where the rounding of z itself is up to
    ulp(|z|) / 2 = 1.1e-16 |z| sqrt(alpha) = 3.3e-15 sd per unit of |z|.  The bound is ten times the measured figure; scipy's
    truncnorm.ppf is 2.8e-12 off on this grid, so a map that needed 1e-12 would be wrong.  (The form with 1 - v for the complement
    in the reflected branch is 1e-5 sd off at a = -7.9, width 16, u = 1e-8: the small u are in the grid for that.)"""
    rng = np.random.default_rng(7)
    worst, at = 0.0, None
    from mpmath import mpf
    for alpha in (0.04, 5.0, 900.0):
        ra = np.sqrt(alpha)
        for _ in range(100):
            a, w, m = rng.uniform(-8.0, 8.0), 10.0 ** rng.uniform(-3.0, np.log10(16.0)), rng.standard_normal()
            lo, hi = m + a / ra, m + (a + w) / ra
            for u in (rng.random(), rng.random() * 10.0 ** rng.uniform(-12.0, 0.0), 2.0 ** -54, 1.0):
                z = float(IR.draw_z(m, lo, hi, alpha, u))
                assert lo <= z <= hi
                err = float(abs(mpf(z) - _exact_quantile(m, lo, hi, alpha, u)) * mpf(ra))
                if err > worst:
                    worst, at = err, (alpha, a, w, u)
    print(f"draw_z against the 40-digit inversion: worst |z - exact| sqrt(alpha) = {worst:.3e} at (alpha, a, width, u) = {at}")
    assert worst <= 6.5e-14
    # and the extreme uniforms give the bounds to that accuracy
    z = IR.draw_z(0.0, np.array([-1.0, 2.0, -9.0]), np.array([1.0, 3.0, -8.5]), 1.0, 1.0)
    assert np.abs(z - np.array([1.0, 3.0, -8.5])).max() <= 6.5e-14


@pytest.mark.parametrize("alpha", [0.04, 5.0, 900.0])
@pytest.mark.parametrize("a,b", [(-1.0, 1.0), (2.0, 3.0), (-9.0, -8.5), (-3.0, 7.0), (0.5, INF), (-INF, -2.0), (5.0, 5.001)])
def test_draw_z_mean_matches_the_truncated_normal(a, b, alpha):
    """stratified u = (k + 1/2) / n: the mean of the draws is the midpoint rule for the integral of the quantile function, which
    is the mean of the truncated normal.  The strata and the bound are those of the censored model's stratified test (2^20 strata,
    1e-4 standard deviations: the quantile of an interval with an open side is unbounded at one end, like sqrt(-2 log u), where
    the rule's error is a few 1e-6; a closed interval does better); it separates any wrong branch, a wrong reflection or a
    misplaced sqrt(alpha), which are off by order 1 or by the interval's width."""
    n = 1 << 20
    u = (np.arange(n) + 0.5) / n
    ra, m = np.sqrt(alpha), 0.7
    lo, hi = m + a / ra, m + b / ra
    z = IR.draw_z(np.full(n, m), lo, hi, alpha, u)
    expect = truncnorm.mean(a, b, loc=m, scale=1.0 / ra)
    assert np.all(np.isfinite(z)) and np.all(z >= lo) and np.all(z <= hi)
    assert abs(z.mean() - expect) * ra <= 1e-4 * min(1.0, b - a), (z.mean(), expect)
    assert np.all(np.diff(z) >= 0)                     # an inversion: monotone in u, reflected or not


def test_draw_z_is_finite_and_inside_the_bounds_everywhere():
    a = np.linspace(-50.0, 50.0, 2001)
    for alpha in (1e-2, 1.0, 1e3):
        ra = np.sqrt(alpha)
        for u in (2.0 ** -54, 0.5, 1.0 - 2.0 ** -53, 1.0):
            for w in (1e-6, 0.3, 4.0, 60.0, INF):
                for m in (0.0, -3.25, 1e3):
                    lo, hi = m + a / ra, m + (a + w) / ra
                    for lo_, hi_ in ((lo, hi), (np.full_like(lo, -INF), hi)):
                        z = IR.draw_z(m, lo_, hi_, alpha, np.full_like(a, u))
                        assert np.all(np.isfinite(z)) and np.all(z >= lo_) and np.all(z <= hi_)
    for u in (2.0 ** -54, 0.5, 1.0):
        assert np.isfinite(IR.draw_z(0.3, -INF, INF, 2.0, u))       # the row that says nothing: a draw of N(m, 1 / alpha)
    assert abs(float(IR.draw_z(0.3, -INF, INF, 4.0, 0.5)) - 0.3) <= 1e-15
    # both bounds beyond the underflow of Phi on one side of m: the nearer bound (the exact law lies within about sd / 37 of it)
    z = IR.draw_z(0.0, np.array([40.0, -45.0]), np.array([45.0, -40.0]), 1.0, np.array([0.5, 0.999]))
    assert np.array_equal(z, [40.0, -40.0])


def test_exact_observations_keep_their_value():
    rng = np.random.default_rng(0)
    m, y, u = rng.standard_normal(100) * 50, rng.standard_normal(100), rng.random(100)
    assert np.array_equal(IR.draw_z(m, y, y, 3.0, u, y=y), y)
    assert np.array_equal(IR.draw_z(m, y, y, 3.0, u), y)


def test_header_and_restatement_state_the_same_map():
    """the scalar map of csrc/interval.h, compiled for the host where a C++ compiler is at hand, against the restatement: the same
    formula, so they agree to the difference of two erfc and inverse-CDF implementations (the library's AS 241 and scipy's ndtri,
    each good to a few ulp of x: 1e-12 of |z| leaves three digits)"""
    import shutil
    import subprocess
    import tempfile
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")         # (csrc/Makefile's: as a host compiler, when there is no other)
    cxx = [shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")]
    if cxx[0] is None:
        cxx = [hipcc, "-x", "c++"]
    rng = np.random.default_rng(2)
    n = 4000
    alpha = np.repeat([0.04, 5.0, 900.0], n // 3 + 1)[:n]
    ra = np.sqrt(alpha)
    m = rng.standard_normal(n)
    a, w = rng.uniform(-45.0, 45.0, n), 10.0 ** rng.uniform(-6.0, 2.0, n)
    a[::3] = rng.uniform(-8.0, 8.0, len(a[::3]))
    lo, hi = m + a / ra, m + (a + w) / ra
    lo[5::11], hi[7::13] = -INF, INF
    u = rng.random(n)
    u[::17], u[1::17] = 2.0 ** -54, 1.0
    src = r'''
        #include <cstdio>
        #include "interval.h"
        int main() { double m, lo, hi, al, u; while (scanf("%lf %lf %lf %lf %lf", &m, &lo, &hi, &al, &u) == 5)
                         printf("%.17g\n", bdf_interval_z(m, 0.5 * (lo + hi), lo, hi, al, u)); return 0; }
    '''
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "t.cpp"), "w").write(src)
        subprocess.run(cxx + ["-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "bayesiandatafusion.jl_amd", "csrc"), os.path.join(td, "t.cpp"),
                        "-o", os.path.join(td, "t")], check=True)
        text = "".join("%.17g %.17g %.17g %.17g %.17g\n" % t for t in zip(m, lo, hi, alpha, u))
        out = subprocess.run([os.path.join(td, "t")], input=text, capture_output=True, text=True, check=True).stdout
    z_c = np.array([float(t) for t in out.split()])
    z = IR.draw_z(m, lo, hi, alpha, u)
    assert len(z_c) == n and np.all(np.isfinite(z_c)) and np.all(z_c >= lo) and np.all(z_c <= hi)
    assert np.abs(z_c - z).max() <= 1e-12 * np.maximum(1.0, np.abs(z)).max()


# ---- the resource listing -------------------------------------------------------------------------------------------------------
# (VGPRs, scratch bytes per lane, waves per SIMD) of the nine shapes <modes, vector width, row pieces> of k_interval_draw, as
# DESIGN.md section 14 prints them
INTERVAL_KERNELS = {
    "15k_interval_drawILi2ELi1ELi1EEEvNS_8IntvArgsE": (49, 0, 8),
    "15k_interval_drawILi2ELi4ELi1EEEvNS_8IntvArgsE": (86, 0, 5),
    "15k_interval_drawILi2ELi4ELi2EEEvNS_8IntvArgsE": (88, 0, 5),
    "15k_interval_drawILi3ELi1ELi1EEEvNS_8IntvArgsE": (49, 0, 8),
    "15k_interval_drawILi3ELi4ELi1EEEvNS_8IntvArgsE": (119, 0, 4),
    "15k_interval_drawILi3ELi4ELi2EEEvNS_8IntvArgsE": (121, 0, 4),
    "15k_interval_drawILi4ELi1ELi1EEEvNS_8IntvArgsE": (49, 0, 8),
    "15k_interval_drawILi4ELi4ELi1EEEvNS_8IntvArgsE": (88, 0, 5),
    "15k_interval_drawILi4ELi4ELi2EEEvNS_8IntvArgsE": (154, 0, 3),
}


def test_interval_kernels_use_no_scratch_and_no_lds():
    draws = _resources("k_interval")
    assert draws == INTERVAL_KERNELS
    for k, v in draws.items():
        assert v[1] == 0 and v[2] >= 2, (k, v)
    path = os.path.join(ROOT, "bayesiandatafusion.jl_amd", "csrc", "k_interval.o.res")
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", open(path).read())]
    assert len(lds) == 9 and not any(lds)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for k, (vgprs, scratch, waves) in INTERVAL_KERNELS.items():
        nm, vec, nc = re.search(r"ILi(\d)ELi(\d)ELi(\d)E", k).groups()
        assert re.search(rf"\|\s*{nm}\s*\|\s*{vec}\s*\|\s*{nc}\s*\|\s*{vgprs}\s*\|\s*{scratch}\s*\|\s*0\s*\|\s*{waves}\s*\|", design), k
