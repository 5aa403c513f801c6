"""The non-negative prior of an entity's rows without a GPU: the restated sweep leaves the exact truncated
law invariant, the scalar map of csrc/nonneg.h (compiled for the host) against a 50-digit quantile and against the restatement,
the restated hyper draw's Gamma mean, the setter's guards, the stream numbers in include/bdf.h, the sweep kernel's resource usage,
and the branch margins of the GPU tests' inputs."""
import glob
import math
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import nonneg_restatement as NR
import spike_restatement as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bayesiandatafusion.jl_amd", "csrc")


# ---- (a) the sweep leaves the exact law invariant -----------------------------------------------------------------------------
def _moments_by_quadrature(P, c, hi=8.0, n=321):
    """mean and second moment of every component under exp(-u'Pu / 2 + c'u) on [0, hi]^3: the trapezoid rule, n points per axis"""
    x = np.linspace(0.0, hi, n)
    w = np.full(n, x[1] - x[0])
    w[0] = w[-1] = 0.5 * (x[1] - x[0])
    X1, X2 = np.meshgrid(x, x, indexing="ij")
    W12 = np.outer(w, w)
    Z, m1, m2 = 0.0, np.zeros(3), np.zeros(3)
    for i, x0 in enumerate(x):                    # one plane of the grid at a time
        q = P[0, 0] * x0 * x0 + P[1, 1] * X1 * X1 + P[2, 2] * X2 * X2 + 2.0 * (P[0, 1] * x0 * X1 + P[0, 2] * x0 * X2 + P[1, 2] * X1 * X2)
        f = np.exp(-0.5 * q + c[0] * x0 + c[1] * X1 + c[2] * X2) * W12 * w[i]
        s = f.sum()
        Z += s
        m1 += np.array([x0 * s, (f * X1).sum(), (f * X2).sum()])
        m2 += np.array([x0 * x0 * s, (f * X1 * X1).sum(), (f * X2 * X2).sum()])
    return m1 / Z, m2 / Z


@pytest.mark.parametrize("corr", [0.05, 0.9])
@pytest.mark.parametrize("c", [(0.9, -0.7, 0.5), (-3.0, 2.0, -1.0)])
def test_sweep_leaves_the_exact_law_invariant(corr, c):
    """D = 3, P = diag(0.8, 1.5, 2.5) + K with K's off-diagonal correlation `corr`: a chain of 200,000 restated sweeps, each from
    the output of the one before; mean and second moment of every component within 5 standard errors of the quadrature of
    exp(-u'Pu / 2 + c'u) on [0, 8]^3 (the mass beyond 8 is below 1e-12 for these P and c); the standard errors from 200 batch means
    of 1,000 sweeps."""
    n, nb = 200_000, 200
    rng = np.random.default_rng([26, int(100 * corr), int(abs(10 * c[0]))])
    sd = np.array([1.2, 0.9, 1.1])
    K = corr * np.outer(sd, sd)
    K[np.diag_indices(3)] = sd * sd
    P, c = np.diag([0.8, 1.5, 2.5]) + K, np.array(c)
    m1, m2 = _moments_by_quadrature(P, c)
    U = rng.random((n, 3))
    u, chain = np.zeros(3), np.zeros((n, 3))
    for t in range(n):
        u, _ = NR.sweep_row(P, c, u, U[t])
        chain[t] = u
    assert np.all(chain >= 0.0) and np.all(np.isfinite(chain)) and chain.max() < 8.0
    dev = []
    for stat, exact in ((chain, m1), (chain * chain, m2)):
        batches = stat.reshape(nb, n // nb, 3).mean(axis=1)
        se = batches.std(axis=0, ddof=1) / np.sqrt(nb)
        dev.append(np.abs(stat.mean(axis=0) - exact) / se)
    print(f"corr {corr} c {tuple(c)}: means {np.round(m1, 4)}, second moments {np.round(m2, 4)}; deviations in standard errors "
          f"{np.round(dev[0], 2)} {np.round(dev[1], 2)}")
    assert np.all(np.concatenate(dev) <= 5.0), dev


def test_the_two_restated_sweeps_agree():
    """sweep_row (scalar) against sweep_rows (all rows at once) on a crafted case that meets both branches of the map"""
    case = NR.sweep_case(5, 63)
    U = NR.uniforms(NR.SWEEP_SEED, case["sweep"], NR.SWEEP_TAG, 63, 5, NR.SWEEP_ROW_BEGIN)
    many, margin, t = NR.sweep_rows(case["P"], case["c"], case["u_current"], U, with_t=True)
    one = [NR.sweep_row(case["P"][i], case["c"][i], case["u_current"][i], U[i]) for i in range(63)]
    np.testing.assert_allclose(many, np.stack([o[0] for o in one]), rtol=1e-11, atol=1e-13)
    assert abs(margin - min(o[1] for o in one)) <= 1e-9 * margin
    assert all(k > 0 for k in NR.t_classes(t))


# ---- (b) the header against a 50-digit quantile and against the restatement ----------------------------------------------------
@pytest.fixture(scope="module")
def host_program():
    """csrc/nonneg.h compiled for the host into a stand-alone program that maps lines of (m, lam, U) to bdf_nonneg of them"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")         # (csrc/Makefile's: as a host compiler, when there is no other)
    cxx = [shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")]
    if cxx[0] is None:
        cxx = [hipcc, "-x", "c++"]
    src = r'''
        #include <cstdio>
        #include "nonneg.h"
        int main() { double m, lam, u; while (scanf("%lf %lf %lf", &m, &lam, &u) == 3) printf("%.17g\n", bdf_nonneg(m, lam, u)); return 0; }
    '''
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "t.cpp"), "w").write(src)
        subprocess.run(cxx + ["-O1", "-ffp-contract=off", "-I", CSRC, os.path.join(td, "t.cpp"), "-o", os.path.join(td, "t")], check=True)
        yield os.path.join(td, "t")


def _host_map(program, m, lam, U):
    """bdf_nonneg of every (m, lam, U) by the host program"""
    m, lam, U = np.broadcast_arrays(np.asarray(m, dtype=np.float64), np.asarray(lam, dtype=np.float64), np.asarray(U, dtype=np.float64))
    text = "".join("%.17g %.17g %.17g\n" % t for t in zip(m.ravel(), lam.ravel(), U.ravel()))
    out = subprocess.run([program], input=text, capture_output=True, text=True, check=True).stdout
    got = np.array([float(t) for t in out.split()])
    assert len(got) == m.size
    return got.reshape(m.shape)


U_MIN, U_MAX = 2.0 ** -54, float(np.nextafter(1.0, 0.0))      # the smallest uniform of the stream; the largest double below 1


def _exact_excess_sd(t, U):
    """(u - 0) sqrt(lam) of the exact law, from the doubles as they are, in 50-digit arithmetic.  t >= -37: Newton's iteration on
    the tail probability that is at most 1/2, from the double estimate, then max(t + x, 0).  t < -37: the excess e over the bound
    a = -t with Q(a + e) / Q(a) = U, by Newton's iteration on its logarithm from the map's own leading term."""
    from mpmath import mp, mpf
    from scipy.special import ndtri
    with mp.workdps(50):
        t, U = mpf(float(t)), mpf(float(U))
        if t >= NR.TAIL:
            Pt = mp.ncdf(t)
            p, q = mp.ncdf(-t) + U * Pt, (1 - U) * Pt
            if q == 0:
                return mp.inf
            tt = min(p, q)
            x = mpf(float(ndtri(float(tt))))
            for _ in range(3):                     # quadratic from a start good to 1e-15
                x -= (mp.ncdf(x) - tt) / mp.npdf(x)
            return max(t + (x if p <= q else -x), mpf(0))
        a, L = -t, -2 * mp.log(U)
        e = L / (mp.sqrt(a * a + L) + a)
        lq = lambda z: mp.log(mp.erfc(z / mp.sqrt(2)) / 2)
        for _ in range(7):                         # quadratic from a start good to 1 / t^2
            f = lq(a + e) - lq(a) - mp.log(U)
            e += f * mp.exp(lq(a + e)) / mp.npdf(a + e)
        return e


def test_header_map_is_finite_and_non_negative_everywhere(host_program):
    """t in [-45, 45] (18,001 points) at the smallest uniform, the largest below 1, 1 and 1/2, at three precisions"""
    t = np.linspace(-45.0, 45.0, 18001)
    for lam in (0.04, 1.0, 900.0):
        for U in (U_MIN, U_MAX, 1.0, 0.5):
            u = _host_map(host_program, t / np.sqrt(lam), lam, U)
            assert np.all(np.isfinite(u)) and np.all(u >= 0.0), (lam, U)
    assert _host_map(host_program, -50.0, 1.0, 1.0) == 0.0 and _host_map(host_program, -50.0, 1.0, U_MIN) > 0.0


def test_header_map_against_a_50_digit_quantile(host_program):
    """The exact branch: t in [-37, 40] in steps of 1/4, per t three uniforms that are multiples of 2^-12 (for which 1 - U is exact),
    lam in {0.04, 1, 900} in turn; the error in standard deviations is held to the project's 1e-9 for a kernel's map against the
    exact law (tests/test_censored_host.py).  Measured: 2.2e-14 standard deviations (printed below).
    The tail: t in {-37 - 1e-7, -40, -50, -100, -200, -500, -1000} x U in {1e-12, 1e-6, 0.01, 1/2, 0.99, the largest below 1}: the
    excess over the bound is within 1.1 / t^2 relative of the exact one -- 1 / t^2 is the next term of the tail's expansion, the
    10 % cover the rounding of log and sqrt."""
    from mpmath import mpf
    rng = np.random.default_rng(5)
    ts = np.arange(-37.0, 40.0 + 1e-9, 0.25)
    lams = np.array([0.04, 1.0, 900.0])[np.arange(len(ts)) % 3]
    worst, at = 0.0, None
    Us = rng.integers(1, 4096, (len(ts), 3)) / 4096.0
    got = _host_map(host_program, (ts / np.sqrt(lams))[:, None], lams[:, None], Us)
    for i, t in enumerate(ts):
        s = math.sqrt(lams[i])
        t_map = (t / s) * s                       # the t the map forms from the doubles it is given
        for k in range(3):
            err = float(abs(mpf(float(got[i, k])) * mpf(s) - _exact_excess_sd(t_map, Us[i, k])))
            if err > worst:
                worst, at = err, (t, lams[i], Us[i, k])
    print(f"nonneg map against the 50-digit quantile: worst error {worst:.3e} standard deviations at (t, lam, U) = {at}")
    assert worst <= 1e-9
    worst_tail = 0.0
    tail_t, tail_U = (-37.0 - 1e-7, -40.0, -50.0, -100.0, -200.0, -500.0, -1000.0), (1e-12, 1e-6, 0.01, 0.5, 0.99, U_MAX)
    tail = _host_map(host_program, np.array(tail_t)[:, None], 1.0, np.array(tail_U)[None, :])
    for i, t in enumerate(tail_t):
        for k, U in enumerate(tail_U):
            e = float(tail[i, k])
            exact = _exact_excess_sd(t, U)
            rel = float(abs(mpf(e) - exact) / exact)
            worst_tail = max(worst_tail, rel * t * t)
            assert rel <= 1.1 / (t * t), (t, U, rel)
            assert e < 1.0 / abs(t) * max(1.0, -2.0 * math.log(U))
    print(f"nonneg map's tail: worst (relative error) t^2 = {worst_tail:.4f}")


def test_header_and_restatement_state_the_same_map(host_program):
    """csrc/nonneg.h against nonneg_restatement.draw_u: the same formulas on two erfc and inverse-CDF implementations (AS 241 and
    scipy's ndtri) -- 1e-12 standard deviations; and the scalar path of sweep_row against the vectorised draw_u"""
    rng = np.random.default_rng(8)
    n = 6000
    lam = np.repeat([0.04, 5.0, 900.0], n // 3)
    t = rng.uniform(-60.0, 45.0, n)
    t[::5] = rng.uniform(-37.5, -36.5, len(t[::5]))              # around the seam of the two branches
    U = rng.random(n)
    U[::17], U[1::17], U[2::17] = U_MIN, 1.0, U_MAX
    m = t / np.sqrt(lam)
    ref = NR.draw_u(m, lam, U)
    got = _host_map(host_program, m, lam, U)
    assert np.all(ref >= 0.0) and np.all(np.isfinite(ref))
    assert np.max(np.abs(got - ref) * np.sqrt(lam)) <= 1e-12
    assert np.sum(m * np.sqrt(lam) < NR.TAIL) > 500 and np.sum(m * np.sqrt(lam) >= NR.TAIL) > 500
    one = np.array([NR.draw_u1(float(m[i]), float(lam[i]), float(U[i])) for i in range(n)])
    assert np.max(np.abs(one - ref) * np.sqrt(lam)) <= 1e-13


# ---- (c) the hyper draw's mean ------------------------------------------------------------------------------------------------
def test_hyper_draw_mean():
    """20,000 restated draws (sweep numbers 1 .. 20,000) at fixed q: the mean of tau within 5 standard errors of the mean of
    Gamma(shape + N / 2, rate + q / 2)"""
    draws, N = 20_000, 30
    q = np.array([0.0, 5.5, 41.0])
    shape, rate = 0.5, 0.7
    out = np.stack([NR.hyper_draw_q(q, N, shape, rate, 77, t, 3) for t in range(1, draws + 1)])
    k, r = shape + 0.5 * N, rate + 0.5 * q
    dev = np.abs(out.mean(axis=0) - k / r) / np.sqrt(k / r ** 2 / draws)
    print(f"nonneg hyper draw: deviations of the mean in standard errors {np.round(dev, 2)}")
    assert np.all(out > 0) and np.all(dev <= 5.0)
    S = np.abs(np.random.default_rng(1).standard_normal((N, 3)))
    assert np.array_equal(NR.hyper_draw(S, shape, rate, 77, 4, 3), NR.hyper_draw_q(np.sum(S * S, axis=0), N, shape, rate, 77, 4, 3))


# ---- (d) the setter's guards --------------------------------------------------------------------------------------------------
def _model(B, F=None):
    rng = np.random.default_rng(0)
    ids = np.stack([rng.integers(1, 21, 200), rng.integers(1, 11, 200)], axis=1)
    ids[:20, 0], ids[:10, 1] = np.arange(1, 21), np.arange(1, 11)
    ents = [B.Entity("u"), B.Entity("v", F=F)]
    rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": rng.standard_normal(200)}, "r", ents, dims=[20, 10])
    return ents, rel, B.RelationData(rel)


def test_setter_guards(B):
    ents, rel, rd = _model(B)
    assert ents[1].nonneg is None
    B.setNonNegative(ents[1])
    assert ents[1].nonneg == {"shape": 1.0, "rate": 1.0} and ents[0].nonneg is None
    B.setNonNegative(ents[0], shape=2.5, rate=1e-3)
    assert ents[0].nonneg == {"shape": 2.5, "rate": 1e-3}
    for bad in (0.49, -1.0, float("inf"), float("nan"), "1", True, None):
        with pytest.raises(B.ArgumentError, match=r"Entity v: shape = .* must be a finite number, at least 0\.5 \(setNonNegative\)"):
            B.setNonNegative(ents[1], shape=bad)
    for bad in (0.0, -2.0, float("inf"), float("nan"), None):
        with pytest.raises(B.ArgumentError, match=r"Entity v: rate = .* must be a finite number above 0 \(setNonNegative\)"):
            B.setNonNegative(ents[1], rate=bad)
    assert ents[1].nonneg == {"shape": 1.0, "rate": 1.0}            # a refused call leaves the entity as it was
    with pytest.raises(B.ArgumentError, match="setNonNegative takes an Entity"):
        B.setNonNegative("v")
    # no side information and no new rows on the entity
    fents, frel, frd = _model(B, F=np.ones((10, 2)))
    with pytest.raises(B.ArgumentError, match=r"Entity v has features: the non-negative prior \(setNonNegative\) does not take side information"):
        B.setNonNegative(fents[1])
    assert fents[1].nonneg is None
    from bdf_amd._two_mode import relation_of
    relation_of(frd, 4, "bpmf_vb")                    # ... so the trainers that refuse the prior still take the data
    B.setNewRows(fents[1], np.ones((3, 2)))
    fents[1].F = None
    with pytest.raises(B.ArgumentError, match=r"Entity v has new rows \(setNewRows\): the non-negative prior"):
        B.setNonNegative(fents[1])
    B.setNonNegative(fents[0])                        # ... the other entity may have it
    nents, _, _ = _model(B, F=np.ones((10, 2)))
    nents[1].F = None
    B.setNonNegative(nents[1])
    nents[1].F = np.ones((10, 2))
    with pytest.raises(B.ArgumentError, match=r"Entity v has the non-negative prior \(setNonNegative\): it takes no side information and no new rows"):
        B.setNewRows(nents[1], np.ones((3, 2)))
    # exclusive with the spike-and-slab prior on the same entity, either way round
    sents, _, _ = _model(B)
    B.setSpikeAndSlab(sents[1])
    with pytest.raises(B.ArgumentError, match=r"Entity v has the spike-and-slab prior \(setSpikeAndSlab\): it does not take the non-negative prior"):
        B.setNonNegative(sents[1])
    assert sents[1].nonneg is None
    B.setNonNegative(sents[0])                        # (a spike-and-slab and a non-negative entity may share a relation)
    with pytest.raises(B.ArgumentError, match=r"Entity u has the non-negative prior \(setNonNegative\): it does not take the spike-and-slab prior"):
        B.setSpikeAndSlab(sents[0])
    assert sents[0].spike is None
    # no background and no dense path on the entity's relations, either way round
    bents, brel, brd = _model(B)
    ids = np.unique(np.asarray(brel.data.ids), axis=0)

    def listed(name):
        r = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": np.ones(len(ids))}, name, [B.Entity("u"), B.Entity("v")], dims=[20, 10])
        return r, B.RelationData(r)
    brel2, _ = listed("b")
    B.setBackground(brel2, 0.1)
    with pytest.raises(B.ArgumentError, match=r"Relation b has a background \(setBackground\): its entity v does not take the non-negative prior"):
        B.setNonNegative(brel2.entities[1])
    assert brel2.entities[1].nonneg is None
    brel3, _ = listed("c")
    B.setNonNegative(brel3.entities[0])
    with pytest.raises(B.ArgumentError, match=r"Entity u has the non-negative prior \(setNonNegative\): its relation c does not take a background"):
        B.setBackground(brel3, 0.1)
    full = np.stack(np.meshgrid(np.arange(1, 21), np.arange(1, 11), indexing="ij"), axis=-1).reshape(-1, 2)
    drel = B.Relation({"u": full[:, 0], "v": full[:, 1], "y": np.ones(len(full))}, "d", [B.Entity("u"), B.Entity("v")], dims=[20, 10])
    B.RelationData(drel)
    B.setNonNegative(drel.entities[1])
    with pytest.raises(B.ArgumentError, match=r"Entity v has the non-negative prior \(setNonNegative\): its relation d does not take"):
        B.setDense(drel)
    drel.entities[1].nonneg = None
    B.setDense(drel)
    with pytest.raises(B.ArgumentError, match=r"Relation d is dense \(setDense\): its entity v does not take the non-negative prior"):
        B.setNonNegative(drel.entities[1])
    # ... checked again when a sampler is built (features may come after the setter), and one rank only
    from bdf_amd.relation_data import check_nonneg
    check_nonneg(ents[1])
    with pytest.raises(B.ArgumentError, match=r"Entity v has the non-negative prior \(setNonNegative\): one rank only"):
        check_nonneg(ents[1], world=2)
    ents[1].nonneg["shape"] = 0.1
    with pytest.raises(B.ArgumentError, match="shape = 0.1"):
        check_nonneg(ents[1])
    ents[1].nonneg["shape"] = 1.0
    ents[1].F = np.ones((10, 2))
    with pytest.raises(B.ArgumentError, match="Entity v has features"):
        check_nonneg(ents[1])
    ents[1].F = None
    # the two-mode trainers refuse it
    for who in ("bpmf_vb", "macau_hmc"):
        with pytest.raises(B.ArgumentError, match=rf"{who} has the Normal-Wishart prior only; . has the non-negative prior"):
            relation_of(rd, 4, who)
    assert B.toStr(ents[1]) == "v[]"                   # no model yet: what it was
    assert "not centred" in B.setNonNegative.__doc__.replace("NOT", "not")


# ---- (e) the stream numbers ---------------------------------------------------------------------------------------------------
def test_stream_numbers_in_the_header(B):
    h = open(os.path.join(ROOT, "include", "bdf.h")).read()
    got = {name: int(v) for name, v in re.findall(r"#define (BDF_P_NONNEG\w*)\s+(\d+)", h)}
    assert got == {"BDF_P_NONNEG": 25, "BDF_P_NONNEG_N": 26, "BDF_P_NONNEG_U": 27}
    from bdf_amd import _lib
    assert (_lib.P_NONNEG, _lib.P_NONNEG_N, _lib.P_NONNEG_U) == (25, 26, 27) == (NR.P_NONNEG, NR.P_NONNEG_N, NR.P_NONNEG_U)
    every = [int(v) for v in re.findall(r"#define BDF_P_\w+\s+(\d+)", h)]
    assert len(every) == len(set(every))               # no stream number is used twice


# ---- (f) the sweep kernel's resource usage -------------------------------------------------------------------------------------
def test_sweep_kernel_uses_no_scratch_and_spills_nothing():
    """every instantiation of k_nonneg_sweep in the build's csrc/*.o.res, DP in {16, 32, 64} (the figures of a kernel include the
    map it calls): no scratch, no spill; the registers, LDS and occupancy are the ones DESIGN.md section 26 quotes"""
    res, name = {}, None
    for f in glob.glob(os.path.join(CSRC, "*.o.res")):
        for line in open(f):
            m = re.search(r"remark: \s*(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill|Occupancy \[waves/SIMD\]|"
                          r"LDS Size \[bytes/block\]): (\S+)", line)
            if not m:
                continue
            if m.group(1) == "Function Name":
                name = m.group(2)
                res[name] = {}
            elif name is not None:
                res[name][m.group(1)] = int(m.group(2))
    assert res, "no csrc/*.o.res: build with __graft_entry__.build() (make)"
    sw = {k: v for k, v in res.items() if "k_nonneg_sweepILi" in k}
    assert set(sw) == {"_ZN12_GLOBAL__N_114k_nonneg_sweepILi%dEEEv15NonnegSweepArgs" % dp for dp in (16, 32, 64)}, sorted(sw)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for k, v in sorted(sw.items()):
        print(k, v)
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
        dp = re.search(r"sweepILi(\d+)E", k)
        if dp:
            assert v["LDS Size [bytes/block]"] == 8 * int(dp.group(1)) * 64
            assert re.search(rf"\|\s*{dp.group(1)}\s*\|\s*{v['VGPRs']}\s*\|\s*{v['LDS Size [bytes/block]']}\s*\|\s*{v['Occupancy [waves/SIMD]']}\s*\|", design), k


# ---- (g) the GPU tests' inputs: no t near the seam of the two branches ---------------------------------------------------------
def test_branch_margins_of_the_gpu_inputs(O):
    """tests/test_gpu_nonneg.py holds the device to the restatement to 1e-9 when no t is nearer -37 than 1e-9: checked here for
    every sweep case, every row case (numpy row systems, the oracle's streams) and every whole-iteration model"""
    worst = np.inf
    seen = np.zeros(4, dtype=np.int64)
    for D in NR.SWEEP_DS:
        for n_rows in NR.SWEEP_ROWS:
            case = NR.sweep_case(D, n_rows)
            U = NR.uniforms(NR.SWEEP_SEED, case["sweep"], NR.SWEEP_TAG, n_rows, D, NR.SWEEP_ROW_BEGIN)
            u, margin, t = NR.sweep_rows(case["P"], case["c"], case["u_current"], U, with_t=True)
            assert margin >= 1e-9, (D, n_rows, margin)
            k = NR.t_classes(t)
            assert n_rows * D < 8 or all(x > 0 for x in k), (D, n_rows, k)
            seen += k
            worst = min(worst, margin)
    assert np.all(seen > 0)
    for D, n_modes, mode, variant in SR.row_cases():
        case = NR.row_case(D, n_modes, mode, variant)
        terms = [(ids, vals, w, mode, alpha, float(np.mean(vals)), case["facs"]) for ids, vals, w, alpha in case["rels"]]
        P, c = SR.row_systems(terms, case["N"], D, np.diag(case["tau"]), np.zeros(D))
        u, margin = NR.sweep_rows(P, c, case["u_current"], NR.uniforms(SR.ROW_SEED, case["sweep"], NR.ROW_TAG, case["N"], D))
        assert margin >= 1e-9 and np.all(u >= 0), (D, n_modes, mode, variant, margin)
        worst = min(worst, margin)
    for name in NR.CHAIN_MODELS:
        dims, rels, nonneg, spike, feats, n_test = NR.chain_model(name)
        train = [dict(r, ids=r["ids"][n_test:], values=r["values"][n_test:]) if i == 0 else r for i, r in enumerate(rels)]
        out = NR.run_chain(train, dims, NR.CHAIN_D, NR.CHAIN_SEED, 6, nonneg, spike=spike, feats=feats, burnin=3)
        assert out["margin"] >= 1e-9 and out["spike_margin"] >= 1e-9, (name, out["margin"], out["spike_margin"])
        assert (out["mean"][0] == 0.0) == (name == "both")
        for j in nonneg:
            assert np.all(out["S"][j] >= 0)
        worst = min(worst, out["margin"])
    print(f"smallest branch margin of the GPU tests' inputs: {worst:.3e}")
