"""The Polya-Gamma noise models on the host (no GPU): setLogit / setCounts and what they guard, the stream purpose in include/bdf.h,
csrc/pg.h compiled for the host against tests/pg_restatement.py (the scalar maps, and the sampler itself on the same cursor), the
law of PG(b, c), the moments of the normal branch against an evaluation in extended precision, the invariance of the exact
posterior of a tiny model under the restated sweep, and the resource listing the build leaves for the new kernels."""
import math
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import pg_restatement as PG
from test_probit_host import _resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _relation(B, kind="counts", n=40, test=None, names=("u", "v"), dims=(8, 6)):
    rng = np.random.default_rng(3)
    table = {nm: rng.integers(1, d + 1, n) for nm, d in zip(names, dims)}
    table["y"] = (np.arange(n) % 2).astype(np.float64) if kind == "logit" else (np.arange(n) % 5).astype(np.float64)
    rel = B.Relation(table, "plays", [B.Entity(nm) for nm in names], alpha=2.0, dims=list(dims))
    if test is not None:
        B.assignToTest(rel, test)
    return rel


SETTERS = {"logit": lambda B, rel: B.setLogit(rel), "counts": lambda B, rel: B.setCounts(rel, 3)}


# ---- setLogit / setCounts ---------------------------------------------------------------------------------------------------------
def test_default_has_neither(B):
    assert _relation(B).model.pg is None and B.RelationModel().pg is None


def test_setters_store_the_model_and_reset_the_device_state(B):
    rel = _relation(B, "logit", test=np.arange(1, 11))
    rel._dev = object()
    rel.model.alpha_sample = False
    assert B.setLogit(rel, offset=-0.4) is None
    assert rel.model.pg == {"model": "logit", "r": 0, "offset": -0.4} and rel._dev is None
    assert rel.model.alpha == 1.0 and rel.model.alpha_sample is False and rel.model.mean_value == -0.4
    assert rel.class_cut == 0.5 and np.array_equal(rel.test_label, rel.test_vec.values < 0.5)
    rel = _relation(B, "counts", test=np.arange(1, 11))
    rel._dev = object()
    assert B.setCounts(rel, 5, offset=0.25) is None
    assert rel.model.pg == {"model": "counts", "r": 5, "offset": 0.25} and rel._dev is None
    assert rel.model.alpha == 1.0 and rel.model.alpha_sample is False and rel.model.mean_value == 0.25
    B.setCounts(rel, r=np.int64(2))                                 # again: the dispersion is replaced
    assert rel.model.pg == {"model": "counts", "r": 2, "offset": 0.0}
    with pytest.raises(B.ArgumentError, match="precision"):
        B.setPrecision(rel, 3.0)


@pytest.mark.parametrize("bad", [0, -1, 1.5, float("nan"), float("inf"), "3", None, True, 2 ** 31 + 1])
def test_setcounts_refuses_a_dispersion_that_is_no_positive_integer(B, bad):
    rel = _relation(B)
    with pytest.raises(B.ArgumentError, match="r ="):
        B.setCounts(rel, bad)
    assert rel.model.pg is None


@pytest.mark.parametrize("which", ["logit", "counts"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), "0", None, True])
def test_offset_must_be_finite(B, which, bad):
    rel = _relation(B, which)
    with pytest.raises(B.ArgumentError, match="offset"):
        B.setLogit(rel, offset=bad) if which == "logit" else B.setCounts(rel, 3, offset=bad)
    assert rel.model.pg is None


def test_values_are_validated_in_training_and_test(B):
    for bad in (0.5, -1.0, 2.0, float("nan")):
        rel = _relation(B, "logit")
        rel.data.values[7] = bad
        with pytest.raises(B.ArgumentError, match="0 and 1"):
            B.setLogit(rel)
        rel = _relation(B, "logit", test=np.arange(1, 11))
        rel.test_vec.values[3] = bad
        with pytest.raises(B.ArgumentError, match="0 and 1"):
            B.setLogit(rel)
    for bad in (0.5, -1.0, float("nan"), float("inf"), 2.0 ** 31 + 1):
        rel = _relation(B, "counts")
        rel.data.values[7] = bad
        with pytest.raises(B.ArgumentError, match="integers"):
            B.setCounts(rel, 3)
        rel = _relation(B, "counts", test=np.arange(1, 11))
        rel.test_vec.values[3] = bad
        with pytest.raises(B.ArgumentError, match="integers"):
            B.setCounts(rel, 3)
    rel = _relation(B, "counts")
    rel.data.values[7] = 2.0 ** 31                                  # the largest count is taken
    B.setCounts(rel, 1)
    # a test set given later is held to the same
    rel = _relation(B, "logit")
    B.setLogit(rel)
    with pytest.raises(B.ArgumentError, match="0 or 1"):
        B.setTest(rel, {"u": [1, 2], "v": [1, 1], "y": [0.0, 2.0]})
    rel = _relation(B, "counts")
    B.setCounts(rel, 3)
    with pytest.raises(B.ArgumentError, match="integers"):
        B.setTest(rel, {"u": [1, 2], "v": [1, 1], "y": [0.0, 1.5]})
    B.setTest(rel, {"u": [1, 2], "v": [1, 1], "y": [0.0, 7.0]})
    assert len(rel.test_vec) == 2


@pytest.mark.parametrize("which", ["logit", "counts"])
def test_offset_survives_the_test_split(B, which):
    from bdf_amd.relation_data import check_pg
    rel = _relation(B, which)
    B.setLogit(rel, offset=0.7) if which == "logit" else B.setCounts(rel, 4, offset=0.7)
    B.assignToTest(rel, np.arange(1, 11))
    assert rel.model.pg["offset"] == 0.7 and rel.data.nnz() == 30 and len(rel.test_vec) == 10
    B.setTest(rel, {"u": [1, 2, 3], "v": [1, 1, 2], "y": [0.0, 1.0, 1.0]})
    assert rel.model.pg["offset"] == 0.7
    rel.model.mean_value = 123.0                                   # whatever became of it: the sampler's set-up puts the offset back
    check_pg(rel)
    assert rel.model.mean_value == 0.7


@pytest.mark.parametrize("which", ["logit", "counts"])
def test_exclusions_in_both_orders(B, which):
    mine = SETTERS[which]
    other = SETTERS["counts" if which == "logit" else "logit"]

    def fresh(kind=None):
        if kind == "ordinal":
            r = _relation(B, which)
            r.data.values[:] = np.arange(40) % 5 + 1
            return r
        if kind == "both":                                         # values both models take: 0 / 1
            return _relation(B, "logit")
        return _relation(B, which)

    # each other
    rel = fresh("both")
    other(B, rel)
    with pytest.raises(B.ArgumentError, match="setLogit|setCounts"):
        mine(B, rel)
    assert rel.model.pg["model"] != which
    # relation features, a sampled precision
    rel = fresh()
    rel.F = np.ones((40, 2))
    with pytest.raises(B.ArgumentError, match="features"):
        mine(B, rel)
    rel = fresh()
    rel.model.alpha_sample = True
    with pytest.raises(B.ArgumentError, match="alpha_sample"):
        mine(B, rel)
    assert rel.model.pg is None
    theirs = {
        "probit": lambda r: B.setProbit(r),
        "censored": lambda r: B.setCensored(r, np.zeros(40, dtype=int)),
        "interval": lambda r: B.setInterval(r, r.data.values - 1.0, r.data.values + 1.0),
        "binned": lambda r: B.setBinned(r, [0.5, 1.5, 2.5]),
        "ordinal": lambda r: B.setOrdinal(r),
        "robust": lambda r: B.setRobust(r, 4.0),
        "weights": lambda r: B.setWeights(r, np.ones(40)),
        "waic": lambda r: B.setWaic(r),
    }
    for kind, setter in theirs.items():
        base = "both" if kind == "probit" else kind
        r = fresh(base)
        setter(r)
        with pytest.raises(B.ArgumentError, match="not scored yet" if kind == "waic" else None):
            mine(B, r)
        assert r.model.pg is None, kind
        r = fresh(base)
        if kind == "ordinal" and which == "logit":                 # (levels 1 .. 5 are no 0/1 values: the other order is the test)
            continue
        mine(B, r)
        with pytest.raises(B.ArgumentError, match="not scored yet" if kind == "waic" else None):
            setter(r)
        m = r.model
        assert m.probit is False and m.censor is None and m.interval is None and m.ordinal is None and m.robust is None \
            and m.weights is None and m.waic is None, kind


@pytest.mark.parametrize("which", ["logit", "counts"])
def test_samplers_refuse_what_the_model_does_not_cover(B, which):
    from bdf_amd.relation_data import check_pg
    rel = _relation(B, which, test=np.arange(1, 6))
    SETTERS[which](B, rel)
    rd = B.RelationData(rel)
    with pytest.raises(B.ArgumentError):
        B.bpmf_vb(rd, num_latent=4, verbose=False, niter=1)
    with pytest.raises(B.ArgumentError):
        B.macau_hmc(rd, num_latent=4, verbose=False, burnin=1, psamples=1)
    with pytest.raises(B.ArgumentError, match="one rank"):
        B.GibbsEngine(rd, 4, shard=(0, 2))
    with pytest.raises(B.ArgumentError, match="not scored yet"):
        B.macau(rd, num_latent=4, burnin=1, psamples=1, verbose=False, lpd=True)
    with pytest.raises(B.ArgumentError, match="all elements"):
        B.macau(rd, num_latent=4, burnin=1, psamples=1, verbose=False, full_prediction=True)
    # changed behind the setter's back: the engine looks again (check_pg)
    for attr, val, pat in (("waic", {"pointwise": False}, "WAIC"), ("robust", {"nu": 4.0}, "setRobust"), ("weights", np.ones(35), "setWeights"),
                           ("censor", np.zeros(35, dtype=np.int8), "setCensored"), ("probit", True, "probit")):
        keep = getattr(rel.model, attr)
        setattr(rel.model, attr, val)
        with pytest.raises(B.ArgumentError, match=pat):
            B.GibbsEngine(rd, 4)
        setattr(rel.model, attr, keep)
    rel.F = np.ones((35, 2))
    with pytest.raises(B.ArgumentError, match="features"):
        B.GibbsEngine(rd, 4)
    rel.F = None
    rel.model.alpha_sample = True
    with pytest.raises(B.ArgumentError, match="alpha_sample"):
        check_pg(rel)
    rel.model.alpha_sample = False
    rel.model.alpha = 2.0
    with pytest.raises(B.ArgumentError, match="alpha"):
        check_pg(rel)
    rel.model.alpha = 1.0
    rel.data.values[3] = 0.5
    with pytest.raises(B.ArgumentError):
        check_pg(rel)
    rel.data.values[3] = 1.0
    if which == "counts":
        rel.model.pg["r"] = 2.5
        with pytest.raises(B.ArgumentError, match="r ="):
            check_pg(rel)
        rel.model.pg["r"] = 3
    check_pg(rel)


def test_tostr_names_the_model_and_leaves_the_others_alone(B):
    rel = _relation(B, "logit")
    assert B.toStr(rel) == "play[α=2.0]"
    B.setLogit(rel)
    assert B.toStr(rel) == "play[logit]"
    rel = _relation(B)
    B.setCounts(rel, 5)
    assert B.toStr(rel) == "play[nb:5]"


# ---- the stream -------------------------------------------------------------------------------------------------------------------
def test_stream_purpose_is_defined_and_unused_by_others():
    h = open(os.path.join(ROOT, "include", "bdf.h")).read()
    purposes = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (BDF_P_[A-Z0-9_]+)\s+(\d+)", h)}
    assert purposes["BDF_P_PG"] == 18
    assert len(set(purposes.values())) == len(purposes)           # no two purposes share a number
    from bdf_amd import _lib
    assert _lib.P_PG == PG.P_PG == 18


def test_vectorised_draw_is_the_scalar_sampler_on_the_oracles_streams(O):
    """pg() draws one observation at a time from oracle.draw and oracle.normals, line for line as the header; draw_pg must give the
    same numbers and the same decision margins: every branch of the sampler (the exponential tail, both truncated inverse
    Gaussians, the normal above b = 170) and the extremes of psi"""
    rng = np.random.default_rng(1)
    psi = np.concatenate([rng.uniform(-8.0, 8.0, 150), [0.0, 1e-8, -1e-8, 40.0, -40.0, 12.0, 3.2, 100.0, -2000.0, 1e4, 3.1, -3.1]])
    b = np.concatenate([rng.integers(1, 12, 150), [1, 2, 3, 1, 7, 171, 170, 1, 3, 2, 1e4, 1e6]]).astype(float)
    rows = np.concatenate([np.arange(160), [2 ** 33 + 5, 2 ** 20]])
    for seed, sweep, tag in ((1234, 3, 1), (2 ** 40 + 7, 77, 3)):
        w, mg = PG.draw_pg(psi, b, seed, sweep, tag, rows=rows)
        for k in range(len(psi)):
            x, m = PG.pg(b[k], psi[k], PG.Cursor(seed, sweep, tag, int(rows[k])))
            assert abs(x - w[k]) <= 1e-13 * x and (m == mg[k] or abs(m - mg[k]) <= 1e-9 * m), (k, x, w[k], m, mg[k])
        assert np.all(np.isfinite(w)) and np.all(w > 0.0)


# ---- csrc/pg.h on the host --------------------------------------------------------------------------------------------------------
_HOST_SRC = r'''
#include <cstdio>
#include <cstdint>
#include <cmath>
#include "pg.h"
// the library's counter layout on a Philox4x32-10 of its own, with libm's log and cos
struct Cur {
    uint64_t seed, row; uint32_t sweep, entity, pair;
    void block(double &u1, double &u2) {
        uint32_t c[4] = {(uint32_t)row, (uint32_t)((row >> 32) & 0xffffu) | ((pair++ & 0xffffu) << 16), sweep, (18u << 24) | (entity & 0xffffffu)};
        uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
        for (int r = 0; r < 10; r++) {
            uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
            uint32_t n[4] = {(uint32_t)(p1 >> 32) ^ c[1] ^ k0, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ c[3] ^ k1, (uint32_t)p0};
            for (int i = 0; i < 4; i++) c[i] = n[i];
            k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
        }
        u1 = ((double)((((uint64_t)c[1] << 32) | c[0]) >> 11) + 0.5) * 0x1.0p-53;
        u2 = ((double)((((uint64_t)c[3] << 32) | c[2]) >> 11) + 0.5) * 0x1.0p-53;
    }
    double uniform() { double a, b; block(a, b); return a; }
    double expo() { return -log(uniform()); }
    void expo2(double &E, double &F) { double a, b; block(a, b); E = -log(a); F = -log(b); }
    double normal() { double a, b; block(a, b); return sqrt(-2.0 * log(a)) * cos(6.283185307179586476925286766559 * b); }
};
int main() {
    int k; double x[6];
    while (scanf("%d %lf %lf %lf %lf %lf %lf", &k, x, x + 1, x + 2, x + 3, x + 4, x + 5) == 7) {
        double o[3] = {0.0, 0.0, 0.0};
        if (k == 0) { o[0] = bdf_pg_b((int)x[0], x[1], x[2]); o[1] = bdf_pg_kappa((int)x[0], x[1], x[2]); o[2] = bdf_pg_linear(x[3], x[1], o[1], x[4]); }
        else if (k == 1) { o[0] = bdf_pg_logistic(x[0]); o[1] = bdf_pg_count_mean(x[0], x[1]); }
        else if (k == 2) bdf_pg_moments(x[0], x[1], o[0], o[1]);
        else if (k == 3) o[0] = bdf_pg_coef((int)x[0], x[1]);
        else if (k == 4) { const bdf_pg_tilt w = bdf_pg_tilt_of(x[0]); o[0] = w.K; o[1] = w.p; o[2] = w.q; }
        else { Cur c = {(uint64_t)x[2], (uint64_t)x[5], (uint32_t)x[3], 0x800000u | (uint32_t)x[4], 0u}; o[0] = bdf_pg_omega(x[0], x[1], c); o[1] = c.pair; }
        printf("%.17g %.17g %.17g\n", o[0], o[1], o[2]);
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def header():
    """csrc/pg.h compiled for the host where a C++ compiler is at hand (csrc/Makefile's, as a host compiler, when there is no other):
    -> run(lines of (kind, six numbers)) -> (len(lines), 3) values"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cxx = [shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")]
    if cxx[0] is None:
        cxx = [hipcc, "-x", "c++"]
    td = tempfile.mkdtemp()
    open(os.path.join(td, "t.cpp"), "w").write(_HOST_SRC)
    subprocess.run(cxx + ["-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "bayesiandatafusion.jl_amd", "csrc"), os.path.join(td, "t.cpp"),
                          "-o", os.path.join(td, "t")], check=True)

    def run(lines):
        text = "".join("%d %.17g %.17g %.17g %.17g %.17g %.17g\n" % tuple(t) for t in lines)
        out = subprocess.run([os.path.join(td, "t")], input=text, capture_output=True, text=True, check=True).stdout
        return np.array([float(t) for t in out.split()]).reshape(len(lines), 3)

    yield run
    shutil.rmtree(td, ignore_errors=True)


def test_header_and_restatement_state_the_same_scalar_maps(header):
    rng = np.random.default_rng(2)
    n = 400
    y = rng.integers(0, 50, n).astype(float)
    r = rng.integers(1, 9, n).astype(float)
    mean, om = rng.standard_normal(n), np.exp(rng.uniform(-9.0, 3.0, n))
    for model in (1, 2):
        yy = (y % 2) if model == 1 else y
        got = header([(0, model, yy[k], r[k], mean[k], om[k], 0) for k in range(n)])
        kap = PG.kappa_of(model, yy, r)
        assert np.array_equal(got[:, 0], PG.b_of(model, yy, r)) and np.array_equal(got[:, 1], kap)
        np.testing.assert_allclose(got[:, 2], PG.linear_of(mean, yy, kap, om), rtol=1e-15, atol=0)
    psi = np.concatenate([rng.uniform(-50.0, 50.0, n - 6), [0.0, -0.0, 800.0, -800.0, 700.0, 745.0]])
    got = header([(1, psi[k], r[k], 0, 0, 0, 0) for k in range(n)])
    np.testing.assert_allclose(got[:, 0], PG.link(1, psi), rtol=1e-15, atol=0)
    np.testing.assert_allclose(got[:, 1], PG.link(2, psi, r), rtol=1e-14, atol=0)
    assert np.all(np.isfinite(got)) and got[n - 4, 0] == 1.0 and got[n - 3, 0] == 0.0
    a = np.concatenate([10.0 ** rng.uniform(-10.0, 3.0, n - 4), [0.0, PG.SERIES_BELOW, np.nextafter(PG.SERIES_BELOW, 0.0), 1e4]])
    got = header([(2, 171.0 + k, a[k], 0, 0, 0, 0) for k in range(n)])
    m, v = PG.moments(171.0 + np.arange(n), a)
    np.testing.assert_allclose(got[:, 0], m, rtol=1e-14)
    np.testing.assert_allclose(got[:, 1], v, rtol=1e-14)
    assert got[n - 4, 0] == (171.0 + n - 4) / 4.0 and abs(got[n - 4, 1] - (171.0 + n - 4) / 24.0) <= 1e-15 * got[n - 4, 1]
    x = np.concatenate([10.0 ** rng.uniform(-4.0, 1.5, n - 2), [PG.T, np.nextafter(PG.T, 1.0)]])
    for nn in (0, 1, 2, 5):
        got = header([(3, nn, x[k], 0, 0, 0, 0) for k in range(n)])
        np.testing.assert_allclose(got[:, 0], PG.coef(nn, x), rtol=1e-13, atol=1e-300)
    z = np.concatenate([rng.uniform(0.0, 30.0, n - 5), [0.0, 5e-9, 1.0 / PG.T, 1000.0, 5000.0]])
    got = header([(4, z[k], 0, 0, 0, 0, 0) for k in range(n)])
    K, p, q = PG.tilt(z)
    np.testing.assert_allclose(got[:, 0], K, rtol=1e-15)
    np.testing.assert_allclose(got[:, 1], p, rtol=1e-13, atol=1e-300)
    np.testing.assert_allclose(got[:, 2], q, rtol=1e-12, atol=1e-300)      # (two erfc implementations)


def test_header_draws_what_the_restatement_draws(header):
    """the header's sampler on a host cursor against draw_pg on the same streams: every observation whose decisions were not close
    calls (margin above 1e-6: all but a few in a million) to 1e-12, and none may differ by more than a flipped decision explains"""
    rng = np.random.default_rng(5)
    n = 3000
    psi = np.concatenate([rng.uniform(-9.0, 9.0, n - 8), [0.0, 1e-8, 40.0, -40.0, 100.0, -2000.0, 1e4, -1e4]])
    b = np.concatenate([rng.integers(1, 30, n - 8), [1, 1, 1, 2, 1, 3, 1, 171]]).astype(float)
    b[:40] = [169, 170, 171, 172] * 10
    w, mg = PG.draw_pg(psi, b, 991, 4, 2)
    got = header([(5, b[k], psi[k], 991, 4, 2, k) for k in range(n)])[:, 0]
    ok = mg > 1e-6
    assert ok.sum() >= n - 3
    np.testing.assert_allclose(got[ok], w[ok], rtol=1e-12)
    assert np.all(np.isfinite(got)) and np.all(got > 0.0)


def test_values_outside_the_contract_still_give_finite_outputs(header):
    """bdf.h promises a finite, positive omega and a finite linear_out for every finite value: a stored count that is negative or no
    integer, which only the bare C ABI lets through, takes b held at 1 (and its integer part) instead of an empty sum"""
    y = np.array([-1.0, -7.0, -1e9, 0.5, 2.5, -0.5])
    got = header([(0, 2, v, 1.0, 0.0, 1.0, 0) for v in y])
    assert np.array_equal(got[:, 0], np.maximum(y + 1.0, 1.0))
    for v, b in zip(y, got[:, 0]):
        w = header([(5, b, 0.3, 7, 2, 1, 0)])[0, 0]
        lin = header([(0, 2, v, 1.0, 0.25, w, 0)])[0, 2]
        assert np.isfinite(w) and w > 0.0 and np.isfinite(lin), (v, b, w, lin)


# ---- the law of PG(b, c) ------------------------------------------------------------------------------------------------------------
def _laplace1(b, c):
    """E exp(-omega) for omega ~ PG(b, c): (cosh(c / 2) / cosh(sqrt((c^2 / 2 + 1) / 2)))^b, through logarithms"""
    lc = lambda x: abs(x) + np.log1p(np.exp(-2.0 * abs(x))) - np.log(2.0)
    return float(np.exp(b * (lc(c / 2.0) - lc(np.sqrt((c * c / 2.0 + 1.0) / 2.0)))))


@pytest.mark.parametrize("c", [0.0, 1e-8, 0.7, 3.0, 12.0, 60.0])
@pytest.mark.parametrize("b", [1, 2, 7, 170])
def test_pg_has_the_right_law(b, c):
    """20,000 draws (one observation over 20,000 sweeps) against PG(b, c)'s closed forms: the mean b / (2c) tanh(c / 2), the variance
    b / (4 c^3) (sinh c - c) sech^2(c / 2) and the Laplace transform at 1.  Bounds: 5 standard errors -- of the sample mean; of the
    sample variance, (mu4 - sigma^4) / n with mu4 estimated from the sample; of the mean of exp(-omega), from its sample variance."""
    n = 20000
    w, _ = PG.draw_pg(np.full(n, c), np.full(n, float(b)), 77 + b, np.arange(1, n + 1), 2, rows=np.full(n, 11))
    assert np.all(w > 0) and np.all(np.isfinite(w))
    if c < 1e-4:
        mean, var = b / 4.0, b / 24.0
    else:
        mean = b / (2.0 * c) * np.tanh(c / 2.0)
        var = b / (4.0 * c ** 3) * (np.sinh(c) - c) / np.cosh(c / 2.0) ** 2
    d = w - w.mean()
    mu4 = np.mean(d ** 4)
    print(f"PG({b}, {c}): mean {(w.mean() - mean) / np.sqrt(var / n):+.2f} se, variance ratio {w.var(ddof=1) / var:.4f}")
    assert abs(w.mean() - mean) <= 5.0 * np.sqrt(var / n)
    assert abs(w.var(ddof=1) - var) <= 5.0 * np.sqrt(max(mu4 - var ** 2, 0.0) / n)
    e = np.exp(-w)
    assert abs(e.mean() - _laplace1(b, c)) <= 5.0 * np.sqrt(e.var(ddof=1) / n)


def test_normal_branch_has_the_moments_of_pg_in_extended_precision(header):
    """b = 171: m and v as the header and the restatement evaluate them against the closed forms in extended precision, at |c| from
    1e-10 to 1e3 across the switch to the series at 0.25: 1e-12 relative"""
    a = np.concatenate([10.0 ** np.linspace(-10.0, 3.0, 131), [PG.SERIES_BELOW, np.nextafter(PG.SERIES_BELOW, 0.0), np.nextafter(PG.SERIES_BELOW, 1.0),
                                                               0.2, 0.24, 0.26, 0.3, 0.5]])
    b = 171.0
    try:
        from mpmath import mp, mpf
        with mp.workdps(60):
            em = [float(mpf(b) / (2 * mpf(x)) * mp.tanh(mpf(x) / 2)) for x in a]
            ev = [float(mpf(b) / (4 * mpf(x) ** 3) * (mp.sinh(mpf(x)) - mpf(x)) * mp.sech(mpf(x) / 2) ** 2) for x in a]
    except ImportError:
        L = np.longdouble
        x = a.astype(L)
        e = np.exp(-x)
        em = (L(b) / (2 * x) * (-np.expm1(-x)) / (1 + e)).astype(np.float64)
        # (sinh x - x) by its series below 1 (no cancellation), sech^2 in terms of e^-x
        ser = sum(x ** (2 * k) / L(math.factorial(2 * k + 3)) for k in range(12))
        big = ((1 - e * e) / 2 - x * e) / x ** 3
        ev = (L(b) / 4 * np.where(x < 1, ser * e, big) * 4 / (1 + e) ** 2).astype(np.float64)
    em, ev = np.asarray(em), np.asarray(ev)
    m, v = PG.moments(b, a)
    got = header([(2, b, x, 0, 0, 0, 0) for x in a])
    for name, val, ex in (("m", m, em), ("v", v, ev), ("header m", got[:, 0], em), ("header v", got[:, 1], ev)):
        err = np.abs(val - ex) / ex
        print(f"{name}: worst relative error {err.max():.2e} at |c| = {a[int(np.argmax(err))]:.3g}")
        assert err.max() <= 1e-12, name
    # and the branch's draw is that normal
    w, _ = PG.draw_pg(np.array([1.3]), np.array([171.0]), 5, 9, 1)
    z = PG.Cursor(5, 9, 1, 0).normal()
    mm, vv = PG.moments(171.0, 1.3)
    assert w[0] == max(float(mm) + float(np.sqrt(vv)) * z, PG.TINY)


@pytest.mark.parametrize("b", [1.0, 3.0, 170.0, 171.0, 1e6])
def test_omega_is_finite_and_positive_at_the_extremes(header, b):
    psi = np.array([0.0, 1e-8, -1e-8, 40.0, -40.0, 100.0, -100.0, 2000.0, -2000.0, 1e4, -1e4])
    w, _ = PG.draw_pg(psi, np.full(len(psi), b), 3, 8, 1)
    got = header([(5, b, psi[k], 3, 8, 1, k) for k in range(len(psi))])[:, 0]
    for x in (w, got):
        assert np.all(np.isfinite(x)) and np.all(x > 0.0)
        for model, y in ((1, 1.0), (1, 0.0), (2, 0.0), (2, b)):
            lin = PG.linear_of(0.3, y, PG.kappa_of(model, y, 5), x)
            assert np.all(np.isfinite(lin))
    np.testing.assert_allclose(got, w, rtol=1e-9)
    assert np.array_equal(w, PG.draw_pg(-psi, np.full(len(psi), b), 3, 8, 1)[0])      # the draw sees |psi| alone


# ---- the sweep leaves the exact posterior invariant -----------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [1, 2])
def test_the_sweep_leaves_the_exact_posterior_invariant(O, model):
    """One row u with D = 1 and three cells with the other side's factors v_k fixed, u ~ N(0, 1 / lambda): omega | u from the
    restatement's pg() and u | omega from its Gaussian conditional, alternated for 50,000 sweeps.  The mean and the variance of u
    against the exact posterior (the likelihood times the prior by quadrature on a grid), within 5 Monte-Carlo standard errors from
    the means of 50 batches of 1,000 sweeps."""
    v = np.array([1.0, -0.7, 1.6])
    offset, lam, r = 0.3, 0.8, 1
    y = np.array([1.0, 0.0, 1.0]) if model == 1 else np.array([0.0, 2.0, 1.0])
    bb, kappa = PG.b_of(model, y, r), PG.kappa_of(model, y, r)
    # the exact posterior: prod_k e^(a_k psi_k) / (1 + e^psi_k)^b_k, a = y
    g = np.linspace(-14.0, 14.0, 56001)
    psi = g[:, None] * v[None, :] + offset
    lp = -0.5 * lam * g * g + (y[None, :] * psi - bb[None, :] * np.logaddexp(0.0, psi)).sum(axis=1)
    wq = np.exp(lp - lp.max())
    wq /= wq.sum()
    mean = float((wq * g).sum())
    var = float((wq * (g - mean) ** 2).sum())
    n, rng = 50000, np.random.default_rng(12 + model)
    zs = rng.standard_normal(n)
    us = np.zeros(n)
    u = 0.0
    for it in range(n):
        om = np.array([PG.pg(bb[k], u * v[k] + offset, PG.Cursor(2024, it + 1, 1, k))[0] for k in range(3)])
        P = lam + float((om * v * v).sum())
        u = float((v * (kappa - om * offset)).sum()) / P + zs[it] / np.sqrt(P)
        us[it] = u
    bm = us.reshape(50, 1000).mean(axis=1)
    bv = ((us - mean) ** 2).reshape(50, 1000).mean(axis=1)
    se_m, se_v = bm.std(ddof=1) / np.sqrt(50), bv.std(ddof=1) / np.sqrt(50)
    print(f"model {model}: mean {us.mean():.4f} (exact {mean:.4f}, {abs(us.mean() - mean) / se_m:.2f} se), "
          f"variance {bv.mean():.4f} (exact {var:.4f}, {abs(bv.mean() - var) / se_v:.2f} se)")
    assert abs(us.mean() - mean) <= 5.0 * se_m
    assert abs(bv.mean() - var) <= 5.0 * se_v


# ---- the build's listing ------------------------------------------------------------------------------------------------------------
def test_pg_kernels_use_no_scratch():
    res = _resources("k_pg")
    draws = {k: v for k, v in res.items() if "k_pg_draw" in k}
    links = {k: v for k, v in res.items() if "k_predict_logit" in k or "k_predict_count" in k}
    assert len(draws) == 9 and len(links) == 18
    for k, v in {**draws, **links}.items():
        assert v[1] == 0 and v[2] >= 2, (k, v)
    assert draws["9k_pg_drawILi2ELi4ELi1EEEvNS_6PgArgsE"][2] >= 3            # two modes, D <= 32: the MovieLens draw
    path = os.path.join(ROOT, "bayesiandatafusion.jl_amd", "csrc", "k_pg.o.res")
    name, spills = None, {}
    for line in open(path):
        m = re.search(r"remark: \s*(Function Name|VGPRs Spill): (\S+)", line)
        if m and m.group(1) == "Function Name":
            name = m.group(2)
        elif m and name:
            spills[name] = int(m.group(2))
    assert len(spills) >= 27 and not any(spills.values()), spills
