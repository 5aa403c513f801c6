"""The per-row noise model on the host (no GPU): setEntityNoise and what it guards in both orders, noise_kind and
the one-rank refusal, the stream purposes in include/bdf.h, the restated gamma variates of tests/entity_noise_restatement.py against
the oracle's Philox and against the law tau must follow, csrc/entity_noise.h compiled for the host against the restatement, and the
resource listings the build leaves for the new kernels."""
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import entity_noise_restatement as ER
from test_probit_host import _resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bayesiandatafusion.jl_amd", "csrc")


def _relation(B, n=40, test=None, alpha=2.0, names=("u", "v"), dims=(8, 6), values=None):
    rng = np.random.default_rng(3)
    table = {nm: rng.integers(1, d + 1, n) for nm, d in zip(names, dims)}
    if len(dims) == 2:                                   # distinct cells (setBackground refuses a cell listed twice)
        cells = rng.choice(dims[0] * dims[1], size=n, replace=False)
        table = {names[0]: cells // dims[1] + 1, names[1]: cells % dims[1] + 1}
    table["y"] = rng.standard_normal(n) if values is None else values
    rel = B.Relation(table, "ratings", [B.Entity(nm) for nm in names], alpha=alpha, dims=list(dims))
    if test is not None:
        B.assignToTest(rel, test)
    return rel


# ---- the setter ---------------------------------------------------------------------------------------------------------------
def test_default_has_none_and_the_setter_stores_its_spec(B):
    rel = _relation(B)
    assert rel.model.entity_noise is None
    rel._dev = object()
    assert B.setEntityNoise(rel, rel.entities[1]) is None
    assert rel.model.entity_noise == {"mode": 2, "shape": 2.0, "rate": 2.0} and rel._dev is None
    B.setEntityNoise(rel, "u", shape=0.5, rate=3)
    assert rel.model.entity_noise == {"mode": 1, "shape": 0.5, "rate": 3.0}
    B.setEntityNoise(rel, 2, 1.5, 0.25)
    assert rel.model.entity_noise == {"mode": 2, "shape": 1.5, "rate": 0.25}
    B.setEntityNoise(rel, np.int64(1))
    assert rel.model.entity_noise["mode"] == 1
    rel3 = _relation(B, names=("a", "b", "c"), dims=(8, 6, 4))
    B.setEntityNoise(rel3, "c")
    assert rel3.model.entity_noise["mode"] == 3
    assert B.toStr(rel3) == "rati[α=2.0 τ:c]" and B.toStr(rel) == "rati[α=2.0 τ:u]"


@pytest.mark.parametrize("bad", [0, 3, -1, "w", None, 1.0, True, "", ["u"]])
def test_the_setter_refuses_what_is_no_entity_of_the_relation(B, bad):
    rel = _relation(B)
    with pytest.raises(B.ArgumentError, match="entity"):
        B.setEntityNoise(rel, bad)
    with pytest.raises(B.ArgumentError, match="entity"):
        B.setEntityNoise(rel, B.Entity("u"))                        # an entity of that name, but not the relation's
    assert rel.model.entity_noise is None


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), float("inf"), "2", None, True])
def test_the_setter_refuses_a_shape_or_rate_that_is_not_positive_and_finite(B, bad):
    rel = _relation(B)
    with pytest.raises(B.ArgumentError, match="shape"):
        B.setEntityNoise(rel, 1, shape=bad)
    with pytest.raises(B.ArgumentError, match="rate"):
        B.setEntityNoise(rel, 1, rate=bad)
    assert rel.model.entity_noise is None


def test_it_works_before_and_after_the_test_split(B):
    rel = _relation(B, test=np.arange(1, 6))
    B.setEntityNoise(rel, "v")
    rel2 = _relation(B)
    B.setEntityNoise(rel2, "v")
    B.assignToTest(rel2, np.arange(1, 6))
    assert rel.model.entity_noise == rel2.model.entity_noise == {"mode": 2, "shape": 2.0, "rate": 2.0}


# ---- what it excludes, in both orders -------------------------------------------------------------------------------------------
def _fresh(B, kind):
    if kind in ("probit", "logit"):
        return _relation(B, values=(np.arange(40) % 2).astype(np.float64))
    if kind == "counts":
        return _relation(B, values=(np.arange(40) % 7).astype(np.float64))
    if kind == "ordinal":
        return _relation(B, values=(np.arange(40) % 5 + 1).astype(np.float64))
    return _relation(B)


THEIRS = {
    "robust": (lambda B, r: B.setRobust(r, 4.0), "robust"),
    "weights": (lambda B, r: B.setWeights(r, np.full(40, 2.0)), "weights"),
    "probit": (lambda B, r: B.setProbit(r), "probit"),
    "censored": (lambda B, r: B.setCensored(r, np.zeros(40, dtype=int)), "censor"),
    "interval": (lambda B, r: B.setInterval(r, r.data.values - 1.0, r.data.values + 1.0), "interval"),
    "binned": (lambda B, r: B.setBinned(r, [-1.0, 0.0, 1.0]), "interval"),
    "ordinal": (lambda B, r: B.setOrdinal(r), "ordinal"),
    "logit": (lambda B, r: B.setLogit(r), "pg"),
    "counts": (lambda B, r: B.setCounts(r, 3), "pg"),
    "background": (lambda B, r: B.setBackground(r, 0.1), "background"),
    "waic": (lambda B, r: B.setWaic(r), "waic"),
}


@pytest.mark.parametrize("kind", list(THEIRS))
def test_exclusions_in_both_orders(B, kind):
    setter, field = THEIRS[kind]
    empty = lambda r: getattr(r.model, field) is None or getattr(r.model, field) is False
    # theirs first: setEntityNoise is refused and leaves nothing
    r = _fresh(B, kind)
    setter(B, r)
    with pytest.raises(B.ArgumentError, match="setEntityNoise"):
        B.setEntityNoise(r, "u")
    assert r.model.entity_noise is None and not empty(r)
    # setEntityNoise first: theirs is refused, names it and leaves nothing
    r = _fresh(B, kind)
    B.setEntityNoise(r, "u")
    with pytest.raises(B.ArgumentError, match="setEntityNoise"):
        setter(B, r)
    assert empty(r) and r.model.entity_noise is not None


def test_waic_and_the_noise_model_say_not_scored_yet(B):
    r = _relation(B)
    B.setWaic(r)
    with pytest.raises(B.ArgumentError, match="not scored yet"):
        B.setEntityNoise(r, "u")
    r = _relation(B)
    B.setEntityNoise(r, "u")
    with pytest.raises(B.ArgumentError, match="not scored yet"):
        B.setWaic(r)
    B.setWaic(r, on=False)                                          # taking it back is no request to score


def test_relation_features_in_both_orders(B):
    from bdf_amd.relation_data import check_entity_noise, check_model
    r = _relation(B)
    r.F = np.ones((40, 2))
    with pytest.raises(B.ArgumentError, match="features"):
        B.setEntityNoise(r, "u")
    r = _relation(B)
    B.setEntityNoise(r, "u")
    r.F = np.ones((40, 2))                                          # (features are a field, not a setter: the sampler's check finds them)
    with pytest.raises(B.ArgumentError, match="features"):
        check_entity_noise(r)
    with pytest.raises(B.ArgumentError, match="features"):
        check_model(r)


# ---- noise_kind, check_model ----------------------------------------------------------------------------------------------------
def test_noise_kind_and_the_one_rank_refusal(B):
    from bdf_amd.relation_data import check_entity_noise, check_model, noise_kind
    rel = _relation(B)
    assert noise_kind(rel) == "gauss"
    B.setEntityNoise(rel, "v")
    assert noise_kind(rel) == "entity_noise"
    assert check_model(rel) is None and check_model(rel, world=1) is None and noise_kind(rel) == "entity_noise"
    with pytest.raises(B.ArgumentError) as e:
        check_model(rel, world=2)
    assert str(e.value) == "Relation ratings has a noise precision per row: one rank only"
    with pytest.raises(B.ArgumentError, match="one rank"):
        B.GibbsEngine(B.RelationData(rel), 4, shard=(0, 2))
    # changed behind the setter's back: the check looks again, and raises what check_model raises
    for spoil in ({"mode": 3, "shape": 2.0, "rate": 2.0}, {"mode": 1, "shape": 0.0, "rate": 2.0}, {"mode": 1, "shape": 2.0, "rate": float("nan")}, {"mode": 1}):
        rel.model.entity_noise = spoil
        with pytest.raises(B.ArgumentError) as e1:
            check_entity_noise(rel)
        with pytest.raises(B.ArgumentError) as e2:
            check_model(rel)
        assert str(e1.value) == str(e2.value)
    rel.model.entity_noise = {"mode": np.int64(2), "shape": 3, "rate": 1}
    check_model(rel)
    assert rel.model.entity_noise == {"mode": 2, "shape": 3.0, "rate": 1.0}
    rel.model.robust = {"nu": 4.0}
    with pytest.raises(B.ArgumentError, match="setRobust"):
        check_model(rel)


def test_the_two_mode_trainers_refuse_it(B):
    rel = _relation(B, test=np.arange(1, 6))
    B.setEntityNoise(rel, "v")
    rd = B.RelationData(rel)
    with pytest.raises(B.ArgumentError, match="per row"):
        B.bpmf_vb(rd, num_latent=4, verbose=False, niter=1)
    with pytest.raises(B.ArgumentError, match="per row"):
        B.macau_hmc(rd, num_latent=4, verbose=False, burnin=1, psamples=1)


# ---- the streams --------------------------------------------------------------------------------------------------------------
def test_stream_purposes_are_defined_and_unused_by_others():
    h = open(os.path.join(ROOT, "include", "bdf.h")).read()
    purposes = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (BDF_P_[A-Z0-9_]+)\s+(\d+)", h)}
    assert purposes["BDF_P_NOISE_N"] == 19 and purposes["BDF_P_NOISE_U"] == 20
    assert len(set(purposes.values())) == len(purposes)           # no two purposes share a number
    from bdf_amd import _lib
    assert (_lib.P_NOISE_N, _lib.P_NOISE_U) == (ER.P_NOISE_N, ER.P_NOISE_U) == (19, 20)


def test_vectorised_gamma_is_marsaglia_tsang_on_the_oracles_streams(O):
    """gamma_mt draws one variate at a time from oracle.draw and oracle.normals; gamma_variates must be the same numbers, on either
    side of shape 1 and with a shape per row"""
    rows = np.array([0, 1, 2, 5, 17, 1002, 2 ** 33 + 5])
    for seed, sweep, tag, a in ((1234, 3, 1, 1.0), (91, 1, 2, 2.5), (2 ** 40 + 7, 77, 3, 152.0), (5, 9, 1, 0.5), (5, 9, 2, 0.01), (6, 2, 1, 0.999)):
        got = ER.gamma_variates(seed, sweep, tag, rows, a)
        want = np.array([ER.gamma_mt(seed, sweep, tag, int(r), a) for r in rows])
        np.testing.assert_allclose(got, want, rtol=1e-13)
        assert np.all(got > 0) and np.all(np.isfinite(got))
    shapes = np.array([0.5, 1.0, 1.5, 2.0, 5.5, 0.25, 152.0])
    got = ER.gamma_variates(77, 4, 2, rows, shapes)
    want = np.array([ER.gamma_mt(77, 4, 2, int(r), float(a)) for r, a in zip(rows, shapes)])
    np.testing.assert_allclose(got, want, rtol=1e-13)
    # and neither sample_alpha's stream nor the robust model's: the same (entity, row, shape) gives other numbers there
    import robust_restatement as RR
    assert abs(O.gamma(1234, 3, 0x800000 | 1, 0, 2.5) - ER.gamma_mt(1234, 3, 1, 0, 2.5)) > 1e-6
    assert abs(RR.gamma_mt(1234, 3, 1, 0, 2.5) - ER.gamma_mt(1234, 3, 1, 0, 2.5)) > 1e-6


MOMENT_CASES = [(2.0, 2.0, 0, 0.0), (2.0, 2.0, 1, 0.3), (2.0, 2.0, 300, 50.0), (0.5, 2.0, 0, 0.0)]


@pytest.mark.parametrize("shape,rate,n_j,S_j", MOMENT_CASES)
def test_tau_has_the_right_law(shape, rate, n_j, S_j):
    """tau_j | U, V, alpha ~ Gamma(a = shape + n_j / 2, b = rate + alpha S_j / 2): mean a / b, variance a / b^2; one row over 2e5
    sweeps.  Bounds: 4 standard errors of the sample mean, and of the sample variance (whose variance is (mu4 - sigma^4) / n with
    the gamma's fourth central moment mu4 = 3 a (a + 2) / b^4).  The last case draws from a prior of shape 1/2: the boost branch."""
    n, alpha = 200_000, 1.7
    a, b = shape + 0.5 * n_j, rate + 0.5 * alpha * S_j
    G = ER.gamma_variates(77, np.arange(1, n + 1), 2, np.full(n, 11), a)
    tau = ER.draw_tau(G, S_j, alpha, rate)
    mean, var = a / b, a / b ** 2
    assert np.all(tau > 0) and np.all(np.isfinite(tau))
    assert abs(tau.mean() - mean) <= 4.0 * np.sqrt(var / n), (tau.mean(), mean)
    mu4 = 3.0 * a * (a + 2.0) / b ** 4
    assert abs(tau.var(ddof=1) - var) <= 4.0 * np.sqrt((mu4 - var ** 2) / n), (tau.var(ddof=1), var)


def test_taus_is_the_draw_row_by_row():
    """taus (what run_chain and the GPU tests call) against the definition written out: per row its cells, their sum of squares, the
    row's own gamma variate of shape + n_j / 2; a row without cells draws from the prior; wsse = sum_j tau_j S_j"""
    rng = np.random.default_rng(12)
    N, n = 9, 60
    rows0 = rng.integers(0, N, n)
    rows0[rows0 == 4] = 5                                   # row 4 has no cell
    e = rng.standard_normal(n)
    tau, omega, wsse, S = ER.taus(31, 7, 3, rows0, N, e, 1.3, 0.5, 2.0)
    for j in range(N):
        sel = rows0 == j
        Sj = float(np.sum(e[sel] ** 2))
        G = ER.gamma_mt(31, 7, 3, j, 0.5 + 0.5 * sel.sum())
        assert abs(S[j] - Sj) <= 1e-15 * max(Sj, 1.0)
        assert abs(tau[j] - G / (2.0 + 0.5 * 1.3 * Sj)) <= 1e-13 * tau[j]
    assert S[4] == 0.0 and abs(tau[4] - ER.gamma_mt(31, 7, 3, 4, 0.5) / 2.0) <= 1e-13 * tau[4]
    assert np.array_equal(omega, tau[rows0]) and abs(wsse - np.sum(tau * S)) <= 1e-12 * wsse


# ---- the header -----------------------------------------------------------------------------------------------------------------
def test_header_and_restatement_state_the_same_map():
    """csrc/entity_noise.h, the text the kernel forms tau with, compiled for the host (as test_lpd_host.py compiles lpd.h) against
    draw_tau and the shape rule: the same three operations in the same order, so the same bits"""
    cxx = [shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")]
    if cxx[0] is None:
        cxx = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "c++"]
    src = r'''
        #include <cstdio>
        #include "entity_noise.h"
        int main() { int n; if (scanf("%d", &n) != 1) return 1;
                     for (int i = 0; i < n; i++) { double G, rate, alpha, S, shape; long long nj;
                         if (scanf("%lf %lf %lf %lf %lf %lld", &G, &rate, &alpha, &S, &shape, &nj) != 6) return 1;
                         const double tau = bdf_entity_noise_tau(G, rate, alpha, S);
                         printf("%.17g %.17g %.17g\n", tau, bdf_entity_noise_term(tau, S), bdf_entity_noise_shape(shape, nj)); }
                     return 0; }
    '''
    rng = np.random.default_rng(21)
    n = 400
    G, rate, alpha = rng.gamma(3.0, size=n), np.exp(rng.uniform(-3, 3, n)), np.exp(rng.uniform(-4, 7, n))
    S, shape, nj = np.where(rng.random(n) < 0.2, 0.0, np.exp(rng.uniform(-6, 6, n))), np.exp(rng.uniform(-2, 2, n)), rng.integers(0, 20000, n)
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "t.cpp"), "w").write(src)
        subprocess.run(cxx + ["-O1", "-ffp-contract=off", "-I", CSRC, os.path.join(td, "t.cpp"), "-o", os.path.join(td, "t")], check=True)
        text = "%d\n" % n + "".join("%.17g %.17g %.17g %.17g %.17g %d\n" % t for t in zip(G, rate, alpha, S, shape, nj))
        out = subprocess.run([os.path.join(td, "t")], input=text, capture_output=True, text=True, check=True).stdout
    got = np.array([float(t) for t in out.split()]).reshape(n, 3)
    tau = ER.draw_tau(G, S, alpha, rate)
    assert np.array_equal(got[:, 0], tau) and np.array_equal(got[:, 1], tau * S) and np.array_equal(got[:, 2], shape + 0.5 * nj)


def test_header_writes_down_the_summation_order_of_both_widths():
    text = open(os.path.join(CSRC, "entity_noise.h")).read()
    assert "W = 8" in text and "W = 64" in text and "((p0 + p4) + (p2 + p6)) + ((p1 + p5) + (p3 + p7))" in text


# ---- the build's listings -------------------------------------------------------------------------------------------------------
def test_entity_noise_kernels_use_no_scratch():
    res = _resources("k_entity_noise")
    resid = {k: v for k, v in res.items() if "k_noise_resid" in k}
    rows = {k: v for k, v in res.items() if "k_noise_rows" in k}
    assert len(resid) == 9 and sorted(rows) == ["12k_noise_rowsILi64EEEvNS_13NoiseRowsArgsE", "12k_noise_rowsILi8EEEvNS_13NoiseRowsArgsE"]
    assert "13k_noise_finalEiPKdPd" in res
    for k, v in res.items():
        assert v[1] == 0 and v[2] >= 2, (k, v)
    assert resid["13k_noise_residILi2ELi4ELi1EEEvNS_14NoiseResidArgsE"][2] >= 3      # two modes, D <= 32: the MovieLens gather


def test_scaled_lpd_kernels_stand_beside_the_unscaled_ones():
    """k_lpd's nine shapes keep their unit (tests/test_lpd_host.py pins its listing); the scaled ones are nine more in a unit of
    their own, free of scratch and at most one wave per SIMD below their unscaled twin"""
    key = lambda k: re.search(r"ILi\dELi\dELi\dE", k).group(0)
    plain = {key(k): v for k, v in _resources("k_lpd").items() if "k_lpdI" in k}
    scaled = {key(k): v for k, v in _resources("k_lpd_scaled").items() if "k_lpd_scaledI" in k}
    assert len(plain) == 9 and sorted(scaled) == sorted(plain)
    for k, (vgprs, scratch, waves) in scaled.items():
        assert scratch == 0 and waves >= plain[k][2] - 1, (k, vgprs, scratch, waves)
