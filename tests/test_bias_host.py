"""Row and column biases on the host (no GPU): setBias, how it resolves its entity and what it guards in both
orders, the re-checks when a sampler is built, the restated step of tests/bias_restatement.py against the conditional read off the
joint Gaussian of all biases and against the oracle's Philox, csrc/bias.h compiled for the host against the restatement, the entry
points in the header, the binding, the Julia file and INTEGRATION.md, the stream purposes, and the resource listings the build
leaves for the new kernels."""
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import bias_restatement as BR
from test_newrows_host import _resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bayesiandatafusion.jl_amd", "csrc")


def _relation(B, n=40, test=None, alpha=2.0, names=("u", "v"), dims=(8, 6), values=None, ents=None):
    rng = np.random.default_rng(3)
    table = {nm: rng.integers(1, d + 1, n) for nm, d in zip(names, dims)}
    if len(dims) == 2:                                   # distinct cells (setBackground refuses a cell listed twice)
        cells = rng.choice(dims[0] * dims[1], size=n, replace=False)
        table = {names[0]: cells // dims[1] + 1, names[1]: cells % dims[1] + 1}
    table["y"] = rng.standard_normal(n) if values is None else values
    rel = B.Relation(table, "ratings", ents or [B.Entity(nm) for nm in names], alpha=alpha, dims=list(dims))
    if test is not None:
        B.assignToTest(rel, test)
    return rel


# ---- the setter ---------------------------------------------------------------------------------------------------------------
def test_setter_is_exported_and_in_the_readme(B):
    assert callable(B.setBias) and "setBias" in open(os.path.join(ROOT, "README.md")).read()


def test_default_has_none_and_the_setter_stores_its_spec(B):
    rel = _relation(B)
    assert rel.model.bias == {}
    rel._dev = object()
    assert B.setBias(rel, rel.entities[1]) is None
    assert rel.model.bias == {2: {"shape": 1.0, "rate": 1.0}} and rel._dev is None
    B.setBias(rel, "u", shape=0.5, rate=3)
    assert rel.model.bias == {2: {"shape": 1.0, "rate": 1.0}, 1: {"shape": 0.5, "rate": 3.0}}
    with pytest.raises(B.ArgumentError, match="once per entity"):
        B.setBias(rel, 1)
    with pytest.raises(B.ArgumentError, match="once per entity"):
        B.setBias(rel, "v")
    rel3 = _relation(B, names=("a", "b", "c"), dims=(8, 6, 4))
    B.setBias(rel3, np.int64(3), 1.5, 0.25)
    B.setBias(rel3, 1)
    assert rel3.model.bias == {3: {"shape": 1.5, "rate": 0.25}, 1: {"shape": 1.0, "rate": 1.0}}
    assert B.toStr(rel3) == "rati[α=2.0 b:a,c]" and B.toStr(rel) == "rati[α=2.0 b:u,v]"
    # a second relation keeps its own: the default is not shared
    assert _relation(B).model.bias == {}


@pytest.mark.parametrize("bad", [0, 3, -1, "w", None, 1.0, True, "", ["u"]])
def test_the_setter_refuses_what_is_no_entity_of_the_relation(B, bad):
    rel = _relation(B)
    with pytest.raises(B.ArgumentError, match="entity"):
        B.setBias(rel, bad)
    with pytest.raises(B.ArgumentError, match="entity"):
        B.setBias(rel, B.Entity("u"))                               # an entity of that name, but not the relation's
    assert rel.model.bias == {}


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), float("inf"), "2", None, True])
def test_the_setter_refuses_a_shape_or_rate_that_is_not_positive_and_finite(B, bad):
    rel = _relation(B)
    with pytest.raises(B.ArgumentError, match="shape"):
        B.setBias(rel, "u", shape=bad)
    with pytest.raises(B.ArgumentError, match="rate"):
        B.setBias(rel, "u", rate=bad)
    assert rel.model.bias == {}


def test_it_works_before_and_after_the_test_split_and_with_waic(B):
    rel = _relation(B)
    B.setBias(rel, "u")
    B.assignToTest(rel, np.arange(1, 6))
    B.setBias(rel, "v")
    B.setWaic(rel)
    assert sorted(rel.model.bias) == [1, 2] and rel.model.waic is not None
    rel = _relation(B)
    B.setWaic(rel)
    B.setBias(rel, "v")
    rel.model.alpha_sample = True
    from bdf_amd.relation_data import check_model
    check_model(rel)


# ---- what it excludes, in both orders -------------------------------------------------------------------------------------------
def _fresh(B, kind):
    if kind in ("probit", "logit"):
        return _relation(B, values=(np.arange(40) % 2).astype(np.float64))
    if kind == "counts":
        return _relation(B, values=(np.arange(40) % 7).astype(np.float64))
    if kind == "ordinal":
        return _relation(B, values=(np.arange(40) % 5 + 1).astype(np.float64))
    if kind == "dense":
        return _relation(B, n=40, dims=(8, 6))               # 40 of 48 cells listed
    if kind == "newtest":
        ents = [B.Entity("u", F=np.eye(8)), B.Entity("v")]
        B.setNewRows(ents[0], np.ones((2, 8)))
        return _relation(B, ents=ents)
    if kind in ("spike", "nonneg"):
        r = _relation(B)
        r._keep = B.RelationData(r)                          # (an entity learns of its relations there: before, only the sampler's check can see both)
        return r
    return _relation(B)


def _set_new_test(B, r):
    B.setNewTest(r, r.entities[0], (np.array([[1, 1], [2, 3]]), np.array([0.5, np.nan])))


THEIRS = {
    "robust": (lambda B, r: B.setRobust(r, 4.0), lambda r: r.model.robust is None),
    "weights": (lambda B, r: B.setWeights(r, np.full(40, 2.0)), lambda r: r.model.weights is None),
    "probit": (lambda B, r: B.setProbit(r), lambda r: not r.model.probit),
    "censored": (lambda B, r: B.setCensored(r, np.zeros(40, dtype=int)), lambda r: r.model.censor is None),
    "interval": (lambda B, r: B.setInterval(r, r.data.values - 1.0, r.data.values + 1.0), lambda r: r.model.interval is None),
    "binned": (lambda B, r: B.setBinned(r, [-1.0, 0.0, 1.0]), lambda r: r.model.interval is None),
    "ordinal": (lambda B, r: B.setOrdinal(r), lambda r: r.model.ordinal is None),
    "logit": (lambda B, r: B.setLogit(r), lambda r: r.model.pg is None),
    "counts": (lambda B, r: B.setCounts(r, 3), lambda r: r.model.pg is None),
    "entity_noise": (lambda B, r: B.setEntityNoise(r, "v"), lambda r: r.model.entity_noise is None),
    "background": (lambda B, r: B.setBackground(r, 0.1), lambda r: r.model.background is None),
    "dense": (lambda B, r: B.setDense(r), lambda r: not r.model.dense),
    "recommend": (lambda B, r: B.setRecommend(r, 3), lambda r: r.model.recommend is None),
    "newtest": (_set_new_test, lambda r: r.model.new_test is None),
    "spike": (lambda B, r: B.setSpikeAndSlab(r.entities[1]), lambda r: r.entities[1].spike is None),
    "nonneg": (lambda B, r: B.setNonNegative(r.entities[0]), lambda r: r.entities[0].nonneg is None),
}


@pytest.mark.parametrize("kind", list(THEIRS))
def test_exclusions_in_both_orders(B, kind):
    setter, empty = THEIRS[kind]
    # theirs first: setBias is refused and leaves nothing
    r = _fresh(B, kind)
    setter(B, r)
    with pytest.raises(B.ArgumentError, match="setBias"):
        B.setBias(r, "u")
    assert r.model.bias == {} and not empty(r)
    # setBias first: theirs is refused, names it and leaves nothing
    r = _fresh(B, kind)
    B.setBias(r, "u")
    with pytest.raises(B.ArgumentError, match="setBias"):
        setter(B, r)
    assert empty(r) and r.model.bias == {1: {"shape": 1.0, "rate": 1.0}}


def test_relation_features_in_both_orders(B):
    from bdf_amd.relation_data import check_bias, check_model
    r = _relation(B)
    r.F = np.ones((40, 2))
    with pytest.raises(B.ArgumentError, match="features"):
        B.setBias(r, "u")
    r = _relation(B)
    B.setBias(r, "u")
    r.F = np.ones((40, 2))                                          # (features are a field, not a setter: the sampler's check finds them)
    with pytest.raises(B.ArgumentError, match="features"):
        check_bias(r)
    with pytest.raises(B.ArgumentError, match="features"):
        check_model(r)


def test_rechecks_when_a_sampler_is_built_and_the_one_rank_refusal(B):
    from bdf_amd.relation_data import check_bias, check_model, noise_kind
    rel = _relation(B)
    B.setBias(rel, "v")
    assert noise_kind(rel) == "gauss"
    assert check_model(rel) is None and check_model(rel, world=1) is None
    with pytest.raises(B.ArgumentError) as e:
        check_model(rel, world=2)
    assert str(e.value) == "Relation ratings has biases (setBias): one rank only"
    with pytest.raises(B.ArgumentError, match="one rank"):
        B.GibbsEngine(B.RelationData(rel), 4, shard=(0, 2))
    # changed behind the setter's back: the check looks again, and raises what check_model raises
    for spoil in ({3: {"shape": 1.0, "rate": 1.0}}, {1: {"shape": 0.0, "rate": 1.0}}, {1: {"shape": 1.0, "rate": float("nan")}}, {1: {}}, {"w": {"shape": 1.0, "rate": 1.0}}):
        rel.model.bias = spoil
        with pytest.raises(B.ArgumentError) as e1:
            check_bias(rel)
        with pytest.raises(B.ArgumentError) as e2:
            check_model(rel)
        assert str(e1.value) == str(e2.value)
    rel.model.bias = {np.int64(2): {"shape": 3, "rate": 1}, "u": {"shape": 2.0, "rate": 0.5}}
    check_model(rel)
    assert rel.model.bias == {2: {"shape": 3.0, "rate": 1.0}, 1: {"shape": 2.0, "rate": 0.5}}
    for field, value, name in (("robust", {"nu": 4.0}, "setRobust"), ("background", {"weight": 0.1, "value": 0.0}, "setBackground"),
                               ("recommend", {"k": 3, "rows": None, "exclude_listed": True, "batch": 8}, "setRecommend")):
        setattr(rel.model, field, value)
        with pytest.raises(B.ArgumentError, match=name):
            check_model(rel)
        setattr(rel.model, field, None)
    rel.entities[0].spike = {"incl_a": 1.0, "incl_b": 1.0, "shape": 1.0, "rate": 1.0}
    with pytest.raises(B.ArgumentError, match="setSpikeAndSlab"):
        check_model(rel)


def test_the_two_mode_trainers_refuse_it(B):
    rel = _relation(B, test=np.arange(1, 6))
    B.setBias(rel, "v")
    rd = B.RelationData(rel)
    with pytest.raises(B.ArgumentError, match="setBias"):
        B.bpmf_vb(rd, num_latent=4, verbose=False, niter=1)
    with pytest.raises(B.ArgumentError, match="setBias"):
        B.macau_hmc(rd, num_latent=4, verbose=False, burnin=1, psamples=1)


# ---- the streams and the entry points --------------------------------------------------------------------------------------------
def test_stream_purposes_are_defined_and_unused_by_others():
    h = open(os.path.join(ROOT, "include", "bdf.h")).read()
    purposes = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (BDF_P_[A-Z0-9_]+)\s+(\d+)", h)}
    assert (purposes["BDF_P_BIAS"], purposes["BDF_P_BIAS_N"], purposes["BDF_P_BIAS_U"]) == (28, 29, 30)
    assert len(set(purposes.values())) == len(purposes)           # no two purposes share a number
    from bdf_amd import _lib
    assert (_lib.P_BIAS, _lib.P_BIAS_N, _lib.P_BIAS_U) == (BR.P_BIAS, BR.P_BIAS_N, BR.P_BIAS_U) == (28, 29, 30)


def test_entry_points_are_declared_bound_and_documented():
    import ctypes as C
    from bdf_amd import _lib
    h = open(os.path.join(ROOT, "include", "bdf.h")).read()
    jl = open(os.path.join(ROOT, "julia", "BDFHip.jl")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("bdf_bias_draw", "bdf_bias_baseline"):
        assert re.search(r"\bint %s\(" % name, h) and name in _lib.declared_symbols() and ":" + name in jl and name in doc
    assert len(_lib._SIGS["bdf_bias_draw"][1]) == 13 and len(_lib._SIGS["bdf_bias_baseline"][1]) == 6
    # the term and the relation's tail, field for field
    assert [f[0] for f in _lib.BiasTerm._fields_] == ["mode", "_pad", "shape", "rate", "bias", "lambda_"] and C.sizeof(_lib.BiasTerm) == 40
    m = re.search(r"typedef struct \{([^}]*)\} bdf_bias_term;", h)
    assert m and re.findall(r"(\w+)[;,]", m.group(1)) == ["mode", "_pad", "shape", "rate", "bias", "lambda"]
    tail = [f[0] for f in _lib.GibbsRelation._fields_][-5:]
    assert tail == ["n_bias", "_pad_bias", "bias", "bias_resid", "bias_test"]
    body = re.search(r"typedef struct \{((?:(?!typedef struct)[\s\S])*?)\} bdf_gibbs_relation;", h).group(1)
    body = re.sub(r"/\*[\s\S]*?\*/", "", body)
    assert re.findall(r"(\w+)(?:\[\w+\])?;", body)[-5:] == tail
    for field in tail:
        assert re.search(r"\b%s::" % field, jl), field
    assert "struct BiasTerm" in jl and "bias_draw!" in jl and "bias_baseline!" in jl


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def test_vectorised_draws_are_the_oracles_streams(O):
    """normal_one and gamma_mt draw one number at a time from oracle.normals and oracle.draw; normals and gamma_variates must be the
    same numbers, for every mode (either element of the pair) and on either side of shape 1"""
    rows = np.array([0, 1, 2, 5, 17, 1002, 2 ** 33 + 5])
    for seed, sweep, tag in ((1234, 3, 1), (2 ** 40 + 7, 77, 3)):
        for mode in range(4):
            got = BR.normals(seed, sweep, tag, rows, mode)
            want = np.array([BR.normal_one(seed, sweep, tag, int(r), mode) for r in rows])
            np.testing.assert_allclose(got, want, rtol=1e-13, atol=1e-15)
        assert abs(BR.normal_one(seed, sweep, tag, 5, 0) - BR.normal_one(seed, sweep, tag, 5, 1)) > 1e-9
    for seed, sweep, tag, a in ((1234, 3, 1, 1.0), (91, 1, 2, 2.5), (2 ** 40 + 7, 77, 3, 152.0), (5, 9, 1, 0.5), (5, 9, 2, 0.01)):
        got = BR.gamma_variates(seed, sweep, tag, [0, 1, 2, 3], a)
        want = np.array([BR.gamma_mt(seed, sweep, tag, m, a) for m in range(4)])
        np.testing.assert_allclose(got, want, rtol=1e-13)
        assert np.all(got > 0) and np.all(np.isfinite(got))
    # and neither sample_alpha's stream nor the per-row noise model's
    import entity_noise_restatement as ER
    assert abs(O.gamma(1234, 3, 0x800000 | 1, 0, 2.5) - BR.gamma_mt(1234, 3, 1, 0, 2.5)) > 1e-6
    assert abs(ER.gamma_mt(1234, 3, 1, 0, 2.5) - BR.gamma_mt(1234, 3, 1, 0, 2.5)) > 1e-6


def test_row_conditional_is_the_joint_gaussians():
    """3 x 2 cells, both modes biased, fixed U, V, alpha and lambda.  Given the factors the five biases are jointly Gaussian: precision
    Q = diag(lambda) + alpha A'A and linear term h = alpha A'e, A the (cells x biases) incidence matrix.  The conditional of bias t
    given the others has precision Q_tt and mean (h_t - sum_{s != t} Q_ts b_s) / Q_tt; the restatement's (mean_j, prec_j) must be
    that, to 1e-12, for every row of both modes and arbitrary values of the other biases."""
    rng = np.random.default_rng(8)
    dims, D, alpha, lam = [3, 2], 2, 1.7, {0: 0.6, 1: 2.3}
    ids = np.array([[i + 1, j + 1] for i in range(3) for j in range(2)], dtype=np.int64)
    U, V = rng.standard_normal((3, D)), rng.standard_normal((2, D))
    y, mean = rng.standard_normal(6), 0.2
    e = y - ((U[ids[:, 0] - 1] * V[ids[:, 1] - 1]).sum(axis=1) + mean)
    A = np.zeros((6, 5))
    A[np.arange(6), ids[:, 0] - 1] = 1.0
    A[np.arange(6), 3 + ids[:, 1] - 1] = 1.0
    Q = np.diag([lam[0]] * 3 + [lam[1]] * 2) + alpha * A.T @ A
    h = alpha * A.T @ e
    b = {0: rng.standard_normal(3), 1: rng.standard_normal(2)}
    ball = np.concatenate([b[0], b[1]])
    for mode, off in ((0, 0), (1, 3)):
        n, S = BR.row_sums(ids[:, mode] - 1, dims[mode], BR.others_off(e, ids, b, mode))
        m_ref, p_ref = BR.row_conditional(S, n, alpha, lam[mode])
        for j in range(dims[mode]):
            t = off + j
            prec = Q[t, t]
            cond = (h[t] - (Q[t] @ ball - Q[t, t] * ball[t])) / prec
            assert abs(p_ref[j] - prec) <= 1e-12 and abs(m_ref[j] - cond) <= 1e-12, (mode, j)
    # and the draw is mean + z / sqrt(prec); the precision's is G / (rate + sum b^2 / 2)
    z = rng.standard_normal(3)
    n, S = BR.row_sums(ids[:, 0] - 1, 3, BR.others_off(e, ids, b, 0))
    m_ref, p_ref = BR.row_conditional(S, n, alpha, lam[0])
    assert np.allclose(BR.draw_rows(S, n, alpha, lam[0], z), m_ref + z / np.sqrt(p_ref), rtol=0, atol=1e-15)
    assert BR.draw_lambda(3.0, 2.0, 4.0) == 0.75


def test_step_is_the_draw_mode_by_mode():
    """step (what run_chain and the GPU tests call) against the definition written out: rising mode order, a mode drawn earlier
    contributes its new value, every mode's rows read the lambda the step found, a row without cells draws from its prior, and the
    base adds the biases in rising mode order"""
    rng = np.random.default_rng(12)
    dims, n = [9, 5, 4], 60
    ids = np.stack([rng.integers(1, d + 1, n) for d in dims], axis=1)
    ids[ids[:, 0] == 5, 0] = 6                              # row 4 of mode 0 has no cell
    e = rng.standard_normal(n)
    spec = {2: (0.5, 2.0), 0: (1.5, 0.7)}
    b0 = {0: rng.standard_normal(9), 2: rng.standard_normal(4)}
    lam0 = {0: 0.8, 2: 3.0}
    b, lam = BR.step(31, 7, 3, ids, dims, e, 1.3, spec, b0, lam0)
    # mode 0 first, against mode 2's OLD biases
    for j in range(9):
        sel = ids[:, 0] == j + 1
        S = float(np.sum(e[sel] - b0[2][ids[sel, 2] - 1]))
        prec = 0.8 + 1.3 * sel.sum()
        want = 1.3 * S / prec + BR.normal_one(31, 7, 3, j, 0) / np.sqrt(prec)
        assert abs(b[0][j] - want) <= 1e-13 * max(1.0, abs(want)), j
    assert abs(b[0][4] - BR.normal_one(31, 7, 3, 4, 0) / np.sqrt(0.8)) <= 1e-14
    # mode 2 second, against mode 0's NEW biases
    for j in range(4):
        sel = ids[:, 2] == j + 1
        S = float(np.sum(e[sel] - b[0][ids[sel, 0] - 1]))
        prec = 3.0 + 1.3 * sel.sum()
        want = 1.3 * S / prec + BR.normal_one(31, 7, 3, j, 2) / np.sqrt(prec)
        assert abs(b[2][j] - want) <= 1e-13 * max(1.0, abs(want)), j
    assert abs(lam[0] - BR.gamma_mt(31, 7, 3, 0, 1.5 + 4.5) / (0.7 + 0.5 * np.sum(b[0] ** 2))) <= 1e-13 * lam[0]
    assert abs(lam[2] - BR.gamma_mt(31, 7, 3, 2, 0.5 + 2.0) / (2.0 + 0.5 * np.sum(b[2] ** 2))) <= 1e-13 * lam[2]
    assert np.array_equal(BR.base(ids, b, 0.25), (0.25 + b[0][ids[:, 0] - 1]) + b[2][ids[:, 2] - 1])


def test_run_chain_without_biases_is_the_gaussian_chain():
    """spec = None: the same numbers as entity_noise_restatement's Gaussian chain (mode = None) on the same data"""
    import entity_noise_restatement as ER
    ids, y, dims, feats, n_test, alpha, _ = BR.iteration_case(2, 0, 1)
    a = BR.run_chain(ids[n_test:], y[n_test:], dims, 4, 91, 2, alpha=alpha, alpha_sample=True, test_ids=ids[:n_test], test_values=y[:n_test], burnin=1)
    b = ER.run_chain(ids[n_test:], y[n_test:], dims, 4, 91, 2, alpha=alpha, alpha_sample=True, test_ids=ids[:n_test], test_values=y[:n_test], burnin=1)
    for k in range(2):
        np.testing.assert_allclose(a["S"][k], b["S"][k], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(a["pred"], b["pred"], rtol=1e-12, atol=1e-12)
    assert abs(a["alpha"] - b["alpha"]) <= 1e-12 * b["alpha"] and abs(a["LPD"] - b["LPD"]) <= 1e-12
    c = BR.run_chain(ids[n_test:], y[n_test:], dims, 4, 91, 2, spec={0: (1.0, 1.0)}, alpha=alpha, alpha_sample=True, test_ids=ids[:n_test], burnin=1)
    assert np.abs(c["S"][0] - a["S"][0]).max() > 1e-3 and np.abs(c["bias"][0]).max() > 0.1


# ---- the header -----------------------------------------------------------------------------------------------------------------
def test_header_and_restatement_state_the_same_map():
    """csrc/bias.h, the text the kernels form b and lambda with, compiled for the host (as test_entity_noise_host.py compiles
    entity_noise.h) against draw_rows, draw_lambda and others_off: the same operations in the same order, so the same bits; every
    fifth row has no cells"""
    cxx = [shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")]
    if cxx[0] is None:
        cxx = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "c++"]
    src = r'''
        #include <cstdio>
        #include "bias.h"
        int main() { int n; if (scanf("%d", &n) != 1) return 1;
                     for (int i = 0; i < n; i++) { double S, alpha, lambda, z, G, rate, sb2, shape, e, o1, o2; long long nj;
                         if (scanf("%lf %lld %lf %lf %lf %lf %lf %lf %lf %lf %lf %lf", &S, &nj, &alpha, &lambda, &z, &G, &rate, &sb2, &shape, &e, &o1, &o2) != 12) return 1;
                         printf("%.17g %.17g %.17g %.17g %.17g\n", bdf_bias_row(S, nj, alpha, lambda, z), bdf_bias_prec(lambda, alpha, nj),
                                bdf_bias_lambda(G, rate, sb2), bdf_bias_lambda_shape(shape, nj), bdf_bias_resid(bdf_bias_resid(e, o1), o2)); }
                     return 0; }
    '''
    rng = np.random.default_rng(21)
    n = 400
    nj = rng.integers(1, 20000, n)
    nj[::5] = 0
    S = np.where(nj == 0, 0.0, rng.standard_normal(n) * np.sqrt(np.maximum(nj, 1)))
    alpha, lam, z = np.exp(rng.uniform(-4, 7, n)), np.exp(rng.uniform(-3, 3, n)), rng.standard_normal(n)
    G, rate, sb2, shape = rng.gamma(3.0, size=n), np.exp(rng.uniform(-3, 3, n)), np.exp(rng.uniform(-6, 6, n)), np.exp(rng.uniform(-2, 2, n))
    e, o1, o2 = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "t.cpp"), "w").write(src)
        subprocess.run(cxx + ["-O1", "-ffp-contract=off", "-I", CSRC, os.path.join(td, "t.cpp"), "-o", os.path.join(td, "t")], check=True)
        text = "%d\n" % n + "".join("%.17g %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n" % t
                                    for t in zip(S, nj, alpha, lam, z, G, rate, sb2, shape, e, o1, o2))
        out = subprocess.run([os.path.join(td, "t")], input=text, capture_output=True, text=True, check=True).stdout
    got = np.array([float(t) for t in out.split()]).reshape(n, 5)
    assert np.array_equal(got[:, 0], BR.draw_rows(S, nj, alpha, lam, z))
    assert np.array_equal(got[:, 1], BR.row_conditional(S, nj, alpha, lam)[1])
    assert np.array_equal(got[::5, 0], z[::5] / np.sqrt(lam[::5]))            # no cells: the prior's draw
    assert np.array_equal(got[:, 2], BR.draw_lambda(G, rate, sb2)) and np.array_equal(got[:, 3], shape + 0.5 * nj)
    assert np.array_equal(got[:, 4], (e - o1) - o2)


def test_header_writes_down_the_summation_order_of_both_widths():
    text = open(os.path.join(CSRC, "bias.h")).read()
    assert "W = 8" in text and "W = 64" in text and "((p0 + p4) + (p2 + p6)) + ((p1 + p5) + (p3 + p7))" in text
    assert "(w0 + w1) + (w2 + w3)" in text and "rising mode order" in text


# ---- the build's listings -------------------------------------------------------------------------------------------------------
def test_bias_kernels_use_no_scratch_and_fit_their_launch_bounds():
    """the build's resource listing of k_bias: nine residual kernels (2-4 modes x <vector width, row pieces> = <1, 1>, <4, 1>, <4, 2>),
    the row kernel at both widths, the lambda and the base kernel; none keeps registers in scratch memory; each reaches the waves
    per SIMD its launch bounds declare -- k_bias_resid 3, or 2 where NM x NC >= 8 with 16-byte loads (k_noise_resid's bounds), the
    others 1 -- and LDS holds the four wave sums of a reduction and nothing else"""
    res = _resources("k_bias")
    resid = {k: v for k, v in res.items() if "k_bias_residI" in k}
    rows = {k: v for k, v in res.items() if "k_bias_rowsI" in k}
    assert len(resid) == 9 and len(rows) == 2 and any("ILi8E" in k for k in rows) and any("ILi64E" in k for k in rows)
    assert sum("k_bias_lambda" in k for k in res) == 1 and sum("k_bias_base" in k for k in res) == 1 and len(res) == 13
    for k, v in res.items():
        assert v["ScratchSize"] == 0, (k, v)
        want = 1
        if "k_bias_residI" in k:
            nm, vec, nc = (int(x) for x in re.search(r"ILi(\d)ELi(\d)ELi(\d)E", k).groups())
            want = 2 if (vec == 4 and nm * nc >= 8) else 3
        assert v["Occupancy"] >= want, (k, v, want)
        assert v["LDS"] == (32 if ("k_bias_rows" in k or "k_bias_lambda" in k) else 0), (k, v)
