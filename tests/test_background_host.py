"""Background cells (setBackground) on the host (no GPU): the setter and what it guards, check_model's
second look, the values and weights the engine hands the row kernels, the two identities of tests/background_restatement.py against
the dense explicit sums, csrc/background.h compiled for the host, and the resource listing the build leaves for the new kernels."""
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import background_restatement as BR
from test_probit_host import _resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _relation(B, weights=False, alpha=2.0, names=("u", "v")):
    ids, y, w = BR.listing(weights=weights)
    rel = B.Relation({names[0]: ids[:, 0], names[1]: ids[:, 1], "y": y}, "plays", [B.Entity(nm) for nm in names], alpha=alpha, dims=[37, 29])
    if weights:
        B.setWeights(rel, w)
    return rel


# ---- the setter -----------------------------------------------------------------------------------------------------------------
def test_default_has_none(B):
    assert _relation(B).model.background is None and B.RelationModel().background is None


def test_setbackground_stores_weight_and_value_and_resets_the_device_state(B):
    rel = _relation(B)
    rel._dev = object()
    assert B.setBackground(rel, 0.25) is None
    assert rel.model.background == {"weight": 0.25, "value": 0.0} and rel._dev is None
    B.setBackground(rel, 1e-3, value=-1.5)
    assert rel.model.background == {"weight": 1e-3, "value": -1.5}
    assert rel.model.alpha == 2.0 and rel.model.alpha_sample is False


def test_noise_kind_does_not_change(B):
    from bdf_amd.relation_data import noise_kind
    rel, relw = _relation(B), _relation(B, weights=True)
    B.setBackground(rel, 0.3)
    B.setBackground(relw, 0.3 * relw.model.weights.min())
    assert noise_kind(rel) == "gauss" and noise_kind(relw) == "weights"
    assert "bg:0.3" in B.toStr(rel)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf"), "0.1", None, True])
def test_refuses_a_weight_that_is_not_finite(B, bad):
    rel = _relation(B)
    with pytest.raises(B.ArgumentError, match="weight"):
        B.setBackground(rel, bad)
    assert rel.model.background is None


@pytest.mark.parametrize("bad", [0.0, -0.1, 1.0, 1.5])
def test_refuses_a_weight_outside_zero_to_the_smallest_listed_weight(B, bad):
    rel = _relation(B)
    with pytest.raises(B.ArgumentError, match="strictly between 0 and the smallest weight"):
        B.setBackground(rel, bad)
    relw = _relation(B, weights=True)
    least = float(relw.model.weights.min())
    assert least < 1.0
    with pytest.raises(B.ArgumentError, match="strictly between 0 and the smallest weight"):
        B.setBackground(relw, least)                      # 0.9 of it is fine, the weight itself is not
    B.setBackground(relw, 0.9 * least)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), "0", None])
def test_refuses_a_value_that_is_not_finite(B, bad):
    rel = _relation(B)
    with pytest.raises(B.ArgumentError, match="value"):
        B.setBackground(rel, 0.1, bad)


def test_refuses_three_modes(B):
    rng = np.random.default_rng(0)
    t = {"a": rng.integers(1, 5, 20), "b": rng.integers(1, 6, 20), "c": rng.integers(1, 4, 20), "y": rng.standard_normal(20)}
    rel = B.Relation(t, "tensor", [B.Entity("a"), B.Entity("b"), B.Entity("c")], dims=[4, 5, 3])
    with pytest.raises(B.ArgumentError, match="has 3 modes"):
        B.setBackground(rel, 0.1)


def test_refuses_a_cell_listed_twice(B):
    rel = B.Relation({"u": [1, 2, 1], "v": [1, 3, 1], "y": [1.0, 1.0, 1.0]}, "plays", [B.Entity("u"), B.Entity("v")], dims=[3, 3])
    with pytest.raises(B.ArgumentError, match="more than once"):
        B.setBackground(rel, 0.1)


def test_refuses_relation_features(B):
    rel = _relation(B)
    rel.F = np.ones((rel.data.nnz(), 2))
    with pytest.raises(B.ArgumentError, match="has features"):
        B.setBackground(rel, 0.1)


def _other_models(B):
    return {
        "setProbit": lambda rel: B.setProbit(rel),
        "setCensored": lambda rel: B.setCensored(rel, np.zeros(rel.data.nnz(), dtype=np.int8)),
        "setInterval": lambda rel: B.setInterval(rel, rel.data.values - 1.0, rel.data.values + 1.0),
        "setBinned": lambda rel: B.setBinned(rel, [0.0, 1.0, 2.0]),
        "setOrdinal": lambda rel: B.setOrdinal(rel),
        "setRobust": lambda rel: B.setRobust(rel),
        "setLogit": lambda rel: B.setLogit(rel),
        "setCounts": lambda rel: B.setCounts(rel, 2),
        "setWaic": lambda rel: B.setWaic(rel),
    }


def _levels(B):
    """a relation whose values suit every noise model's setter: 0/1 for probit, logit and counts, 1 .. 4 for the ordinal model"""
    ids, _, _ = BR.listing()
    return lambda vals: B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": np.resize(np.asarray(vals, dtype=float), len(ids))}, "plays",
                                   [B.Entity("u"), B.Entity("v")], dims=[37, 29])


@pytest.mark.parametrize("name", ["setProbit", "setCensored", "setInterval", "setBinned", "setOrdinal", "setRobust", "setLogit", "setCounts", "setWaic"])
def test_refuses_every_other_noise_model_and_waic(B, name):
    vals = [1, 2, 3, 4] if name == "setOrdinal" else [0, 1]
    rel = _levels(B)(vals)
    _other_models(B)[name](rel)
    with pytest.raises(B.ArgumentError, match="setBackground"):
        B.setBackground(rel, 0.1)
    assert rel.model.background is None
    # ... and the other way round: the model set after the background is caught when a sampler is built
    from bdf_amd.relation_data import check_model
    rel = _levels(B)(vals)
    B.setBackground(rel, 0.1)
    _other_models(B)[name](rel)
    with pytest.raises(B.ArgumentError, match="setBackground"):
        check_model(rel)


def test_refuses_more_than_one_rank(B):
    from bdf_amd.relation_data import check_model
    rel = _relation(B)
    B.setBackground(rel, 0.1)
    check_model(rel, 1)
    with pytest.raises(B.ArgumentError, match="Relation plays has a background: one rank only"):
        check_model(rel, 2)


def test_check_model_catches_setweights_after_setbackground(B):
    from bdf_amd.relation_data import check_model
    rel = _relation(B)
    B.setBackground(rel, 0.5)
    check_model(rel)
    w = np.ones(rel.data.nnz())
    w[3] = 0.4                                            # a listed cell that would count for less than a background cell
    B.setWeights(rel, w)
    with pytest.raises(B.ArgumentError, match="strictly between 0 and the smallest weight"):
        check_model(rel)
    w[3] = 0.6
    B.setWeights(rel, w)
    check_model(rel)


def test_the_other_trainers_refuse_a_background(B):
    from bdf_amd._two_mode import relation_of
    rel = _relation(B)
    B.setBackground(rel, 0.1)
    with pytest.raises(B.ArgumentError, match="has a background"):
        relation_of(B.RelationData(rel), 8, "bpmf_vb")


# ---- what the engine hands the row kernels ---------------------------------------------------------------------------------------
def test_mean_is_over_all_cells_and_unit_values_keep_their_codes(B):
    from bdf_amd.relation_data import background_mean
    from bdf_amd.engine import _background_values
    rel = _relation(B)
    assert _background_values(rel) is None
    B.setBackground(rel, 0.3, value=0.5)
    ids, y, _ = BR.listing()
    mean = BR.all_cells_mean(37, 29, y, 0.5)
    assert background_mean(rel) == pytest.approx(mean, rel=1e-15)
    _, ya, _ = BR.dense_listing(37, 29, ids, y, np.ones(len(y)), 0.3, 0.5)
    assert background_mean(rel) == pytest.approx(ya.mean(), rel=1e-14)         # valueMean of the dense listing
    yp = _background_values(rel)
    assert np.allclose(yp, BR.unit_values(y, mean, 0.3, 0.5 - mean), rtol=1e-15, atol=0)
    assert len(np.unique(yp)) == len(np.unique(y))                            # a relation of ratings keeps its value codes
    # with setWeights the weighted kernel reads obs_precision and linear_values instead
    relw = _relation(B, weights=True)
    B.setBackground(relw, 0.1)
    assert _background_values(relw) is None


# ---- the two identities ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("rb_zero", [True, False])
def test_fold_row_systems_and_alpha_sum_equal_the_dense_explicit_sums(weights, rb_zero):
    """one background Gibbs iteration restated (the fold, the row systems, alpha's sum of squares) against the dense explicit sums at
    N = 37, M = 29, about 20 % listed, one row with no listed cell and one with every cell listed: to 1e-12 of the largest entry"""
    N, M, D, alpha = 37, 29, 6, 2.0
    ids, y, w = BR.listing(N, M, weights=weights)
    deg = np.bincount(ids[:, 0] - 1, minlength=N)
    assert deg[0] == 0 and deg[1] == M and 0.15 < len(ids) / (N * M) < 0.3
    c0 = 0.3 * w.min()
    value = float(np.mean(y)) if rb_zero else -0.5          # (the mean over all cells is the listed cells' mean iff the value is)
    mean = BR.all_cells_mean(N, M, y, value)
    assert (abs(value - mean) < 1e-14) == rb_zero
    rng = np.random.default_rng(1)
    U, V = rng.standard_normal((N, D)), rng.standard_normal((M, D))
    A = rng.standard_normal((D, D))
    Lam = A @ A.T + D * np.eye(D)
    for mu in (rng.standard_normal(D), rng.standard_normal((N, D))):
        Pf, bf = BR.systems_folded(N, ids, y, w, mean, c0, value, V, alpha, Lam, mu)
        Pd, bd = BR.systems_dense(N, M, ids, y, w, mean, c0, value, V, alpha, Lam, mu)
        scale = np.abs(Pd).max()
        assert np.abs(Pf - Pd).max() <= 1e-12 * scale and np.abs(bf - bd).max() <= 1e-12 * scale
    sf, sd = BR.sse_folded(ids, y, w, mean, c0, value, U, V), BR.sse_dense(ids, y, w, mean, c0, value, U, V)
    assert abs(sf - sd) <= 1e-12 * sd
    # what the engine hands the kernels is the same fold: unit weights through the values and alpha (1 - c0), weights through
    # obs_precision and linear_values
    rb = value - mean
    if not weights:
        assert np.allclose((BR.unit_values(y, mean, c0, rb) - mean) * (1.0 - c0), (y - mean) - c0 * rb, rtol=1e-13, atol=1e-15)
    prec, lin = BR.weighted_terms(y, w, mean, c0, rb)
    assert np.all(prec > 0) and np.allclose(prec * (y - lin), w * (y - mean) - c0 * rb, rtol=1e-13, atol=1e-15)


def test_a_relation_that_lists_every_cell_has_no_background_term():
    """no cell is unlisted: the Gram term and the listed cells' correction cancel, whatever c0"""
    N, M, D = 5, 4, 3
    rng = np.random.default_rng(2)
    ii, jj = np.meshgrid(np.arange(1, N + 1), np.arange(1, M + 1), indexing="ij")
    ids, y, w = np.stack([ii.ravel(), jj.ravel()], axis=1), rng.standard_normal(N * M), np.ones(N * M)
    V, Lam, mu = rng.standard_normal((M, D)), 3.0 * np.eye(D), rng.standard_normal(D)
    mean = float(np.mean(y))
    Pf, bf = BR.systems_folded(N, ids, y, w, mean, 0.3, 0.7, V, 2.0, Lam, mu)
    P0, b0 = BR.row_systems(N, ids, y - mean, w, V, 2.0, Lam, mu)
    assert np.allclose(Pf, P0, rtol=1e-13, atol=1e-13) and np.allclose(bf, b0, rtol=1e-13, atol=1e-13)


# ---- csrc/background.h on the host -------------------------------------------------------------------------------------------------
_HOST_SRC = r"""
#include <cstdio>
#include "background.h"
int main() {
    double w, e, c0, rb, psi, cells, ds, dg, alpha;
    while (scanf("%lf %lf %lf %lf %lf %lf %lf %lf %lf", &w, &e, &c0, &rb, &psi, &cells, &ds, &dg, &alpha) == 9)
        printf("%.17g %.17g %.17g\n", bdf_bg_term(w, e, c0, rb, psi), bdf_bg_all_cells(c0, cells, rb, ds, dg), bdf_bg_alpha_rows(alpha, c0));
    return 0;
}
"""


def test_background_header_on_the_host():
    cxx = [shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")]
    if cxx[0] is None:
        cxx = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "c++"]
    td = tempfile.mkdtemp()
    try:
        open(os.path.join(td, "t.cpp"), "w").write(_HOST_SRC)
        subprocess.run(cxx + ["-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "bayesiandatafusion.jl_amd", "csrc"), os.path.join(td, "t.cpp"),
                              "-o", os.path.join(td, "t")], check=True)
        rng = np.random.default_rng(5)
        rows = rng.standard_normal((50, 9))
        rows[:, 2] = rng.uniform(0.01, 0.9, 50)
        rows[:, 5] = rng.integers(1, 10_000, 50)
        text = "".join(" ".join("%.17g" % x for x in r) + "\n" for r in rows)
        out = subprocess.run([os.path.join(td, "t")], input=text, capture_output=True, text=True, check=True).stdout
        got = np.array([float(t) for t in out.split()]).reshape(50, 3)
    finally:
        shutil.rmtree(td, ignore_errors=True)
    w, e, c0, rb, psi, cells, ds, dg, alpha = rows.T
    assert np.array_equal(got[:, 0], w * (e * e) - c0 * ((rb - psi) * (rb - psi)))
    assert np.array_equal(got[:, 1], c0 * ((cells * (rb * rb) - 2.0 * rb * ds) + dg))
    assert np.array_equal(got[:, 2], alpha * (1.0 - c0))


# ---- the C ABI and the build's listing --------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_documented(B):
    h = open(os.path.join(ROOT, "include", "bdf.h")).read()
    jl = open(os.path.join(ROOT, "julia", "BDFHip.jl")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("bdf_background_prior", "bdf_background_sse"):
        assert name + "(" in h and name in B.declared_symbols() and (":" + name) in jl and name in doc
    assert "bg_weight, bg_value" in h and "bg_weight::Float64" in jl


def test_new_kernels_keep_their_registers():
    """the build's resource listing (csrc/k_background.o.res): the gather and the row product keep no registers in scratch memory; of
    the one-wave fold only the D = 64 variant has the 528 bytes per lane that wl_factor<64> brings to every kernel that takes it"""
    res = _resources("k_background")
    assert len(res) == 10, sorted(res)
    for k, (vgprs, scratch, occ) in res.items():
        if "k_bg_foldILi64" in k:
            assert scratch == _resources("k_feat_beta")["13k_solve_smallILi64EEEviiPKdS2_S2_PdPi"][1], (k, scratch)
        else:
            assert scratch == 0, (k, scratch)
        assert vgprs <= 256 and occ >= 1
        if "k_bg_sse" in k or "k_bg_mu_rows" in k:
            assert occ >= 3, (k, occ)
