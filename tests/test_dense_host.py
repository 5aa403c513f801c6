"""Dense relations (setDense) on the host (no GPU): the setter, denseRelation and what they guard in either
order of the calls, check_model's second look, the identities of tests/dense_restatement.py against the explicit listing,
csrc/dense.h compiled for the host, the C ABI's declarations and the resource listing the build leaves for the new kernels."""
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import background_restatement as BR
import dense_restatement as DR
from test_probit_host import _resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _relation(B, Y=None, alpha=2.0, names=("u", "v")):
    Y = DR.table() if Y is None else Y
    ids, y = DR.listing(Y)
    return B.Relation({names[0]: ids[:, 0], names[1]: ids[:, 1], "y": y}, "panel", [B.Entity(nm) for nm in names], alpha=alpha, dims=list(Y.shape))


# ---- the setter -----------------------------------------------------------------------------------------------------------------
def test_default_is_not_dense(B):
    assert _relation(B).model.dense is False and B.RelationModel().dense is False


def test_setdense_sets_the_flag_resets_the_device_state_and_can_be_taken_back(B):
    from bdf_amd.relation_data import noise_kind
    rel = _relation(B)
    before = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in vars(rel.model).items()}
    text = B.toStr(rel)
    rel._dev = object()
    assert B.setDense(rel) is None
    assert rel.model.dense is True and rel._dev is None and noise_kind(rel) == "gauss"
    assert rel.model.alpha == 2.0 and rel.model.alpha_sample is False and "dense" in B.toStr(rel)
    rel._dev = object()
    assert B.setDense(rel, False) is None and rel._dev is None
    after = vars(rel.model)
    assert set(after) == set(before)
    for k, v in before.items():
        assert np.array_equal(after[k], v) if isinstance(v, np.ndarray) else after[k] == v, k
    assert B.toStr(rel) == text


def test_denserelation_and_setdense_agree(B):
    Y = DR.table()
    a, b = B.denseRelation(Y, "panel", [B.Entity("u"), B.Entity("v")], class_cut=0.5, alpha=2.0), _relation(B, Y)
    B.setDense(b)
    assert a.model.dense and b.model.dense and a.class_cut == 0.5 and a.model.alpha == b.model.alpha == 2.0
    assert np.array_equal(a.data.ids, b.data.ids) and np.array_equal(a.data.values, b.data.values) and list(a.data.dims) == list(b.data.dims) == [37, 29]
    assert [e.count for e in a.entities] == [37, 29]
    # NaN marks a hole: it is not listed
    Y2 = Y.copy()
    Y2[3, 4] = Y2[36, 28] = np.nan
    c = B.denseRelation(Y2, "panel", [B.Entity("u"), B.Entity("v")])
    assert c.data.nnz() == 37 * 29 - 2 and list(c.data.dims) == [37, 29]
    from bdf_amd.relation_data import dense_matrix
    Yc, holes = dense_matrix(c)
    assert np.array_equal(np.isnan(Yc), np.isnan(Y2)) and np.array_equal(Yc[~np.isnan(Y2)], Y2[~np.isnan(Y2)])
    assert holes.tolist() == [[3, 4], [36, 28]]
    with pytest.raises(B.ArgumentError, match="2-D array"):
        B.denseRelation(np.zeros(5), "panel", [B.Entity("u"), B.Entity("v")])
    with pytest.raises(B.ArgumentError, match="number of entities has to be 2"):
        B.denseRelation(Y, "panel", [B.Entity("u")])


def test_a_table_given_to_relation_is_still_a_table(B):
    """Relation reads what it is handed as ids and values, a 2-D array included: only denseRelation reads a matrix of values"""
    rel = B.Relation((np.array([[1, 2], [2, 1]]), np.array([0.5, 1.5])), "r", [B.Entity("u"), B.Entity("v")])
    assert rel.data.nnz() == 2 and rel.model.dense is False and list(rel.data.dims) == [2, 2]


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refuses_three_modes(B):
    rng = np.random.default_rng(0)
    t = {"a": rng.integers(1, 5, 20), "b": rng.integers(1, 6, 20), "c": rng.integers(1, 4, 20), "y": rng.standard_normal(20)}
    rel = B.Relation(t, "tensor", [B.Entity("a"), B.Entity("b"), B.Entity("c")], dims=[4, 5, 3])
    with pytest.raises(B.ArgumentError, match="has 3 modes"):
        B.setDense(rel)
    assert rel.model.dense is False


def test_refuses_a_cell_listed_twice(B):
    rel = B.Relation({"u": [1, 2, 1, 2, 1], "v": [1, 1, 2, 2, 1], "y": [1.0, 2.0, 3.0, 4.0, 5.0]}, "panel", [B.Entity("u"), B.Entity("v")], dims=[2, 2])
    with pytest.raises(B.ArgumentError, match="more than once"):
        B.setDense(rel)


def test_refuses_fewer_than_half_of_the_cells(B):
    from bdf_amd.relation_data import check_model
    ids, y, _ = BR.listing()                                     # about 20 % of 37 x 29
    rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "panel", [B.Entity("u"), B.Entity("v")], dims=[37, 29])
    with pytest.raises(B.ArgumentError, match="at least half"):
        B.setDense(rel)
    # ... and a test split that takes more than half away is caught when a sampler is built
    rel = _relation(B)
    B.setDense(rel)
    B.assignToTest(rel, np.arange(1, 537))
    check_model(rel)                                             # 537 of 1073 listed: just half
    B.assignToTest(rel, np.arange(1, 3))
    with pytest.raises(B.ArgumentError, match="at least half"):
        check_model(rel)


def test_refuses_relation_features(B):
    from bdf_amd.relation_data import check_model
    rel = _relation(B)
    rel.F = np.ones((rel.data.nnz(), 2))
    with pytest.raises(B.ArgumentError, match="has features"):
        B.setDense(rel)
    rel = _relation(B)
    B.setDense(rel)
    rel.F = np.ones((rel.data.nnz(), 2))
    with pytest.raises(B.ArgumentError, match="has features"):
        check_model(rel)


def _other_models(B):
    return {
        "setProbit": lambda rel: B.setProbit(rel),
        "setCensored": lambda rel: B.setCensored(rel, np.zeros(rel.data.nnz(), dtype=np.int8)),
        "setInterval": lambda rel: B.setInterval(rel, rel.data.values - 1.0, rel.data.values + 1.0),
        "setBinned": lambda rel: B.setBinned(rel, [0.0, 1.0, 2.0]),
        "setOrdinal": lambda rel: B.setOrdinal(rel),
        "setRobust": lambda rel: B.setRobust(rel),
        "setWeights": lambda rel: B.setWeights(rel, np.ones(rel.data.nnz())),
        "setEntityNoise": lambda rel: B.setEntityNoise(rel, rel.entities[0]),
        "setLogit": lambda rel: B.setLogit(rel),
        "setCounts": lambda rel: B.setCounts(rel, 2),
        "setBackground": lambda rel: B.setBackground(rel, 0.1),
        "setRecommend": lambda rel: B.setRecommend(rel, 3),
    }


def _levels(B, vals, full=True):
    """a 6 x 5 relation whose values suit every setter: 0/1 for probit, logit and counts, 1 .. 4 for the ordinal model; full: every
    cell listed (setBackground wants an unlisted one: then 25 of the 30)"""
    ii, jj = np.meshgrid(np.arange(1, 7), np.arange(1, 6), indexing="ij")
    n = 30 if full else 25
    return B.Relation({"u": ii.ravel()[:n], "v": jj.ravel()[:n], "y": np.resize(np.asarray(vals, dtype=float), n)}, "panel",
                      [B.Entity("u"), B.Entity("v")], dims=[6, 5])


@pytest.mark.parametrize("name", ["setProbit", "setCensored", "setInterval", "setBinned", "setOrdinal", "setRobust", "setWeights", "setEntityNoise",
                                  "setLogit", "setCounts", "setBackground", "setRecommend"])
def test_refuses_every_noise_model_a_background_and_top_k_lists_in_either_order(B, name):
    from bdf_amd.relation_data import check_model
    vals = [1, 2, 3, 4] if name == "setOrdinal" else [0, 1]
    # the other model first: setDense refuses
    rel = _levels(B, vals, full=name != "setBackground")
    _other_models(B)[name](rel)
    with pytest.raises(B.ArgumentError, match="setDense"):
        B.setDense(rel)
    assert rel.model.dense is False
    # setDense first: the other setter refuses, at once
    rel = _levels(B, vals, full=name != "setBackground")
    B.setDense(rel)
    with pytest.raises(B.ArgumentError, match="setDense"):
        _other_models(B)[name](rel)
    # ... and a model that got there all the same is caught when a sampler is built
    rel = _levels(B, vals, full=name != "setBackground")
    _other_models(B)[name](rel)
    rel.model.dense = True
    with pytest.raises(B.ArgumentError, match="setDense"):
        check_model(rel)


def test_refuses_cells_of_new_rows_in_either_order(B):
    from bdf_amd.relation_data import check_model
    def case():
        u, v = B.Entity("u", F=np.random.default_rng(0).standard_normal((6, 3))), B.Entity("v")
        ii, jj = np.meshgrid(np.arange(1, 7), np.arange(1, 6), indexing="ij")
        rel = B.Relation({"u": ii.ravel(), "v": jj.ravel(), "y": np.arange(30.0)}, "panel", [u, v], dims=[6, 5])
        B.setNewRows(u, np.random.default_rng(1).standard_normal((2, 3)))
        return rel, u
    new = {"u": [1, 2], "v": [1, 2], "y": [0.5, np.nan]}
    rel, u = case()
    B.setNewTest(rel, u, new)
    with pytest.raises(B.ArgumentError, match="setDense"):
        B.setDense(rel)
    rel, u = case()
    B.setDense(rel)
    with pytest.raises(B.ArgumentError, match="setDense"):
        B.setNewTest(rel, u, new)
    rel, u = case()
    B.setNewTest(rel, u, new)
    rel.model.dense = True
    with pytest.raises(B.ArgumentError, match="setDense"):
        check_model(rel)


def test_refuses_the_spike_and_slab_prior_on_an_entity_in_either_order(B):
    from bdf_amd.relation_data import check_model, check_spike
    rel = _relation(B)
    rd = B.RelationData(rel)                                     # (an entity knows its relations once they are in a RelationData)
    B.setSpikeAndSlab(rel.entities[0])
    with pytest.raises(B.ArgumentError, match="setDense"):
        B.setDense(rel)
    rel = _relation(B)
    rd = B.RelationData(rel)
    B.setDense(rel)
    with pytest.raises(B.ArgumentError, match="setDense"):
        B.setSpikeAndSlab(rel.entities[1])
    rel.entities[1].spike = {"incl_a": 1.0, "incl_b": 1.0, "shape": 1.0, "rate": 1.0}
    with pytest.raises(B.ArgumentError, match="setDense"):
        check_model(rel)
    with pytest.raises(B.ArgumentError, match="setDense"):
        check_spike(rel.entities[1])
    assert rd is not None


def test_refuses_more_than_one_rank(B):
    from bdf_amd.relation_data import check_model
    rel = _relation(B)
    B.setDense(rel)
    check_model(rel, 1)
    with pytest.raises(B.ArgumentError, match="Relation panel has a dense matrix \\(setDense\\): one rank only"):
        check_model(rel, 2)


@pytest.mark.parametrize("who", ["bpmf_vb", "macau_hmc"])
def test_the_other_trainers_refuse_a_dense_relation(B, who):
    from bdf_amd._two_mode import relation_of
    rel = _relation(B)
    B.setDense(rel)
    with pytest.raises(B.ArgumentError, match="is dense"):
        relation_of(B.RelationData(rel), 8, who)


def test_what_works_passes_the_checks(B):
    """a sampled or set alpha, the test set, held-out cells as holes, setWaic and entity side information are all admitted"""
    from bdf_amd.relation_data import check_model, dense_matrix
    rel = B.denseRelation(DR.table(), "panel", [B.Entity("u", F=np.ones((37, 2))), B.Entity("v")])
    rel.model.alpha_sample = True
    B.setPrecision(rel, 3.0)
    B.setWaic(rel)
    B.setTest(rel, {"u": [1, 2], "v": [3, 4], "y": [0.0, 1.0]})
    check_model(rel)
    B.assignToTest(rel, np.arange(1, 216))
    check_model(rel)
    Y, holes = dense_matrix(rel)
    assert len(holes) == 215 and np.isnan(Y).sum() == 215 and rel.model.dense and rel.model.waic is not None


# ---- the identities ----------------------------------------------------------------------------------------------------------------
def test_row_systems_and_sums_equal_the_explicit_listing():
    """the row systems from (G, C) against the explicit listing cell by cell at N = 37, M = 29, for the rows of both modes, a shared
    and a per-row prior mean, one and two dense terms: to 1e-12 of max |P|; alpha's closed-form sum against math.fsum over all cells to
    1e-12 of the sum of its pieces' magnitudes"""
    N, M, D, alpha = 37, 29, 6, 2.0
    rng = np.random.default_rng(1)
    Y, Y2 = DR.table(N, M), DR.table(N, 23, seed=9)
    R, R2 = Y - Y.mean(), Y2 - Y2.mean()
    U, V, W = rng.standard_normal((N, D)), rng.standard_normal((M, D)), rng.standard_normal((23, D))
    A = rng.standard_normal((D, D))
    Lam = A @ A.T + D * np.eye(D)
    ids, _ = DR.listing(Y)
    ids2, _ = DR.listing(Y2)
    for mode0 in (0, 1):
        n, Rm, other, idm = (N, R, V, ids) if mode0 == 0 else (M, R.T, U, ids[:, ::-1])
        for mu in (rng.standard_normal(D), rng.standard_normal((n, D))):
            Pd, bd = DR.systems_dense([Rm], [other], [alpha], Lam, mu)
            Pe, be = DR.systems_explicit(n, idm, R.ravel(), other, alpha, Lam, mu)
            scale = np.abs(Pe).max()
            assert np.abs(Pe - Pd).max() <= 1e-12 * scale and np.abs(be - bd).max() <= 1e-12 * scale
    mu = rng.standard_normal((N, D))
    Pd, bd = DR.systems_dense([R, R2], [V, W], [alpha, 0.7], Lam, mu)
    Pe, be = DR.systems_explicit(N, ids, R.ravel(), V, alpha, Lam, mu)
    Pe, be = DR.systems_explicit(N, ids2, R2.ravel(), W, 0.7, Lam, mu, Pe, be)
    scale = np.abs(Pe).max()
    assert np.abs(Pe - Pd).max() <= 1e-12 * scale and np.abs(be - bd).max() <= 1e-12 * scale
    p = DR.sse_pieces(R, U, V)
    assert abs(DR.sse_closed(R, U, V) - DR.sse_explicit(R, U, V)) <= 1e-12 * (p[0] + 2.0 * abs(p[1]) + p[2])


def test_the_imputing_map_touches_the_holes_only():
    rng = np.random.default_rng(2)
    R, U, V = rng.standard_normal((6, 5)), rng.standard_normal((6, 3)), rng.standard_normal((5, 3))
    holes, z = np.array([[0, 1], [5, 4], [2, 2]]), np.array([0.5, -1.0, 2.0])
    out = DR.impute(R, holes, U, V, 4.0, z)
    mask = np.zeros((6, 5), dtype=bool)
    mask[holes[:, 0], holes[:, 1]] = True
    assert np.array_equal(out[~mask], R[~mask])
    assert np.allclose(out[holes[:, 0], holes[:, 1]], [U[0] @ V[1] + 0.25, U[5] @ V[4] - 0.5, U[2] @ V[2] + 1.0], rtol=1e-15)
    assert np.array_equal(DR.impute(R, holes[:0], U, V, 4.0, z[:0]), R)


def test_the_restated_chain_learns_planted_data():
    """the numpy chain on the (G, C) form recovers planted rank-3 data to its noise level, with alpha fixed and sampled; with a fifth
    of the cells as imputed holes the held-out RMSE stays near the noise (what tests/test_gpu_dense.py compares the device with)"""
    Y = DR.table(60, 40, seed=3, rank=3, noise=0.3)
    for sample_alpha in (False, True):
        U, V, mean, trace = DR.gibbs(Y, 6, 10.0, 40, 0, sample_alpha=sample_alpha)
        rmse = float(np.sqrt(np.mean((U @ V.T + mean - Y) ** 2)))
        assert rmse < 0.45, rmse
        if sample_alpha:
            assert 5.0 < trace[-1] < 20.0, trace[-1]          # the planted noise precision is 1 / 0.09 = 11.1
    Yp, held = DR.planted(0)
    got = [DR.gibbs_holes_rmse(Yp, held, 8, 10.0, 40, 20, s) for s in (0, 1)]
    assert all(0.3 < g < 0.36 for g in got), got


# ---- csrc/dense.h on the host ----------------------------------------------------------------------------------------------------
_HOST_SRC = r"""
#include <cstdio>
#include "dense.h"
int main() {
    double a, b, c;
    while (scanf("%lf %lf %lf", &a, &b, &c) == 3) printf("%.17g %.17g\n", bdf_dense_all_cells(a, b, c), bdf_dense_hole(a, b, c));
    return 0;
}
"""


def test_dense_header_on_the_host():
    cxx = [shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")]
    if cxx[0] is None:
        cxx = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "c++"]
    td = tempfile.mkdtemp()
    try:
        open(os.path.join(td, "t.cpp"), "w").write(_HOST_SRC)
        subprocess.run(cxx + ["-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "bayesiandatafusion.jl_amd", "csrc"), os.path.join(td, "t.cpp"),
                              "-o", os.path.join(td, "t")], check=True)
        rng = np.random.default_rng(5)
        rows = rng.standard_normal((50, 3))
        rows[:, 2] = rng.uniform(0.1, 9.0, 50)
        text = "".join(" ".join("%.17g" % x for x in r) + "\n" for r in rows)
        out = subprocess.run([os.path.join(td, "t")], input=text, capture_output=True, text=True, check=True).stdout
        got = np.array([float(t) for t in out.split()]).reshape(50, 2)
    finally:
        shutil.rmtree(td, ignore_errors=True)
    a, b, c = rows.T
    assert np.array_equal(got[:, 0], (a - 2.0 * b) + c)
    assert np.array_equal(got[:, 1], a + b / np.sqrt(c))


# ---- the C ABI and the build's listing ----------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_documented(B):
    h = open(os.path.join(ROOT, "include", "bdf.h")).read()
    jl = open(os.path.join(ROOT, "julia", "BDFHip.jl")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("bdf_dense_product", "bdf_dense_prior", "bdf_dense_sse", "bdf_dense_impute"):
        assert name + "(" in h and name in B.declared_symbols() and (":" + name) in jl and name in doc
    assert "#define BDF_P_DENSE 24" in h and "dense_R" in h and "dense_R::Ptr{Cvoid}" in jl
    from bdf_amd import _lib
    assert _lib.P_DENSE == 24 and DR.P_DENSE == 24
    purposes = [int(x.split()[2]) for x in h.splitlines() if x.startswith("#define BDF_P_")]
    assert len(purposes) == len(set(purposes))                   # no stream purpose is used twice


def test_new_kernels_keep_their_registers():
    """the build's resource listing (csrc/k_dense.o.res): no kernel keeps registers in scratch memory, except that of the one-wave fold
    the D = 64 variant has the 528 bytes per lane that wl_factor<64> brings to every kernel that takes it; the VGPR counts and
    occupancies are those DESIGN.md section 25 quotes"""
    res = {k: v for k, v in _resources("k_dense").items() if "k_dmat_" in k}
    assert len(res) == 17, sorted(res)
    for k, (vgprs, scratch, occ) in res.items():
        if "k_dmat_foldILi64" in k:
            assert scratch == _resources("k_feat_beta")["13k_solve_smallILi64EEEviiPKdS2_S2_PdPi"][1], (k, scratch)
        else:
            assert scratch == 0, (k, scratch)
        assert vgprs <= 256 and occ >= 1
    quoted = {"k_dmat_productILi1ELb0": (69, 7), "k_dmat_productILi2ELb0": (96, 5), "k_dmat_productILi4ELb0": (145, 3),
              "k_dmat_productILi1ELb1": (79, 6), "k_dmat_productILi2ELb1": (106, 4), "k_dmat_productILi4ELb1": (154, 3),
              "k_dmat_mu_rowsILi16": (32, 8), "k_dmat_mu_rowsILi32": (62, 8), "k_dmat_mu_rowsILi64": (124, 4),
              "k_dmat_imputeILi1ELi1": (34, 8), "k_dmat_imputeILi4ELi1": (86, 5), "k_dmat_imputeILi4ELi2": (88, 5)}
    for name, (vgprs, occ) in quoted.items():
        hit = [v for k, v in res.items() if name in k]
        assert len(hit) == 1, name
        assert hit[0][0] <= vgprs and hit[0][2] >= occ, (name, hit[0])
