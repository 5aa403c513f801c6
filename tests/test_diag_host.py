"""Convergence diagnostics (setDiagnostics) on the host (no GPU): the restatement of tests/diag_restatement.py
against what is known of AR(1) series, trends and the smallest chains by hand; the setter and what it refuses; macau()'s three
refusals that need no device; the registry's record, the other trainers and two ranks; the resource listing the build leaves for
the kernels of k_diag.hip (no scratch) and the header's declarations in the bindings."""
import os
import re

import numpy as np
import pytest

import diag_restatement as DR
from test_newrows_host import _resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phi", [0.0, 0.5, 0.9])
def test_ess_of_ar1_series_is_the_theoretical_one(phi):
    """n = 1000, 200 fixed seeds: the median of ESS / n within 15 % of (1 - phi) / (1 + phi)"""
    x = np.concatenate([DR.ar1(np.random.default_rng(1000 + seed), 1000, phi) for seed in range(200)], axis=1)
    _, ess, _ = DR.diagnostics(x)
    ratio, want = float(np.median(ess / 1000.0)), (1.0 - phi) / (1.0 + phi)
    print(f"phi = {phi}: median ESS / n = {ratio:.4f}, theory {want:.4f}")
    assert abs(ratio - want) <= 0.15 * want


def test_rhat_flags_a_trend_and_passes_iid_series():
    rng = np.random.default_rng(7)
    iid = rng.standard_normal((200, 50))
    trend = rng.standard_normal((200, 50)) + np.linspace(0.0, 3.0, 200)[:, None]      # three noise standard deviations long
    assert (DR.diagnostics(trend)[0] > 1.1).all()
    assert (DR.diagnostics(iid)[0] < 1.1).all()


def test_the_cap_binds_for_an_antithetic_series():
    """phi = -0.5 at n = 200: tau falls below 1 / log10(n) and ESS is the cap, n log10(n)"""
    _, ess, _ = DR.diagnostics(DR.ar1(np.random.default_rng(3), 200, -0.5))
    assert ess[0] == 200 * np.log10(200)


@pytest.mark.parametrize("x", [[1.0, 2.0, 4.0, 3.0], [1.0, 2.0, 100.0, 4.0, 3.0]])
def test_four_and_five_draws_by_hand(x):
    """h = 2, chains (1, 2) and (4, 3) -- with five draws the middle one is left out: means 1.5 and 3.5, variances 0.5 and 0.5, W =
    0.5; var+ = 0.5 / 2 + 2^2 / 2 = 2.25; R-hat = sqrt(4.5).  acov_j(1) = (1 / 2)(-0.5)(0.5) = -0.125 in both chains: rho_1 = 1 - (0.5
    + 0.125) / 2.25 = 13 / 18; P_0 = 31 / 18, the only pair; tau = 22 / 9; cap = 4 log10(4) = 2.408 > 4 / tau = 18 / 11"""
    rhat, ess, mcse = (float(v[0]) for v in DR.diagnostics(np.array(x)[:, None]))
    assert rhat == pytest.approx(np.sqrt(4.5), rel=1e-15)
    assert ess == pytest.approx(18.0 / 11.0, rel=1e-14)
    assert mcse == pytest.approx(np.sqrt(2.25 * 11.0 / 18.0), rel=1e-14)


def test_series_without_figures_give_nan():
    x = np.random.default_rng(1).standard_normal((9, 4))
    x[:, 1] = 2.5                                            # constant
    x[3, 2] = np.inf
    x[0, 3] = np.nan
    rhat, ess, mcse = DR.diagnostics(x)
    for v in (rhat, ess, mcse):
        assert np.isnan(v).tolist() == [False, True, True, True]
    s = DR.summary(rhat, ess, 1.1, 100.0)
    assert s["n_constant"] == 3 and s["max_rhat"] == rhat[0] and s["min_ess"] == ess[0] and s["n_ess_low"] == 1
    # constant within each half is W = 0 too, whatever the halves' levels
    assert np.isnan(DR.diagnostics(np.array([1.0, 1.0, 1.0, 2.0, 2.0, 2.0])[:, None])[0][0])


def test_monotone_minimum_and_stop():
    P = np.array([[1.5, 1.5, 1.0], [0.4, 0.9, -0.1], [0.6, 0.2, 5.0], [-0.1, 0.3, 5.0]])
    tau, kept = DR.geyer(P)
    assert tau.tolist() == pytest.approx([-1 + 2 * (1.5 + 0.4 + 0.4), -1 + 2 * (1.5 + 0.9 + 0.2 + 0.2), 1.0])
    assert np.isnan(kept[3, 0]) and kept[2, 0] == 0.4 and np.isnan(kept[1:, 2]).all()


# ---- the setter -------------------------------------------------------------------------------------------------------------------
def _relation(B, test=40):
    rng = np.random.default_rng(0)
    i, j = np.nonzero(rng.random((30, 20)) < 0.5)
    rel = B.Relation({"u": i + 1, "v": j + 1, "y": rng.standard_normal(len(i))}, "plays", [B.Entity("u"), B.Entity("v")], dims=[30, 20])
    if test:
        B.assignToTest(rel, np.arange(1, test + 1))
    return rel


def test_setter_round_trips_and_clears(B):
    rel = _relation(B)
    before = B.toStr(rel)
    assert rel.model.diagnostics is None and B.RelationModel().diagnostics is None
    assert B.setDiagnostics(rel) is None
    assert rel.model.diagnostics == {"pointwise": False, "rhat_cut": 1.1, "ess_cut": 100.0}
    B.setDiagnostics(rel, pointwise=True, rhat_cut=1, ess_cut=np.float64(400))
    m = rel.model.diagnostics
    assert m == {"pointwise": True, "rhat_cut": 1.0, "ess_cut": 400.0} and isinstance(m["rhat_cut"], float) and isinstance(m["ess_cut"], float)
    assert B.toStr(rel) == before                            # (toStr does not show it)
    B.setDiagnostics(rel, False)
    assert rel.model.diagnostics is None
    assert "setDiagnostics" in B.__dict__ and "split R-hat" in B.setDiagnostics.__doc__


@pytest.mark.parametrize("kw, message", [
    (dict(on=1), "on = true / false and pointwise = true / false"), (dict(pointwise="yes"), "on = true / false"),
    (dict(on=False, pointwise=True), "returns no pointwise columns"),
    (dict(rhat_cut=0.99), "rhat_cut = 0.99 must be a finite number, at least 1"), (dict(rhat_cut=float("nan")), "rhat_cut = nan"),
    (dict(rhat_cut="1.1"), "rhat_cut = 1.1 must be"), (dict(rhat_cut=True), "rhat_cut = True"),
    (dict(ess_cut=-1.0), "ess_cut = -1.0 must be a finite number, at least 0"), (dict(ess_cut=float("inf")), "ess_cut = inf")])
def test_setter_refuses(B, kw, message):
    rel = _relation(B)
    with pytest.raises(B.ArgumentError, match=r"Relation plays: .*" + re.escape(message)):
        B.setDiagnostics(rel, **kw)
    assert rel.model.diagnostics is None


# ---- macau()'s refusals ahead of the engine -----------------------------------------------------------------------------------------
def test_macau_refuses_a_later_relation(B):
    u, v, w = B.Entity("u"), B.Entity("v"), B.Entity("w")
    rng = np.random.default_rng(0)
    i, j = np.nonzero(rng.random((30, 20)) < 0.5)
    y = rng.standard_normal(len(i))
    r1 = B.Relation({"u": i + 1, "v": j + 1, "y": y}, "plays", [u, v], dims=[30, 20])
    r2 = B.Relation({"u": i + 1, "w": j + 1, "y": y}, "skips", [u, w], dims=[30, 20])
    B.assignToTest(r1, np.arange(1, 41))
    B.assignToTest(r2, np.arange(1, 41))
    rd = B.RelationData(r1)
    B.addRelation(rd, r2)
    B.setDiagnostics(r2)
    with pytest.raises(B.ArgumentError, match=r"skips asks for convergence diagnostics \(setDiagnostics\) but is not the first relation"):
        B.macau(rd, num_latent=4, burnin=1, psamples=8, verbose=False)


def test_macau_refuses_a_relation_without_test_cells(B):
    rel = _relation(B, test=0)
    B.setDiagnostics(rel)
    with pytest.raises(B.ArgumentError, match=r"setDiagnostics.*the first relation has no test cells"):
        B.macau(B.RelationData(rel), num_latent=4, burnin=1, psamples=8, verbose=False)


@pytest.mark.parametrize("psamples", [0, 3])
def test_macau_refuses_fewer_than_four_draws(B, psamples):
    rel = _relation(B)
    B.setDiagnostics(rel)
    with pytest.raises(B.ArgumentError, match=r"setDiagnostics.*psamples must be at least 4"):
        B.macau(B.RelationData(rel), num_latent=4, burnin=1, psamples=psamples, verbose=False)


# ---- the registry -----------------------------------------------------------------------------------------------------------------
def test_registry_record(B):
    from bdf_amd import model_options as MO
    rec = MO.OPTION["diagnostics"]
    assert rec.scope == MO.RELATION and rec.field == "diagnostics" and rec.one_rank is True
    assert rec.phrase == "convergence diagnostics (setDiagnostics)" and rec.trainer == "keeps no draws of the predictions"
    rel = _relation(B)
    assert not rec.present(rel)
    B.setDiagnostics(rel)
    assert rec.present(rel)
    # it only reads what the prediction computes: no row of the table, no pair left to the build
    assert not [p for p in MO.REFUSED if "diagnostics" in p] and not [p for p in MO._REFUSED_ONLY_AT_BUILD if "diagnostics" in p]


def test_it_goes_with_every_noise_model_and_prior(B):
    from bdf_amd.relation_data import check_model
    def probit(r):
        r.data.values[:] = (r.data.values > 0).astype(np.float64)
        r.test_vec.values[:] = (r.test_vec.values > 0).astype(np.float64)
        B.setProbit(r)

    n = _relation(B).data.nnz()
    for setter in (probit, lambda r: B.setCensored(r, np.zeros(n, dtype=np.int8)), lambda r: B.setRobust(r, 4.0),
                   lambda r: B.setEntityNoise(r, r.entities[0]), lambda r: B.setBias(r, r.entities[1]), lambda r: B.setWaic(r),
                   lambda r: B.setRecommend(r, 3), lambda r: setattr(r.model, "alpha_sample", True), lambda r: B.setSpikeAndSlab(r.entities[0])):
        for first in (True, False):
            r = _relation(B)
            B.RelationData(r)
            if first:
                B.setDiagnostics(r)
                setter(r)
            else:
                setter(r)
                B.setDiagnostics(r)
            check_model(r)
            assert r.model.diagnostics is not None


@pytest.mark.parametrize("who", ["bpmf_vb", "macau_hmc"])
def test_the_other_trainers_refuse_it(B, who):
    from bdf_amd._two_mode import relation_of
    rel = _relation(B)
    B.setDiagnostics(rel)
    with pytest.raises(B.ArgumentError, match=who + r" keeps no draws of the predictions; plays has convergence diagnostics \(setDiagnostics\) \(use macau\)"):
        relation_of(B.RelationData(rel), 8, who)


# ---- the build's listing and the bindings ------------------------------------------------------------------------------------------
def test_diag_kernels_use_no_scratch():
    res = _resources("k_diag")
    push = {k: v for k, v in res.items() if "k_diag_pushI" in k}
    compute = {k: v for k, v in res.items() if re.search(r"\d+k_diagI", k)}
    final = {k: v for k, v in res.items() if "k_diag_final" in k}
    assert len(push) == 9 and len(compute) == 2 and len(final) == 1        # <modes 2..4> x <vector width, row pieces>; the tile in LDS or not
    for k, v in {**push, **compute, **final}.items():
        assert v["ScratchSize"] == 0, (k, v)
    assert all(v["Occupancy"] >= 3 for v in push.values())
    assert all(v["VGPRs"] <= 64 for v in compute.values())                 # (a wave per workgroup: the tile, not the registers, bounds the occupancy)


def test_every_export_is_declared_and_bound(B):
    h = open(os.path.join(ROOT, "include", "bdf.h")).read()
    jl = open(os.path.join(ROOT, "julia", "BDFHip.jl")).read()
    names = sorted(set(re.findall(r"\b(bdf_diag_[a-z_]+)\s*\(", h)))
    assert names == ["bdf_diag_compute", "bdf_diag_create", "bdf_diag_destroy", "bdf_diag_plane", "bdf_diag_push", "bdf_diag_write"]
    for n in names:
        assert n in B.declared_symbols() and (":" + n) in jl
