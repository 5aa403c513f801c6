"""Hamiltonian Monte Carlo BPMF (src/macau_hmc.jl) on the host: HMCModel, the numpy restatement the GPU tests compare
against (energies, gradient, integrator), argument checks, and the kernels' resource usage.  No GPU needed."""
import glob
import math
import os
import re

import numpy as np
import pytest

import hmc_restatement as H
import vb_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hmcmodel_constructor_matches_the_reference(B):
    """HMCModel(num_latent, N, Ldiag) (macau_hmc.jl:13-18): momentum = zeros(D, N), G = repmat(Ldiag, 1, N)"""
    m = B.HMCModel(3, 5, [1.0, 2.0, 5.0])
    assert m.momentum.shape == (3, 5) and not m.momentum.any()
    assert np.array_equal(m.G, np.array([[1.0] * 5, [2.0] * 5, [5.0] * 5]))
    with pytest.raises(B.ArgumentError):
        B.HMCModel(3, 5, [1.0, 2.0])


def test_column_dot_literal():
    """test/macau_hmc.jl:4-7: column_dot(X1, X2, 8, 1) == dot(X1[:,8], X2[:,1])"""
    rng = np.random.default_rng(1)
    X1, X2 = rng.random((5, 10)), rng.random((5, 3))
    assert abs(H.column_dot(X1, X2, 8, 1) - np.dot(X1[:, 7], X2[:, 0])) < 1e-14
    with pytest.raises(ValueError):
        H.column_dot(X1, rng.random((4, 3)), 1, 1)


def _state(D, Nu, Nv, seed):
    rng = np.random.default_rng(seed)
    U, V = rng.standard_normal((D, Nu)) * 0.5, rng.standard_normal((D, Nv)) * 0.5
    mu = [rng.standard_normal(D) * 0.3, rng.standard_normal(D) * 0.3]
    Lam = []
    for _ in range(2):
        A = rng.standard_normal((D, D))
        Lam.append(A @ A.T / D + np.eye(D))
    return U, V, mu, Lam


def test_kinetic_and_potential_match_brute_force():
    """computeKinetic = 1/2 sum(r^2 G + log G); computePotential = alpha/2 sum_obs (u.v - val)^2 (duplicates one by one)
    + sum_n (1/2 u_n' Lambda u_n - mu' Lambda u_n) for both entities"""
    D, Nu, Nv, alpha = 3, 12, 9, 1.7
    uid, vid, vals, _, _, _ = R.make_case(Nu, Nv, 60, seed=4, ntest=1)
    val = vals - vals.mean()
    U, V, mu, Lam = _state(D, Nu, Nv, 2)
    rng = np.random.default_rng(3)
    r, G = rng.standard_normal((D, Nu)), rng.random((D, Nu)) + 0.5
    kin = 0.5 * sum(r[k, n] ** 2 * G[k, n] + math.log(G[k, n]) for k in range(D) for n in range(Nu))
    assert abs(H.compute_kinetic(r, G) - kin) < 1e-12 * abs(kin)
    assert abs(H.compute_kinetic_vec(r, G) - kin) < 1e-12 * abs(kin)
    e = alpha / 2 * sum((U[:, uid[i] - 1] @ V[:, vid[i] - 1] - val[i]) ** 2 for i in range(len(uid)))
    for S, m, Lm in ((U, mu[0], Lam[0]), (V, mu[1], Lam[1])):
        e += sum(0.5 * S[:, n] @ Lm @ S[:, n] - m @ Lm @ S[:, n] for n in range(S.shape[1]))
    for f in (H.compute_potential, H.compute_potential_vec):
        assert abs(f(uid, vid, val, alpha, U, V, mu, Lam) - e) < 1e-11 * abs(e)


@pytest.mark.parametrize("D", [1, 3])
def test_gradient_is_the_finite_difference_of_the_potential(D):
    """on duplicate-free data the gradient (summed duplicates) and the potential (one by one) describe the same function"""
    Nu, Nv, alpha = 8, 7, 2.0
    rng = np.random.default_rng(D)
    pairs = rng.choice(Nu * Nv, 30, replace=False)
    uid, vid = pairs // Nv + 1, pairs % Nv + 1
    val = rng.standard_normal(30)
    U, V, mu, Lam = _state(D, Nu, Nv, 10 + D)
    Udata = H.sparse_data(uid, vid, val, Nu, Nv)
    Vdata = Udata.T.tocsc()
    Vdata.sort_indices()
    h = 1e-6
    for (S, O_, data, e) in ((U, V, Udata, 0), (V, U, Vdata, 1)):
        g_all = H.grad_all(S, O_, data, Lam[e], mu[e], alpha)
        for n in range(S.shape[1]):
            g = H.grad(n, S, O_, data, Lam[e], mu[e], alpha)
            assert np.allclose(g, g_all[:, n], rtol=1e-12, atol=1e-12)
            for k in range(D):
                Sp, Sm = S.copy(), S.copy()
                Sp[k, n] += h
                Sm[k, n] -= h
                args = lambda X: (X, V) if e == 0 else (U, X)
                fd = (H.compute_potential(uid, vid, val, alpha, *args(Sp), mu, Lam) -
                      H.compute_potential(uid, vid, val, alpha, *args(Sm), mu, Lam)) / (2 * h)
                assert abs(fd - g[k]) < 1e-6 * max(1.0, abs(g[k])), (e, n, k, fd, g[k])


def _trajectory_dH(eps, L, G):
    """dH of one trajectory of L steps from a fixed non-trivial state, G overriding the mass"""
    D, Nu, Nv, alpha = 3, 30, 25, 2.0
    uid, vid, vals, _, _, _ = R.make_case(Nu, Nv, 200, seed=7, ntest=1)
    _, first = np.unique(uid * (Nv + 1) + vid, return_index=True)        # duplicate-free: the gradient is the potential's
    uid, vid, vals = uid[first], vid[first], vals[first]
    val = vals - vals.mean()
    Udata = H.sparse_data(uid, vid, val, Nu, Nv)
    Vdata = Udata.T.tocsc()
    Vdata.sort_indices()
    st = H.State(D, Nu, Nv, G)
    st.U, st.V, st.mu, st.Lam = _state(D, Nu, Nv, 5)
    st.rU, st.rV = H.sample_momentum(st.GU, 3, 1, 0), H.sample_momentum(st.GV, 3, 1, 1)
    k0 = H.compute_kinetic_vec(st.rU, st.GU) + H.compute_kinetic_vec(st.rV, st.GV)
    p0 = H.compute_potential_vec(uid, vid, val, alpha, st.U, st.V, st.mu, st.Lam)
    H.leapfrog(st, Udata, Vdata, alpha, L, 1, eps, True)
    k1 = H.compute_kinetic_vec(st.rU, st.GU) + H.compute_kinetic_vec(st.rV, st.GV)
    p1 = H.compute_potential_vec(uid, vid, val, alpha, st.U, st.V, st.mu, st.Lam)
    return p0 - p1 + k0 - k1


def test_halving_eps_quarters_dH_with_a_unit_mass():
    """on duplicate-free data with G = 1 the leapfrog is a consistent second-order integrator: over a trajectory of fixed
    length L eps, |dH| ~ eps^2.  With the reference's G = 5 the position step u += eps r ignores G^-1 and dH does
    not shrink at all (the mass quirk)."""
    r = [abs(_trajectory_dH(eps, L, 1.0)) for eps, L in ((0.004, 10), (0.002, 20), (0.001, 40))]
    for a, b in zip(r, r[1:]):
        assert 3.5 < a / b < 4.5, r
    q = [abs(_trajectory_dH(eps, L, 5.0)) for eps, L in ((0.004, 10), (0.002, 20))]
    assert q[0] / q[1] < 2.5, q


def test_loop_and_vectorised_restatements_agree():
    Nu, Nv, D = 25, 20, 3
    uid, vid, vals, tu, tv, tval = R.make_case(Nu, Nv, 150, seed=11, ntest=40)
    assert len(set(zip(uid.tolist(), vid.tolist()))) < len(uid)            # duplicates
    assert Nu not in uid and Nv not in vid                                  # rows with no observations
    out = [H.run(uid, vid, vals, tu, tv, tval, Nu, Nv, D, 2.0, seed=5, burnin=2, psamples=3, L=4, prior_freq=2, eps=0.05,
                 clamp=(1.0, 5.0), vectorised=v) for v in (False, True)]
    a, b = out
    for f in ("U", "V", "rU", "rV"):
        x, y = getattr(a["state"], f), getattr(b["state"], f)
        assert np.max(np.abs(x - y)) <= 1e-10 * max(1.0, np.max(np.abs(y))), f
    for e in range(2):
        assert np.allclose(a["state"].mu[e], b["state"].mu[e], rtol=1e-10, atol=1e-12)
        assert np.allclose(a["state"].Lam[e], b["state"].Lam[e], rtol=1e-10, atol=1e-12)
    assert [r["accepted"] for r in a["records"]] == [r["accepted"] for r in b["records"]]
    for ra, rb in zip(a["records"], b["records"]):
        assert abs(ra["dH"] - rb["dH"]) < 1e-8 * max(1.0, abs(rb["pot_s"]))
    assert abs(a["rmse"] - b["rmse"]) < 1e-12 and abs(a["rmse_avg"] - b["rmse_avg"]) < 1e-12
    assert (a["eps"], a["L"]) == (b["eps"], b["L"])


def test_macau_hmc_argument_errors(B):
    """every ArgumentError is raised before a device is touched (this test runs without a GPU)"""
    Nu, Nv = 20, 15
    rd = R.relation_data(B, R.make_case(Nu, Nv, 100, seed=1, ntest=10), Nu, Nv)
    bad = [dict(num_latent=0), dict(num_latent=65), dict(L=0), dict(L_inner=0), dict(prior_freq=0), dict(eps=0.0),
           dict(eps=-1.0), dict(eps=float("inf")), dict(eps=float("nan")), dict(burnin=-1), dict(psamples=-1),
           dict(clamp=[1.0]), dict(reset_model=False)]
    for kw in bad:
        with pytest.raises(B.ArgumentError):
            B.macau_hmc(rd, verbose=False, **kw)
    t = B.Relation({"a": [1, 2, 3], "b": [1, 2, 1], "c": [2, 1, 1], "y": [1.0, 2.0, 3.0]}, "t",
                   [B.Entity("a"), B.Entity("b"), B.Entity("c")])
    with pytest.raises(B.ArgumentError):
        B.macau_hmc(B.RelationData(t), num_latent=3, verbose=False)
    F = np.eye(Nu)
    rel = B.Relation({"u": [1, 2, 3], "v": [1, 2, 1], "y": [1.0, 2.0, 3.0]}, "f", [B.Entity("u", F=F), B.Entity("v")],
                     dims=[Nu, Nv])
    with pytest.raises(B.ArgumentError):
        B.macau_hmc(B.RelationData(rel), num_latent=3, verbose=False)


def test_hmc_kernels_use_no_scratch():
    """the build's resource report (csrc/k_hmc.o.res): no k_hmc_* kernel keeps registers in scratch memory"""
    res = {}
    for f in glob.glob(os.path.join(ROOT, "bayesiandatafusion.jl_amd", "csrc", "*.o.res")):
        name = None
        for line in open(f):
            m = re.search(r"remark: \s*(Function Name|ScratchSize \[bytes/lane\]|VGPRs Spill): (\S+)", line)
            if not m:
                continue
            if m.group(1) == "Function Name":
                name = m.group(2)
                res[name] = {}
            elif name is not None:
                res[name][m.group(1)] = int(m.group(2))
    hmc = {k: v for k, v in res.items() if "k_hmc_" in k}
    assert len([k for k in hmc if "k_hmc_leap" in k]) == 3, sorted(res)            # DP = 16, 32, 64
    for name in ("k_hmc_accept", "k_hmc_restore", "k_hmc_predict"):
        assert any(name in k for k in hmc), name
    for k, v in hmc.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v.get("VGPRs Spill", 0) == 0, (k, v)
