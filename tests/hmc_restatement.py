"""A numpy restatement of src/macau_hmc.jl (macau_hmc, sample!, hmc_update_u!, subtract_grad!, grad, computeKinetic,
computePotential, update_yhat_post!), line by line, for the HMC tests.

`run(...)` follows the reference's loops (one row, one observation at a time); `vectorised=True` computes the same gradient
and energies for all rows at once (scipy sparse products), for full-size data.  Every random number comes from the
library's Philox streams through the oracle (DESIGN.md "RNG contract"): the momentum of row n of entity e at iteration i is
oracle.normals(seed, i, 10, e, n, D) / sqrt(G), the Metropolis uniform is the first double of oracle.draw(seed, i, 11, 0, 0,
0), and the prior draw is oracle.hyper_params + oracle.hyper_draw with entity tag e.
"""
import math

import numpy as np
import scipy.sparse as sp

from oracle import oracle as O

P_HMC_MOMENTUM, P_HMC_ACCEPT = 10, 11


def uniform(seed, sweep):
    o = O.draw(seed, sweep, P_HMC_ACCEPT, 0, 0, 0)
    x = (int(o[1]) << 32) | int(o[0])
    return ((x >> 11) + 0.5) * 2.0 ** -53


def sample_momentum(G, seed, sweep, tag):
    """sample!(m) (macau_hmc.jl:153-160): momentum[k, n] = randn() / sqrt(G[k, n])"""
    D, N = G.shape
    mom = np.zeros((D, N))
    for n in range(N):
        z = O.normals(seed, sweep, P_HMC_MOMENTUM, tag, n, D)
        for k in range(D):
            mom[k, n] = z[k] / math.sqrt(G[k, n])
    return mom


def column_dot(X, Y, i, j):
    """column_dot (:246-255), 1-based i, j"""
    if X.shape[0] != Y.shape[0]:
        raise ValueError("X and Y must have the same number of rows.")
    d = 0.0
    for k in range(X.shape[0]):
        d += X[k, i - 1] * Y[k, j - 1]
    return d


def compute_kinetic(mom, G):
    """computeKinetic (:206-215)"""
    kin = 0.0
    for m, g in zip(mom.ravel(order="F"), G.ravel(order="F")):
        kin += m * m * g + math.log(g)
    return 0.5 * kin


def compute_kinetic_vec(mom, G):
    return 0.5 * float(np.sum(mom * mom * G + np.log(G)))


def compute_potential(uid, vid, val, alpha, U, V, mu, Lam):
    """computePotential (:218-243): the observations one by one (duplicates not summed)"""
    energy = 0.0
    for i in range(len(uid)):
        energy += (column_dot(U, V, uid[i], vid[i]) - val[i]) ** 2
    energy *= alpha / 2
    energy += np.sum(Lam[0] * (U @ U.T)) / 2
    energy += np.sum(Lam[1] * (V @ V.T)) / 2
    energy -= mu[0] @ Lam[0] @ U.sum(axis=1)
    energy -= mu[1] @ Lam[1] @ V.sum(axis=1)
    return float(energy)


def compute_potential_vec(uid, vid, val, alpha, U, V, mu, Lam):
    d = np.einsum("kn,kn->n", U[:, uid - 1], V[:, vid - 1])
    energy = float(np.sum((d - val) ** 2)) * (alpha / 2)
    energy += np.sum(Lam[0] * (U @ U.T)) / 2
    energy += np.sum(Lam[1] * (V @ V.T)) / 2
    energy -= mu[0] @ Lam[0] @ U.sum(axis=1)
    energy -= mu[1] @ Lam[1] @ V.sum(axis=1)
    return float(energy)


def grad(n, sample, Vsample, Udata, Lam, mu, alpha):
    """grad (:228-244), n 0-based; Udata: scipy CSC, N_other x N"""
    un = sample[:, n]
    idx = slice(Udata.indptr[n], Udata.indptr[n + 1])
    ff = Udata.indices[idx]
    rr = Udata.data[idx]
    MM = Vsample[:, ff]
    return -alpha * (MM @ rr - (MM @ MM.T) @ un) - Lam @ (mu - un)


def grad_all(sample, Vsample, Udata, Lam, mu, alpha):
    """grad for every row at once (D x N)"""
    P = Udata.T.tocsr()
    coo = P.tocoo()
    b = np.asarray(P @ Vsample.T).T
    d = np.einsum("ke,ke->e", Vsample[:, coo.col], sample[:, coo.row])
    Q = sp.csr_matrix((d, (coo.row, coo.col)), shape=P.shape)
    Au = np.asarray(Q @ Vsample.T).T
    return -alpha * (b - Au) - Lam @ (mu[:, None] - sample)


def subtract_grad(mom, sample, Vsample, Udata, Lam, mu, alpha, eps, vectorised):
    """subtract_grad! (:196-211)"""
    if vectorised:
        mom -= eps * grad_all(sample, Vsample, Udata, Lam, mu, alpha)
        return
    for n in range(sample.shape[1]):
        tmp = grad(n, sample, Vsample, Udata, Lam, mu, alpha)
        for k in range(mom.shape[0]):
            mom[k, n] -= eps * tmp[k]


def hmc_update_u(mom, sample, Vsample, Udata, Lam, mu, alpha, L, eps, vectorised):
    """hmc_update_u! (:163-191)"""
    subtract_grad(mom, sample, Vsample, Udata, Lam, mu, alpha, eps / 2, vectorised)
    for i in range(1, L + 1):
        sample += eps * mom
        if i < L:
            subtract_grad(mom, sample, Vsample, Udata, Lam, mu, alpha, eps, vectorised)
    subtract_grad(mom, sample, Vsample, Udata, Lam, mu, alpha, eps / 2, vectorised)


def sparse_data(uid, vid, val, Nu, Nv):
    """Udata = sparse(vid, uid, val, N_v, N_u): duplicates summed into one entry, rows sorted in every column"""
    U = sp.coo_matrix((val, (vid - 1, uid - 1)), shape=(Nv, Nu)).tocsc()
    U.sum_duplicates()
    U.sort_indices()
    return U


def clamp_(x, clamp):
    if len(clamp):
        x[x < clamp[0]] = clamp[0]
        x[x > clamp[1]] = clamp[1]
    return x


def update_yhat_post(yhat_post, yhat_raw, i, burnin):
    """update_yhat_post! (:277-288)"""
    if i <= burnin + 1:
        yhat_post[:] = yhat_raw
        return yhat_post
    n = i - burnin - 1
    yhat_post[:] = (n * yhat_post + yhat_raw) / (n + 1)
    return yhat_post


class State:
    """the reset! state (samples 0, mu 0, Lambda 5 I) and two HMCModels (G = 5, or the override)"""

    def __init__(self, D, Nu, Nv, G=None):
        self.U, self.V = np.zeros((D, Nu)), np.zeros((D, Nv))
        self.mu = [np.zeros(D), np.zeros(D)]
        self.Lam = [5.0 * np.eye(D), 5.0 * np.eye(D)]
        g = np.full(D, 5.0) if G is None else np.broadcast_to(np.asarray(G, dtype=np.float64), (D,))
        self.GU, self.GV = np.tile(g[:, None], (1, Nu)), np.tile(g[:, None], (1, Nv))
        self.rU, self.rV = np.zeros((D, Nu)), np.zeros((D, Nv))


def leapfrog(st, Udata, Vdata, alpha, L, L_inner, eps, vectorised):
    """the trajectory of one iteration (:77-85); returns the momentum norms after each step and at the end (the reference prints
    these); st.norm0 keeps |r_U| after the opening update, which it does not print"""
    norms = []
    hmc_update_u(st.rU, st.U, st.V, Udata, st.Lam[0], st.mu[0], alpha, L_inner, eps / 2, vectorised)
    st.norm0 = np.linalg.norm(st.rU)
    for l in range(1, L + 1):
        hmc_update_u(st.rV, st.V, st.U, Vdata, st.Lam[1], st.mu[1], alpha, L_inner, eps, vectorised)
        if l < L:
            hmc_update_u(st.rU, st.U, st.V, Udata, st.Lam[0], st.mu[0], alpha, L_inner, eps, vectorised)
        norms.append((np.linalg.norm(st.rU), np.linalg.norm(st.rV)))
    hmc_update_u(st.rU, st.U, st.V, Udata, st.Lam[0], st.mu[0], alpha, L_inner, eps / 2, vectorised)
    norms.append((np.linalg.norm(st.rU), np.linalg.norm(st.rV)))
    return norms


def run(uid, vid, values, test_uid, test_vid, test_val, Nu, Nv, D, alpha, seed, burnin=100, psamples=100, L=10, L_inner=1,
        prior_freq=8, eps=0.01, clamp=(), vectorised=False, G=None, niter=None, phases=None):
    """macau_hmc's loop (:33-137).  niter (optional) stops early; phases (optional) maps an iteration number to the (eps, L) it
    starts with, as bdf_hmc_set_params sets them between two iterations.  Returns a dict: the final State "state", "eps", "L",
    "rmse", "rmse_avg" and per-iteration "records" (dicts of eps, L, kin_s, kin_f, pot_s, pot_f, dH, uniform, accepted, eps_new,
    L_new, |U|, |V|, rmse, rmse_avg, norms, norm0)."""
    uid, vid = np.asarray(uid, dtype=np.int64), np.asarray(vid, dtype=np.int64)
    test_uid, test_vid = np.asarray(test_uid, dtype=np.int64), np.asarray(test_vid, dtype=np.int64)
    test_val = np.asarray(test_val, dtype=np.float64)
    mean_value = np.mean(values)
    val = np.asarray(values, dtype=np.float64) - mean_value
    Udata = sparse_data(uid, vid, val, Nu, Nv)
    Vdata = Udata.T.tocsc()
    Vdata.sort_indices()
    st = State(D, Nu, Nv, G)
    kin = compute_kinetic_vec if vectorised else compute_kinetic
    pot = compute_potential_vec if vectorised else compute_potential
    yhat_post = np.zeros(len(test_val))
    rmse = rmse_post = float("nan")
    records = []
    total = burnin + psamples if niter is None else niter
    for i in range(1, total + 1):
        if phases and i in phases:
            eps, L = phases[i]
        rec = {"eps": eps, "L": L}
        st.rU = sample_momentum(st.GU, seed, i, 0)
        st.rV = sample_momentum(st.GV, seed, i, 1)
        kinetic_start = kin(st.rU, st.GU) + kin(st.rV, st.GV)
        potential_start = pot(uid, vid, val, alpha, st.U, st.V, st.mu, st.Lam)
        Ustart, Vstart = st.U.copy(), st.V.copy()
        rec["norms"] = leapfrog(st, Udata, Vdata, alpha, L, L_inner, eps, vectorised)
        rec["norm0"] = st.norm0
        kinetic_final = kin(st.rU, st.GU) + kin(st.rV, st.GV)
        potential_final = pot(uid, vid, val, alpha, st.U, st.V, st.mu, st.Lam)
        dH = potential_start - potential_final + kinetic_start - kinetic_final
        rec.update(kin_s=kinetic_start, kin_f=kinetic_final, pot_s=potential_start, pot_f=potential_final, dH=dH)
        rec["uniform"] = uniform(seed, i)
        accepted = (dH >= 0 or rec["uniform"] < math.exp(dH)) if not math.isnan(dH) else False     # rand() < 1 <= exp(dH)
        if not accepted:
            st.U[:], st.V[:] = Ustart, Vstart
            if dH < -6:
                eps, L = eps / 2, math.ceil(L * 1.6)
        rec.update(accepted=accepted, eps_new=eps, L_new=L)
        if i % prior_freq == 0:
            for e, S in enumerate((st.U, st.V)):
                D_ = S.shape[0]
                mu_N, beta_N, T_N, nu_N = O.hyper_params(S.T, np.zeros(D_), 2.0, np.eye(D_), float(D_))
                st.mu[e], st.Lam[e] = O.hyper_draw(mu_N, beta_N, T_N, nu_N, seed, i, e)
        if len(test_val):
            yhat_raw = np.einsum("kn,kn->n", st.U[:, test_uid - 1], st.V[:, test_vid - 1]) + mean_value
            yhat = clamp_(yhat_raw, clamp)
            update_yhat_post(yhat_post, yhat_raw, i, burnin)
            rmse = math.sqrt(np.mean((yhat - test_val) ** 2))
            rmse_post = math.sqrt(np.mean((clamp_(yhat_post.copy(), clamp) - test_val) ** 2))
        rec.update(normU=np.linalg.norm(st.U), normV=np.linalg.norm(st.V), rmse=rmse, rmse_avg=rmse_post)
        records.append(rec)
    return {"state": st, "eps": eps, "L": L, "rmse": rmse, "rmse_avg": rmse_post, "records": records,
            "mean_value": mean_value, "Udata": Udata, "Vdata": Vdata, "val": val}
