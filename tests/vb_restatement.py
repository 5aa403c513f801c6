"""A numpy restatement of src/macau_vb.jl (bpmf_vb, update_u!, update_prior!, predict), line by line, for the VB tests.

`run(...)` follows the reference's loop (one row at a time, np.linalg.inv -- LU, as Julia's inv); `vectorised=True` computes
the same update for all rows at once (a scipy CSR product against Euu reshaped N x D^2, then a batched inv), for full-size
data.  Both start from given initial models, which they copy.
"""
import copy

import numpy as np
import scipy.sparse as sp


class Model:
    """the fields of VBModel (macau_vb.jl:5-18)"""

    def __init__(self, m):
        for f in ("mu_u", "Euu", "nu_N", "W_N", "mu_N", "b_N", "Winv_0", "mu_0", "b_0"):
            setattr(self, f, copy.deepcopy(np.asarray(getattr(m, f)) if isinstance(getattr(m, f), np.ndarray) else getattr(m, f)))
        self.mu_u = np.array(self.mu_u, dtype=np.float64)
        self.Euu = np.array(self.Euu, dtype=np.float64)


def clamp_(x, clamp):
    """clamp! (src/sampling.jl:108-114)"""
    if len(clamp):
        x[x < clamp[0]] = clamp[0]
        x[x > clamp[1]] = clamp[1]
    return x


def predict(Um, Vm, mean_value, uids, vids):
    """macau_vb.jl:142-148 (ids 1-based)"""
    yhat = np.zeros(len(uids)) + mean_value
    for i in range(len(uids)):
        yhat[i] += np.dot(Um.mu_u[:, uids[i] - 1], Vm.mu_u[:, vids[i] - 1])
    return yhat


def predict_vec(Um, Vm, mean_value, uids, vids):
    return mean_value + np.einsum("dn,dn->n", Um.mu_u[:, uids - 1], Vm.mu_u[:, vids - 1])


def update_u(Um, Vm, Udata, alpha):
    """update_u! (macau_vb.jl:103-130); Udata: scipy CSC, N_other x N (column uu: the neighbours of row uu)"""
    A = Um.W_N * Um.nu_N
    b = Um.W_N * Um.nu_N @ Um.mu_N
    colptr, rowval, nzval = Udata.indptr, Udata.indices, Udata.data
    for uu in range(Um.mu_u.shape[1]):
        idx = slice(colptr[uu], colptr[uu + 1])
        ff = rowval[idx]
        rr = nzval[idx]
        L = A.copy()
        for vv in ff:
            L += alpha * Vm.Euu[:, :, vv]
        Linv = np.linalg.inv(L)
        MM = Vm.mu_u[:, ff]
        mu = Linv @ (b + alpha * MM @ rr)
        Um.mu_u[:, uu] = mu
        Um.Euu[:, :, uu] = Linv + np.outer(mu, mu)


def update_u_vec(Um, Vm, Udata, alpha):
    """update_u! for all rows at once"""
    D, N = Um.mu_u.shape
    A = Um.W_N * Um.nu_N
    b = A @ Um.mu_N
    R = Udata.T.tocsr()                                         # N x N_other, the centred values
    P = R.copy()
    P.data = np.ones_like(P.data)                               # the pattern
    S = P @ Vm.Euu.reshape(D * D, -1).T                         # N x D^2: sum of the neighbours' Euu
    L = A[None, :, :] + alpha * np.asarray(S).reshape(N, D, D)
    Linv = np.linalg.inv(L)
    rhs = b[None, :] + alpha * np.asarray(R @ Vm.mu_u.T)
    mu = np.einsum("nij,nj->ni", Linv, rhs)
    Um.mu_u = np.ascontiguousarray(mu.T)
    Um.Euu = np.ascontiguousarray((Linv + mu[:, :, None] * mu[:, None, :]).transpose(1, 2, 0))


def update_prior(m):
    """update_prior! (macau_vb.jl:132-140)"""
    m.mu_N = (m.b_0 * m.mu_0 + m.mu_u.sum(axis=1)) / m.b_N
    m.W_N = np.linalg.inv(m.Winv_0 + m.Euu.sum(axis=2) + m.b_0 * np.outer(m.mu_0, m.mu_0) - m.b_N * np.outer(m.mu_N, m.mu_N))


def sparse_data(uid, vid, val, Nu, Nv):
    """Udata = sparse(vid, uid, val, N_v, N_u): duplicates summed into one entry, rows sorted in every column"""
    U = sp.coo_matrix((val, (vid - 1, uid - 1)), shape=(Nv, Nu)).tocsc()
    U.sum_duplicates()
    U.sort_indices()
    return U


def run(U0, V0, uid, vid, values, test_uid, test_vid, test_val, alpha, niter, clamp=(), vectorised=False, log=None):
    """bpmf_vb's loop (macau_vb.jl:46-90) from the initial models U0, V0.  Returns (Umodel, Vmodel, rmse, rmse_train); log,
    if a list, gets (|U|, |V|, rmse, rmse_train) of every iteration."""
    Um, Vm = Model(U0), Model(V0)
    uid, vid = np.asarray(uid, dtype=np.int64), np.asarray(vid, dtype=np.int64)
    test_uid, test_vid = np.asarray(test_uid, dtype=np.int64), np.asarray(test_vid, dtype=np.int64)
    mean_value = np.mean(values)
    val = np.asarray(values, dtype=np.float64) - mean_value
    Udata = sparse_data(uid, vid, val, Um.mu_u.shape[1], Vm.mu_u.shape[1])
    Vdata = Udata.T.tocsc()
    Vdata.sort_indices()
    upd, pred = (update_u_vec, predict_vec) if vectorised else (update_u, predict)
    rmse = rmse_train = float("nan")
    for _ in range(niter):
        upd(Um, Vm, Udata, alpha)
        upd(Vm, Um, Vdata, alpha)
        update_prior(Um)
        update_prior(Vm)
        yhat = clamp_(pred(Um, Vm, mean_value, test_uid, test_vid), clamp)
        rmse = np.sqrt(np.mean((yhat - test_val) ** 2)) if len(test_val) else float("nan")
        yhat_train = clamp_(pred(Um, Vm, mean_value, uid, vid), clamp)
        rmse_train = np.sqrt(np.mean((yhat_train - mean_value - val) ** 2))
        if log is not None:
            log.append((np.linalg.norm(Um.mu_u), np.linalg.norm(Vm.mu_u), rmse, rmse_train))
    return Um, Vm, rmse, rmse_train


def make_case(Nu, Nv, nnz, seed, ntest=200, empty=3, dups=20):
    """ratings from a planted rank-3 model: the last `empty` rows of both entities have no training rows (some test rows do),
    and `dups` (u, v) pairs appear twice.  Returns (uid, vid, values, test_uid, test_vid, test_values), ids 1-based."""
    rng = np.random.default_rng(seed)
    Pu, Pv = rng.standard_normal((Nu, 3)), rng.standard_normal((Nv, 3))
    uid = rng.integers(1, Nu - empty + 1, nnz)
    vid = rng.integers(1, Nv - empty + 1, nnz)
    k = rng.choice(nnz, size=min(dups, nnz), replace=False)
    uid, vid = np.concatenate([uid, uid[k]]), np.concatenate([vid, vid[k]])
    vals = np.clip(3.0 + np.sum(Pu[uid - 1] * Pv[vid - 1], axis=1) + 0.3 * rng.standard_normal(len(uid)), 1.0, 5.0)
    tu, tv = rng.integers(1, Nu + 1, ntest), rng.integers(1, Nv + 1, ntest)
    tval = np.clip(3.0 + np.sum(Pu[tu - 1] * Pv[tv - 1], axis=1) + 0.3 * rng.standard_normal(ntest), 1.0, 5.0)
    return uid, vid, vals, tu, tv, tval


def relation_data(B, case, Nu, Nv, alpha=2.0):
    """a RelationData of one users x items relation holding `case` (make_case) as training and test rows"""
    uid, vid, vals, tu, tv, tval = case
    ids = np.concatenate([np.stack([uid, vid], 1), np.stack([tu, tv], 1)])
    y = np.concatenate([vals, tval])
    rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "r", [B.Entity("u"), B.Entity("v")], dims=[Nu, Nv])
    B.assignToTest(rel, np.arange(len(vals) + 1, len(y) + 1))
    B.setPrecision(rel, alpha)
    return B.RelationData(rel)
