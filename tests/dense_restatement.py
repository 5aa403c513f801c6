"""A dense two-mode relation (setDense) restated in numpy: every one of its N x M cells is observed, so the
relation reaches row i's conditional through G = V'V, which all rows share, and through row i of C = R V.

`table` / `listing` give a dense matrix and its explicit listing; `systems_dense` states the row systems from (G, C) and
`systems_explicit` from the listed cells one by one; `sse_closed` and `sse_explicit` do the same for alpha's sum of squares;
`gibbs` is a whole chain on the (G, C) form with numpy's own generator (what the model learns, not the device's streams)."""
import math

import numpy as np


def table(N=37, M=29, seed=5, rank=3, noise=0.3):
    """an N x M matrix of planted rank with noise, none of its values repeated"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((N, rank)) @ rng.standard_normal((M, rank)).T + noise * rng.standard_normal((N, M)) + 0.7


def listing(Y):
    """every cell of Y as a table of 1-based ids and values, row by row"""
    N, M = Y.shape
    ii, jj = np.meshgrid(np.arange(1, N + 1), np.arange(1, M + 1), indexing="ij")
    return np.stack([ii.ravel(), jj.ravel()], axis=1).astype(np.int64), np.ascontiguousarray(Y, dtype=np.float64).ravel()


def systems_dense(Rs, Vs, alphas, Lam, mu):
    """the row systems of an entity with dense relations k = 0 ..: R_k (N x M_k, values without their mean), V_k the other entity's
    rows -> P (D x D, one for all rows) = Lambda + sum alpha_k G_k, b (N x D) = Lambda mu_i + sum alpha_k C_k,i"""
    N, D = Rs[0].shape[0], Lam.shape[0]
    P = Lam.copy()
    b = np.broadcast_to(mu, (N, D)) @ Lam.T
    for R, V, a in zip(Rs, Vs, alphas):
        P = P + a * (V.T @ V)
        b = b + a * (R @ V)
    return P, b


def systems_explicit(N, ids, r, V, alpha, Lam, mu, P=None, b=None):
    """the same from the listed cells one by one, as sample_user does (ids 1-based, mode 0 the entity's own); P, b: what to add to"""
    D = Lam.shape[0]
    if P is None:
        P = np.broadcast_to(Lam, (N, D, D)).copy()
        b = (np.broadcast_to(mu, (N, D)) @ Lam.T).copy()
    for (i, j), rv in zip(np.asarray(ids) - 1, r):
        P[i] += alpha * np.outer(V[j], V[j])
        b[i] += alpha * rv * V[j]
    return P, b


def sse_pieces(R, U, V):
    """(sum r^2, sum_i u_i.C_i, <U'U, V'V>) of the closed form"""
    return float(np.sum(R * R)), float(np.sum(U * (R @ V))), float(np.sum((U.T @ U) * (V.T @ V)))


def sse_closed(R, U, V):
    r2, uc, gg = sse_pieces(R, U, V)
    return (r2 - 2.0 * uc) + gg


def sse_explicit(R, U, V):
    """math.fsum over all cells"""
    E = R - U @ V.T
    return math.fsum((E * E).ravel().tolist())


def product_reference(R, F, transpose):
    """(R F or R' F, sum_c |r| |f|) per element by math.fsum"""
    A = R.T if transpose else R
    T, D = A.shape[0], F.shape[1]
    out, mag = np.zeros((T, D)), np.zeros((T, D))
    for t in range(T):
        for d in range(D):
            p = A[t] * F[:, d]
            out[t, d], mag[t, d] = math.fsum(p.tolist()), math.fsum(np.abs(p).tolist())
    return out, mag


def gibbs(Y, D, alpha, iters, seed, sample_alpha=False):
    """a whole BPMF chain on a dense Y with the row systems from (G, C): -> (U, V, mean, alpha trace).  The Normal-Wishart
    hyperprior of macau() (mu0 = 0, b0 = 2, W0 = I, nu0 = D); numpy's generator."""
    rng = np.random.default_rng(seed)
    N, M = Y.shape
    mean = float(Y.mean())
    R = Y - mean
    fac = [np.zeros((N, D)), np.zeros((M, D))]
    mu, Lam = [np.zeros(D), np.zeros(D)], [5.0 * np.eye(D), 5.0 * np.eye(D)]
    trace = []
    for _ in range(iters):
        if sample_alpha:
            sse = sse_closed(R, fac[0], fac[1])
            alpha = rng.gamma((2.0 + N * M) / 2.0, 2.0 / (2.0 + sse))        # nu0 = 2, lambda0 = 1 (sample_alpha)
        trace.append(alpha)
        for k in (0, 1):
            Rk, other = (R if k == 0 else R.T), fac[1 - k]
            P, b = systems_dense([Rk], [other], [alpha], Lam[k], mu[k])
            L = np.linalg.cholesky(P)
            z = rng.standard_normal(b.shape)
            fac[k] = np.linalg.solve(P, b.T).T + np.linalg.solve(L.T, z.T).T
            n, S = fac[k].shape[0], fac[k]
            ubar = S.mean(axis=0)
            Sc = (S - ubar).T @ (S - ubar)
            b0, nu0 = 2.0, float(D)
            Winv = np.eye(D) + Sc + (b0 * n / (b0 + n)) * np.outer(ubar, ubar)
            W = np.linalg.inv(Winv)
            W = (W + W.T) / 2
            A = rng.standard_normal((int(nu0 + n), D)) @ np.linalg.cholesky(W).T
            Lam[k] = A.T @ A
            mu[k] = (n * ubar) / (b0 + n) + np.linalg.solve(np.linalg.cholesky((b0 + n) * Lam[k]).T, rng.standard_normal(D))
    return fac[0], fac[1], mean, np.array(trace)


# ---- the holes ------------------------------------------------------------------------------------------------------------------
P_DENSE = 24


def hole_normals(seed, sweep, rel_tag, n):
    """the normal of every hole 0 .. n-1 from the library's streams: normal 0 of (P_DENSE, 0x800000 | rel_tag, row = the hole's index)"""
    from oracle import oracle as O
    return np.array([O.normals(seed, sweep, P_DENSE, 0x800000 | int(rel_tag), k, 1)[0] for k in range(n)], dtype=np.float64).reshape(n)


def impute(R, holes, U, V, alpha, z):
    """the imputing map: R[i, j] = u_i.v_j + z / sqrt(alpha) at the holes (0-based (n, 2)), everything else untouched"""
    out = R.copy()
    if len(holes):
        i, j = holes[:, 0], holes[:, 1]
        out[i, j] = np.sum(U[i] * V[j], axis=1) + np.asarray(z) / np.sqrt(alpha)
    return out


def run_chain(Y, D, seed, iters, alpha=1.0, alpha_sample=False, rel_tag=1, test_ids=None, burnin=0, alpha_lambda0=1.0, alpha_nu0=2.0):
    """macau() on ONE dense relation (Y: N x M, NaN at the holes) from the oracle's row sampler, hyperprior and sample_alpha on the
    explicit listing, in the library's order: holes | U, V, previous alpha -> alpha | U, V, all cells -> rows and hyperprior of either
    entity in turn.  Returns {"S", "alpha", "trace", "mean", "R"} after the last iteration and, with test_ids (1-based), "pred": the
    mean over iterations burnin + 1 .. iters of u.v + mean on those cells."""
    from oracle import oracle as O
    N, M = Y.shape
    listed = ~np.isnan(Y)
    v = Y[listed]                                           # row by row, as the relation lists them
    mean = float(np.cumsum(v)[-1]) / len(v)
    R = np.where(listed, Y - mean, 0.0)
    holes = np.argwhere(~listed)
    ids_all, _ = listing(Y)
    index = O.index_build(ids_all, [N, M])
    S = [np.zeros((N, D)), np.zeros((M, D))]
    mu, Lam = [np.zeros(D), np.zeros(D)], [5.0 * np.eye(D), 5.0 * np.eye(D)]
    alpha, trace, pred = float(alpha), [], None
    for it in range(1, iters + 1):
        if len(holes):
            R = impute(R, holes, S[0], S[1], alpha, hole_normals(seed, it, rel_tag, len(holes)))
        if alpha_sample:
            alpha = O.sample_alpha(alpha_lambda0, alpha_nu0, N * M, sse_explicit(R, S[0], S[1]), seed, it, rel_tag)
        trace.append(alpha)
        for j in (0, 1):
            term = O.Term(ids_all, (R + mean).ravel(), [N, M], j, alpha, mean, [None if k == j else S[k] for k in (0, 1)], index=index)
            S[j] = O.sample_rows(D, (N, M)[j], [term], mu[j], Lam[j], seed, it, j + 1)
            mu_N, beta_N, T_N, nu_N = O.hyper_params(S[j], np.zeros(D), 2.0, np.eye(D), float(D))
            mu[j], Lam[j] = O.hyper_draw(mu_N, beta_N, T_N, nu_N, seed, it, j + 1)
        if test_ids is not None and it > burnin:
            p = np.sum(S[0][test_ids[:, 0] - 1] * S[1][test_ids[:, 1] - 1], axis=1) + mean
            pred = p if pred is None else pred + p
    out = {"S": S, "alpha": alpha, "trace": np.array(trace), "mean": mean, "R": R}
    if pred is not None:
        out["pred"] = pred / (iters - burnin)
    return out


def planted(seed=0, N=150, M=40, rank=4, noise=0.3, held=0.2):
    """planted rank-4 data: Y = U V' + noise (sd 0.3); a fifth of the cells held out -> (Y, the held-out cells' 1-based listing rows)"""
    rng = np.random.default_rng(seed)
    Y = rng.standard_normal((N, rank)) @ rng.standard_normal((M, rank)).T + noise * rng.standard_normal((N, M))
    out = np.sort(rng.choice(N * M, size=int(held * N * M), replace=False)) + 1
    return Y, out


def gibbs_holes_rmse(Y, held, D, alpha, iters, burnin, seed):
    """the held-out RMSE of `gibbs`-style chains on Y whose cells `held` (1-based listing rows) are holes: the dense chain with
    imputation (numpy's generator) -> RMSE of the posterior mean prediction on the holes"""
    rng = np.random.default_rng(seed)
    N, M = Y.shape
    hi, hj = (held - 1) // M, (held - 1) % M
    listed = np.ones((N, M), dtype=bool)
    listed[hi, hj] = False
    mean = float(Y[listed].mean())
    R = np.where(listed, Y - mean, 0.0)
    fac = [np.zeros((N, D)), np.zeros((M, D))]
    mu, Lam = [np.zeros(D), np.zeros(D)], [5.0 * np.eye(D), 5.0 * np.eye(D)]
    pred, n = np.zeros(len(held)), 0
    for it in range(iters):
        R[hi, hj] = np.sum(fac[0][hi] * fac[1][hj], axis=1) + rng.standard_normal(len(held)) / np.sqrt(alpha)
        for k in (0, 1):
            P, b = systems_dense([R if k == 0 else R.T], [fac[1 - k]], [alpha], Lam[k], mu[k])
            L = np.linalg.cholesky(P)
            fac[k] = np.linalg.solve(P, b.T).T + np.linalg.solve(L.T, rng.standard_normal(b.shape).T).T
            S, nn = fac[k], fac[k].shape[0]
            ubar = S.mean(axis=0)
            Winv = np.eye(D) + (S - ubar).T @ (S - ubar) + (2.0 * nn / (2.0 + nn)) * np.outer(ubar, ubar)
            W = np.linalg.inv(Winv)
            A = rng.standard_normal((int(D + nn), D)) @ np.linalg.cholesky((W + W.T) / 2).T
            Lam[k] = A.T @ A
            mu[k] = (nn * ubar) / (2.0 + nn) + np.linalg.solve(np.linalg.cholesky((2.0 + nn) * Lam[k]).T, rng.standard_normal(D))
        if it >= burnin:
            pred += np.sum(fac[0][hi] * fac[1][hj], axis=1) + mean
            n += 1
    return float(np.sqrt(np.mean((pred / n - Y[hi, hj]) ** 2)))
