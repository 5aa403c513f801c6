"""Background cells (setBackground) restated in numpy: every cell of an N x M relation that is not listed
observes a background value with precision alpha c0.  Two ways to the same numbers -- the dense explicit sums over all N M cells, and
the fold the device takes (the other entity's Gram matrix into the prior, the listed cells with weight omega - c0 and a
pseudo-residual) -- and a small Gibbs sampler on top of the fold, for the test that the model learns from where the ones sit."""
import numpy as np


# ---- data ---------------------------------------------------------------------------------------------------------------------
def listing(N=37, M=29, density=0.2, seed=0, weights=False):
    """(ids 1-based (n, 2), y, omega) of about density N M listed cells, no cell twice; row 1 has no listed cell, row 2 every cell"""
    rng = np.random.default_rng(seed)
    on = rng.random((N, M)) < density
    on[0, :] = False
    on[1, :] = True
    i, j = np.nonzero(on)
    p = rng.permutation(len(i))
    i, j = i[p], j[p]
    y = np.round(rng.normal(1.0, 1.0, len(i)), 1)
    w = np.exp(rng.uniform(-0.5, 1.5, len(i))) if weights else np.ones(len(i))
    return np.stack([i + 1, j + 1], axis=1).astype(np.int64), y, w


def dense_listing(N, M, ids, y, w, c0, value):
    """the same data listed densely, row-major: every cell, omega_k and y_k on the listed ones, c0 and `value` on the rest"""
    Y, W = np.full((N, M), float(value)), np.full((N, M), float(c0))
    Y[ids[:, 0] - 1, ids[:, 1] - 1] = y
    W[ids[:, 0] - 1, ids[:, 1] - 1] = w
    ii, jj = np.meshgrid(np.arange(1, N + 1), np.arange(1, M + 1), indexing="ij")
    return np.stack([ii.ravel(), jj.ravel()], axis=1).astype(np.int64), Y.ravel(), W.ravel()


def all_cells_mean(N, M, y, value):
    """mean_value of a background relation: the mean over all N M cells"""
    return (np.sum(y) + (N * M - len(y)) * value) / (N * M)


def chain_case(weights, feat):
    """the relation of the chain tests: listing(weights), a background of weight 0.3 min omega at value -0.5 (rb != 0), 40 test
    cells anywhere in the matrix, and -- feat -- a dense 37 x 4 feature matrix of the first entity"""
    N, M = 37, 29
    ids, y, w = listing(N, M, weights=weights)
    rng = np.random.default_rng(11)
    cells = rng.choice(N * M, size=40, replace=False)
    test = np.stack([cells // M + 1, cells % M + 1], axis=1).astype(np.int64)
    F = rng.standard_normal((N, 4)) if feat else None
    return dict(N=N, M=M, ids=ids, y=y, w=w, c0=0.3 * float(w.min()), value=-0.5, test=test, test_y=rng.standard_normal(40), F=F)


# ---- the fold -----------------------------------------------------------------------------------------------------------------
def fold(Lam, mu, terms):
    """(Lambda_eff, mu_eff, alpha_rows): terms = [(alpha, c0, rb, V)] with V the other entity's (M, D) rows; mu (D,) or (N, D).
    Lambda_eff = Lambda + sum alpha c0 V'V added in the terms' order, mu_eff = Lambda_eff^-1 (Lambda mu + sum alpha c0 rb sum_j v_j)"""
    Le, t = Lam.copy(), np.zeros(Lam.shape[0])
    for alpha, c0, rb, V in terms:
        Le = Le + (alpha * c0) * (V.T @ V)
        t = t + (alpha * c0 * rb) * V.sum(axis=0)
    rhs = (mu @ Lam.T) + t                      # Lambda mu_i + t, row by row (Lambda symmetric)
    return Le, np.linalg.solve(Le, rhs.T).T, np.array([a * (1.0 - c) for a, c, _, _ in terms])


def unit_values(y, mean, c0, rb):
    """y' of a background relation with unit weights: what its rows read beside alpha (1 - c0)"""
    return mean + ((y - mean) - c0 * rb) / (1.0 - c0)


def weighted_terms(y, w, mean, c0, rb):
    """(obs_precision, linear_values) of a background relation with weights: omega - c0 and y - r', r' = (omega r - c0 rb) / (omega - c0)"""
    return w - c0, y - (w * (y - mean) - c0 * rb) / (w - c0)


def row_systems(N, ids, resid, prec, V, alpha, Lam, mu):
    """P_i = Lambda + alpha sum prec_k v v', b_i = Lambda mu_i + alpha sum prec_k resid_k v over the listed cells of row i"""
    D = Lam.shape[0]
    mu = np.broadcast_to(mu, (N, D))
    P, b = np.tile(Lam, (N, 1, 1)), mu @ Lam.T
    Vj = V[ids[:, 1] - 1]
    np.add.at(P, ids[:, 0] - 1, (alpha * np.asarray(prec))[:, None, None] * Vj[:, :, None] * Vj[:, None, :])
    np.add.at(b, ids[:, 0] - 1, (alpha * np.asarray(prec) * np.asarray(resid))[:, None] * Vj)
    return P, b


def systems_folded(N, ids, y, w, mean, c0, value, V, alpha, Lam, mu):
    """the row systems as the device forms them: the folded prior, weight omega - c0, pseudo-residual (omega r - c0 rb) / (omega - c0)"""
    rb = value - mean
    Le, me, _ = fold(Lam, mu, [(alpha, c0, rb, V)])
    return row_systems(N, ids, (w * (y - mean) - c0 * rb) / (w - c0), w - c0, V, alpha, Le, me)


def systems_dense(N, M, ids, y, w, mean, c0, value, V, alpha, Lam, mu):
    """... and as the explicit sums over all M cells of every row"""
    ida, ya, wa = dense_listing(N, M, ids, y, w, c0, value)
    return row_systems(N, ida, ya - mean, wa, V, alpha, Lam, mu)


# ---- alpha's sum of squares -----------------------------------------------------------------------------------------------------
def sse_folded(ids, y, w, mean, c0, value, U, V):
    rb = value - mean
    psi = np.sum(U[ids[:, 0] - 1] * V[ids[:, 1] - 1], axis=1)
    e = (y - mean) - psi
    listed = np.sum(w * e * e - c0 * (rb - psi) ** 2)
    N, M = len(U), len(V)
    return listed + c0 * ((N * M * rb * rb - 2.0 * rb * (U.sum(axis=0) @ V.sum(axis=0))) + np.sum((U.T @ U) * (V.T @ V)))


def sse_dense(ids, y, w, mean, c0, value, U, V):
    N, M = len(U), len(V)
    _, ya, wa = dense_listing(N, M, ids, y, w, c0, value)
    e = (ya - mean) - (U @ V.T).ravel()
    return np.sum(wa * e * e)


# ---- a Gibbs sampler on the fold: does the model learn from where the ones sit? ------------------------------------------------
def planted(seed, N=300, M=200, rank=4):
    """preferences p_ij = sigma(3 u.v - 1), u, v ~ N(0, I); a cell is listed (value 1) with probability p_ij.  Held out: a fifth
    of the ones and as many unlisted cells (value 0).  -> (train ids, test ids, test values), ids 1-based"""
    rng = np.random.default_rng(seed)
    U, V = rng.standard_normal((N, rank)), rng.standard_normal((M, rank))
    on = rng.random((N, M)) < 1.0 / (1.0 + np.exp(-(3.0 * (U @ V.T) - 1.0)))
    ones, zeros = np.argwhere(on), np.argwhere(~on)
    ones, zeros = ones[rng.permutation(len(ones))], zeros[rng.permutation(len(zeros))]
    nt = len(ones) // 5
    test = np.concatenate([ones[:nt], zeros[:nt]]) + 1
    return ones[nt:] + 1, test, np.concatenate([np.ones(nt), np.zeros(nt)])


def auc(labels, scores):
    """AUC_ROC(labels, scores) of src/ROC.jl:1-11"""
    y = np.asarray(labels, dtype=bool)[np.argsort(scores, kind="stable")]
    sx, sy = np.cumsum(y) / y.sum(), np.cumsum(~y) / (~y).sum()
    return float(np.sum((sx[1:] - sx[:-1]) * sy[1:]))


def _normal_wishart(S, rng, b0=2.0):
    """(mu, Lambda) | the rows S, hyper-prior mu0 = 0, b0, W = I, nu0 = D (src/sampling.jl:116-127)"""
    n, D = S.shape
    m, C = S.mean(axis=0), (S - S.mean(axis=0)).T @ (S - S.mean(axis=0))
    Tinv = np.eye(D) + C + (b0 * n / (b0 + n)) * np.outer(m, m)
    L = np.linalg.cholesky(np.linalg.inv(Tinv))
    A = np.tril(rng.standard_normal((D, D)), -1) + np.diag(np.sqrt(rng.chisquare(D + n - np.arange(D))))
    Lam = (L @ A) @ (L @ A).T
    return n * m / (b0 + n) + np.linalg.solve(np.linalg.cholesky((b0 + n) * Lam).T, rng.standard_normal(D)), Lam


def gibbs_auc(seed, c0, D=8, alpha=10.0, burnin=20, psamples=20, value=0.0):
    """held-out AUC of the planted data after burnin + psamples iterations: c0 > 0 with background cells, c0 = 0 on the listed cells alone"""
    ids, test, tv = planted(seed)
    N, M = 300, 200
    y = np.ones(len(ids))
    mean = all_cells_mean(N, M, y, value) if c0 > 0 else 1.0
    rb = value - mean
    resid = ((y - mean) - c0 * rb) / (1.0 - c0)
    rng = np.random.default_rng(1000 + seed)
    S = [np.zeros((N, D)), np.zeros((M, D))]
    mu, Lam = [np.zeros(D), np.zeros(D)], [5.0 * np.eye(D), 5.0 * np.eye(D)]
    avg = np.zeros(len(test))
    for it in range(burnin + psamples):
        for e in (0, 1):
            O, n = S[1 - e], (N, M)[e]
            Le, me = Lam[e], mu[e]
            if c0 > 0:
                Le, me, _ = fold(Lam[e], mu[e], [(alpha, c0, rb, O)])
            P, b = row_systems(n, ids[:, [e, 1 - e]], resid, np.full(len(ids), 1.0 - c0), O, alpha, Le, me)
            for i in range(n):
                Li = np.linalg.cholesky(P[i])
                S[e][i] = np.linalg.solve(P[i], b[i]) + np.linalg.solve(Li.T, rng.standard_normal(D))
            mu[e], Lam[e] = _normal_wishart(S[e], rng)
        if it >= burnin:
            avg += mean + np.sum(S[0][test[:, 0] - 1] * S[1][test[:, 1] - 1], axis=1)
    return auc(tv < 0.5, -avg / psamples)
