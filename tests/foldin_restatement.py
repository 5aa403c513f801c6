"""A numpy restatement of the fold-in of NEW rows from a few cells of their own (setNewObserved), line by line
from the formulas, for the fold-in tests.

Given one posterior draw (mu, Lambda, beta, V, alpha), a new row i with prior mean mu_i (mu + beta' f_i, or mu for an entity without
features) whose cells K_i are known has
  P_i = Lambda + alpha sum_{j in K_i} v_j v_j',   b_i = Lambda mu_i + alpha sum_{j in K_i} (y_ij - mean_value) v_j,   uhat_i = P_i^-1 b_i,
u* | draw, y* ~ N(uhat_i, P_i^-1), and it is integrated out of the cell (i, j):
  y | draw ~ N(m, q_ij + 1 / alpha),   m = mean_value + uhat_i . v_j,   q_ij = v_j' P_i^-1 v_j   (np.linalg.solve).
The new row's cells do not feed back into V: the standard fold-in.  The running state (`Stream`), the eight scalars (`scalars`) and
`quality` are those of newrows_restatement.py; `gibbs` is its sampler without features (plain BPMF) that folds the new rows in behind
every posterior draw, and the quality record at the end holds the five CPU chains' figures.
"""
import math

import numpy as np

import newrows_restatement as NR

Stream, scalars, quality, predict, loglik = NR.Stream, NR.scalars, NR.quality, NR.predict, NR.loglik


# ---- one draw ---------------------------------------------------------------------------------------------------------------------
def systems(Lambda, mu_rows, V, alpha, known_ids, known_y, mean_value):
    """(P, b) of every new row: P (n*, D, D), b (n*, D).  mu_rows (n*, D): the rows' prior means; known_ids (k, 2), 1-based: the new
    row, then the row of V"""
    Lambda, V, mu_rows = (np.asarray(a, dtype=np.float64) for a in (Lambda, V, mu_rows))
    n = len(mu_rows)
    P = np.repeat(Lambda[None, :, :], n, axis=0)
    b = mu_rows @ Lambda.T
    for (i, j), y in zip(np.asarray(known_ids).reshape(-1, 2) - 1, known_y):
        P[i] += alpha * np.outer(V[j], V[j])
        b[i] += alpha * (y - mean_value) * V[j]
    return P, b


def solve(P, b, ids, V, mean_value):
    """uhat (n*, D) and (m, q) per cell of ids (n, 2), 1-based, from the systems"""
    V = np.asarray(V, dtype=np.float64)
    uh = np.stack([np.linalg.solve(P[i], b[i]) for i in range(len(P))]) if len(P) else np.zeros_like(b)
    i, j = ids[:, 0] - 1, ids[:, 1] - 1
    m = mean_value + np.sum(uh[i] * V[j], axis=1)
    q = np.array([V[jj] @ np.linalg.solve(P[ii], V[jj]) for ii, jj in zip(i, j)]) if len(ids) else np.zeros(0)
    return uh, m, q


def cells(Lambda, mu_rows, V, alpha, known_ids, known_y, ids, mean_value):
    P, b = systems(Lambda, mu_rows, V, alpha, known_ids, known_y, mean_value)
    return solve(P, b, ids, V, mean_value)


# ---- planted data without features, and a split of the new rows' cells --------------------------------------------------------
def split_known(new, k, seed):
    """per new row, k of its cells chosen by a seeded shuffle are known, the rest are scored: ((known ids, y), (test ids, y))"""
    ids, y = new
    rng = np.random.default_rng(seed)
    known = np.zeros(len(y), dtype=bool)
    for i in np.unique(ids[:, 0]):
        at = np.nonzero(ids[:, 0] == i)[0]
        known[rng.permutation(at)[:k]] = True
    return (ids[known], y[known]), (ids[~known], y[~known])


# ---- BPMF without features, folding in behind every draw ----------------------------------------------------------------------
def gibbs(train, known, test, N, M, D, alpha, burnin, psamples, seed):
    """newrows_restatement.gibbs without features: the rows of both entities with their Normal-Wishart hyperpriors; behind every
    posterior draw the cells `test` of the new rows conditioned on their cells `known`.  Returns newrows_restatement.quality's
    record of the test cells"""
    rng = np.random.default_rng(seed)
    ids, y = train
    iu, iv = ids[:, 0] - 1, ids[:, 1] - 1
    mean = float(y.mean())
    r = y - mean
    U, V = np.zeros((N, D)), np.zeros((M, D))
    mu_u, Lam_u, mu_v, Lam_v = np.zeros(D), 5.0 * np.eye(D), np.zeros(D), 5.0 * np.eye(D)
    st = Stream()
    (kid, ky), (tid, ty) = known, test
    n_new = int(max(kid[:, 0].max() if len(kid) else 0, tid[:, 0].max() if len(tid) else 0))
    for it in range(1, burnin + psamples + 1):
        U = NR._rows(rng, iu, iv, r, V, alpha, np.tile(mu_u, (N, 1)), Lam_u, N)
        mu_u, Lam_u = NR._normal_wishart(rng, U, np.zeros(D), 2.0, np.eye(D), D)
        V = NR._rows(rng, iv, iu, r, U, alpha, np.tile(mu_v, (M, 1)), Lam_v, M)
        mu_v, Lam_v = NR._normal_wishart(rng, V, np.zeros(D), 2.0, np.eye(D), D)
        if it > burnin:
            _, m, q = cells(Lam_u, np.tile(mu_u, (n_new, 1)), V, alpha, kid, ky, tid, mean)
            st.update(predict(False, m, q), q, loglik(False, ty, m, q, alpha), 1 if it == burnin + 1 else 2)
    return quality(st.mean, st.stdev(False), ty, mean, alpha)


# ---- the quality record ----------------------------------------------------------------------------------
# newrows_restatement.QUALITY_SHAPE without its features: 300 + 100 rows, M = 60, D = 4, 40 % observed, noise sd 0.3, alpha = 1 / 0.09
# fixed, 50 + 100 iterations; 10 known cells per new row by split_known's shuffle (seed QUALITY_SPLIT_SEED), the rest scored
QUALITY_KNOWN = 10
QUALITY_SPLIT_SEED = 11


def quality_data(k=QUALITY_KNOWN):
    sh = dict(NR.QUALITY_SHAPE)
    _, _, train, new = NR.planted(**sh)
    known, test = split_known(new, k, QUALITY_SPLIT_SEED)
    return sh, train, known, test


# the five CPU chains' figures (gibbs on newrows_restatement.QUALITY_SEEDS): ratio = (fold-in RMSE) / (RMSE of predicting mean_value),
# coverage of pred +- 1.645 sqrt(stdev^2 + 1 / alpha); tests/test_foldin_host.py recomputes the first
QUALITY_CPU_RATIOS = (0.18300959, 0.18294673, 0.18280405, 0.18267953, 0.18330797)
QUALITY_CPU_COVERAGE = (0.90593343, 0.90448625, 0.90520984, 0.90593343, 0.90520984)
QUALITY_CPU_COLD_RATIO = 0.99071144        # chain seed 1 with no known cell, scored on the same cells: every row at the prior mean
