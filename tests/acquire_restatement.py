"""Acquisition lists from the moments of u.v over the posterior draws (setAcquire) restated in numpy: a draw's
product in the accumulate kernel's order (from zero, d in ascending blocks of four, as recommend_restatement.score_sum adds them),
the Welford fold of the products in push order, the sum of the draws' exceedance probabilities, the score of every cell by one
expression (csrc/acquire.h: bdf_acq_score) and the lists by recommend_restatement.topk.  What the GPU tests compare the device
with; tests/test_acquire_host.py checks it against np.mean / np.var in extended precision and against the header on the host."""
import math

import numpy as np

import recommend_restatement as RR

RULES = ("ucb", "sd", "prob_above")
_erfc = np.vectorize(math.erfc, otypes=[np.float64])


def product(U, V, rows0=None):
    """(p, mag) of one draw: p[i, j] = u_i . v_j from zero, d in ascending blocks of four; mag[i, j] = sum_d |u_id v_jd|, the
    scale of p's rounding error.  rows0: 0-based rows of U that are scored (None: all)"""
    Us = U if rows0 is None else U[np.asarray(rows0)]
    p, mag = np.zeros((Us.shape[0], V.shape[0])), np.zeros((Us.shape[0], V.shape[0]))
    for d0 in range(0, U.shape[1], 4):
        p = p + Us[:, d0:d0 + 4] @ V[:, d0:d0 + 4].T
        mag = mag + np.abs(Us[:, d0:d0 + 4]) @ np.abs(V[:, d0:d0 + 4]).T
    return p, mag


def phi(x):
    """the standard normal CDF as csrc/probit.h has it: erfc(-x / sqrt 2) / 2"""
    return 0.5 * _erfc(-np.asarray(x, dtype=np.float64) / 1.4142135623730951)


def fold_one(p, n, mean, M2):
    """one draw's products into the moments, n the count of draws with this one: bdf_acq_fold"""
    delta = p - mean
    mean = mean + delta / np.float64(n)
    return mean, M2 + delta * (p - mean)


def prob_term(p, alpha, mean_value, threshold):
    """Phi(sqrt(alpha) (p + mean_value - threshold)): bdf_acq_prob"""
    with np.errstate(over="ignore"):
        return phi(np.sqrt(np.float64(alpha)) * (p + np.float64(mean_value) - np.float64(threshold)))


def fold(draws, rows0=None, alphas=None, mean_value=0.0, threshold=None):
    """the planes {"mean", "M2"[, "psum"]} after the draws [(U, V), ...] in push order, and the largest per-draw sum_d |u_d v_d|
    of every cell; alphas: the draws' precisions (with a threshold)"""
    mean = M2 = psum = mag = None
    for b, (U, V) in enumerate(draws):
        p, m = product(U, V, rows0)
        if mean is None:
            mean, M2, psum, mag = np.zeros_like(p), np.zeros_like(p), np.zeros_like(p), np.zeros_like(p)
        mean, M2 = fold_one(p, b + 1, mean, M2)
        mag = np.maximum(mag, m)
        if threshold is not None:
            psum = psum + prob_term(p, alphas[b], mean_value, threshold)
    planes = {"mean": mean, "M2": M2}
    if threshold is not None:
        planes["psum"] = psum
    return planes, mag


def sd_of(M2, n):
    """the sample standard deviation over n draws, NaN with fewer than two: bdf_acq_sd"""
    M2 = np.asarray(M2, dtype=np.float64)
    if not n >= 2:
        return np.full(M2.shape, np.nan)
    return np.sqrt(M2 / (np.float64(n) - 1.0))


def scores_of(planes, n, rule, kappa=0.0, mean_value=0.0):
    """the acquisition score of every cell, in exactly bdf_acq_score's expression: kappa sd is rounded, then m is added"""
    if rule == "prob_above":
        psum = np.asarray(planes["psum"], dtype=np.float64)
        return psum / np.float64(n) if n >= 1 else np.full(psum.shape, np.nan)
    sd = sd_of(planes["M2"], n)
    if rule == "sd":
        return sd
    m = np.asarray(planes["mean"], dtype=np.float64) + np.float64(mean_value)
    spread = np.float64(kappa) * sd
    return spread + m


def topk(scores, K, listed=None):
    return RR.topk(scores, K, listed)


def gathered(planes, n, items, mean_value=0.0):
    """{"mean", "sd"[, "prob"]} at the lists' items (n_rows x K, 1-based, 0 padding: NaN there)"""
    on = items > 0
    cols = np.where(on, items - 1, 0)
    rows = np.arange(items.shape[0])[:, None]

    def at(a):
        return np.where(on, a[rows, cols], np.nan)
    out = {"mean": at(np.asarray(planes["mean"]) + np.float64(mean_value)), "sd": at(sd_of(planes["M2"], n))}
    if "psum" in planes:
        out["prob"] = at(scores_of(planes, n, "prob_above"))
    return out


# ---- is an unlisted cell of a row with few listed cells less certain? a numpy Gibbs sampler on planted Gaussian data --------------
SPREAD = dict(N=40, M=60, rank=3, sparse=2, full=40, D=4, alpha=5.0, burnin=20, psamples=30)


def planted_spread(seed):
    """(ids 1-based (n, 2), y): y = u.v + 0.3 noise, u, v ~ N(0, I) of rank 3, on a 40 x 60 relation whose first 20 rows list 2 cells
    each and whose last 20 rows list 40 cells each"""
    s = SPREAD
    rng = np.random.default_rng(500 + seed)
    U, V = rng.standard_normal((s["N"], s["rank"])), rng.standard_normal((s["M"], s["rank"]))
    cells = []
    for i in range(s["N"]):
        for j in rng.permutation(s["M"])[:s["sparse"] if i < s["N"] // 2 else s["full"]]:
            cells.append((i + 1, int(j) + 1))
    ids = np.array([cells[q] for q in rng.permutation(len(cells))], dtype=np.int64)
    y = np.sum(U[ids[:, 0] - 1] * V[ids[:, 1] - 1], axis=1) + 0.3 * rng.standard_normal(len(ids))
    return ids, y


def unlisted_medians(sd, ids):
    """(the median sd over the unlisted cells of the sparse rows, of the full rows)"""
    N = SPREAD["N"]
    off = np.ones(sd.shape, dtype=bool)
    off[ids[:, 0] - 1, ids[:, 1] - 1] = False
    return float(np.median(sd[:N // 2][off[:N // 2]])), float(np.median(sd[N // 2:][off[N // 2:]]))


def cpu_spread(seed):
    """the medians of unlisted_medians from a numpy BPMF chain on planted_spread(seed), the sd by the Welford fold"""
    import background_restatement as BR
    s = SPREAD
    ids, y = planted_spread(seed)
    N, M, D, alpha = s["N"], s["M"], s["D"], s["alpha"]
    mean_value = float(np.mean(y))
    rng = np.random.default_rng(900 + seed)
    S = [np.zeros((N, D)), np.zeros((M, D))]
    mu, Lam = [np.zeros(D), np.zeros(D)], [5.0 * np.eye(D), 5.0 * np.eye(D)]
    draws = []
    for it in range(s["burnin"] + s["psamples"]):
        for e in (0, 1):
            n = (N, M)[e]
            P, b = BR.row_systems(n, ids[:, [e, 1 - e]], y - mean_value, np.ones(len(ids)), S[1 - e], alpha, Lam[e], mu[e])
            for i in range(n):
                Li = np.linalg.cholesky(P[i])
                S[e][i] = np.linalg.solve(P[i], b[i]) + np.linalg.solve(Li.T, rng.standard_normal(D))
            mu[e], Lam[e] = BR._normal_wishart(S[e], rng)
        if it >= s["burnin"]:
            draws.append((S[0].copy(), S[1].copy()))
    planes, _ = fold(draws)
    return unlisted_medians(sd_of(planes["M2"], len(draws)), ids)
