"""Top-K lists from the posterior mean score (setRecommend) restated in numpy: the sum of u.v over the draws
in the accumulate kernel's order, the lists by np.lexsort on (item id, -score) with the listed cells removed, and recall@K, NDCG@K
and the hit rate with math.fsum.  What the GPU tests compare the device with; tests/test_recommend_host.py checks it against a
brute-force loop."""
import math

import numpy as np


def score_sum(draws, rows0=None):
    """sum[i, j] = sum over the draws (U, V) of u_i . v_j, in the kernel's order: the draws in push order, d in ascending blocks of
    four, every block added to the running sum.  Also the sum of |terms| per cell, the scale of its rounding error.
    rows0: 0-based rows of U that are scored (None: all)"""
    U0, V0 = draws[0]
    n = U0.shape[0] if rows0 is None else len(rows0)
    acc, mag = np.zeros((n, V0.shape[0])), np.zeros((n, V0.shape[0]))
    for U, V in draws:
        Us = U if rows0 is None else U[np.asarray(rows0)]
        for d0 in range(0, U.shape[1], 4):
            acc = acc + Us[:, d0:d0 + 4] @ V[:, d0:d0 + 4].T
            mag = mag + np.abs(Us[:, d0:d0 + 4]) @ np.abs(V[:, d0:d0 + 4]).T
    return acc, mag


def scores_of(total, draws, mean_value):
    """the score of every cell: sum / draws + mean_value, in exactly that expression (bdf_rec_score)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.asarray(total, dtype=np.float64) / np.float64(draws) + np.float64(mean_value)


def topk(scores, K, listed=None):
    """per row the K best columns: falling score, equal scores by rising column; listed: per row the 0-based columns that never
    appear (None: none).  A score that is NaN is no candidate.  items int32 (n, K), 1-based, 0 behind the last candidate; the
    scores there NaN"""
    n, M = scores.shape
    items, out = np.zeros((n, K), dtype=np.int32), np.full((n, K), np.nan)
    for i in range(n):
        keep = ~np.isnan(scores[i])
        if listed is not None and len(listed[i]):
            keep[np.asarray(sorted(listed[i]), dtype=np.int64)] = False
        cols = np.nonzero(keep)[0]
        order = cols[np.lexsort((cols, -scores[i, cols]))][:K]
        items[i, :len(order)] = order + 1
        out[i, :len(order)] = scores[i, order]
    return items, out


def discount(r):
    return 1.0 / math.log2(r + 1)


def metrics(items, relevant):
    """(recall@K, NDCG@K, hit rate, rows scored) of the lists `items` (n, K; 1-based, 0 padding); relevant: per row the set of
    1-based relevant items.  Rows without a relevant item are left out; means over the rest, by math.fsum"""
    K = items.shape[1]
    rec, ndcg, hit = [], [], []
    for i in range(items.shape[0]):
        R = set(int(x) for x in relevant[i])
        if not R:
            continue
        flags = [int(it) != 0 and int(it) in R for it in items[i]]
        hits = sum(flags)
        rec.append(hits / len(R))
        dcg = math.fsum(discount(p + 1) for p in range(K) if flags[p])
        ndcg.append(dcg / math.fsum(discount(p) for p in range(1, min(K, len(R)) + 1)))
        hit.append(1.0 if hits else 0.0)
    n = len(rec)
    if n == 0:
        return float("nan"), float("nan"), float("nan"), 0
    return math.fsum(rec) / n, math.fsum(ndcg) / n, math.fsum(hit) / n, n


def listed_of(ids, n_rows, rows0=None):
    """per scored row the set of 0-based columns among the training ids (n, 2; 1-based); rows0: the 0-based ids of the scored rows"""
    by = [set() for _ in range(int(np.max(ids[:, 0])) if len(ids) else 0)]
    for i, j in np.asarray(ids, dtype=np.int64):
        by[i - 1].add(int(j - 1))
    pick = range(n_rows) if rows0 is None else rows0
    return [by[i] if i < len(by) else set() for i in pick]


def relevant_of(test_ids, test_values, class_cut, n_rows, rows0=None):
    """per scored row the set of 1-based items of its test cells with value > class_cut"""
    by = {}
    for (i, j), v in zip(np.asarray(test_ids, dtype=np.int64), test_values):
        if v > class_cut:
            by.setdefault(int(i - 1), set()).add(int(j))
    pick = range(n_rows) if rows0 is None else rows0
    return [by.get(int(i), set()) for i in pick]


def popularity_scores(ids, n_rows, M):
    """every row scores item j by the number of training cells that list it: the popularity ranking"""
    return np.tile(np.bincount(np.asarray(ids[:, 1], dtype=np.int64) - 1, minlength=M).astype(np.float64), (n_rows, 1))


# ---- the brute-force loops the restatement is checked against ---------------------------------------------------------------------
def brute_topk(scores, K, listed):
    n, M = scores.shape
    items, out = np.zeros((n, K), dtype=np.int32), np.full((n, K), np.nan)
    for i in range(n):
        taken = set()
        for p in range(K):
            best = None
            for j in range(M):
                if j in taken or j in listed[i] or scores[i, j] != scores[i, j]:
                    continue
                if best is None or scores[i, j] > scores[i, best]:        # (the first of equal scores stays: the smaller column)
                    best = j
            if best is None:
                break
            taken.add(best)
            items[i, p], out[i, p] = best + 1, scores[i, best]
    return items, out


def brute_metrics(items, relevant):
    n_scored, rec, nd, hr = 0, 0.0, 0.0, 0.0
    K = items.shape[1]
    for i in range(items.shape[0]):
        if len(relevant[i]) == 0:
            continue
        n_scored += 1
        hits, dcg, idcg = 0, 0.0, 0.0
        for p in range(K):
            if items[i, p] != 0 and int(items[i, p]) in relevant[i]:
                hits += 1
                dcg += 1.0 / math.log2(p + 2)
        for p in range(min(K, len(relevant[i]))):
            idcg += 1.0 / math.log2(p + 2)
        rec += hits / len(relevant[i])
        nd += dcg / idcg
        hr += 1.0 if hits else 0.0
    if n_scored == 0:
        return float("nan"), float("nan"), float("nan"), 0
    return rec / n_scored, nd / n_scored, hr / n_scored, n_scored


# ---- does the background model rank? the numpy sampler of tests/background_restatement.py with a score sum over every cell --------
def planted_ranking(seed, K=10, c0=0.1, D=8, alpha=10.0, burnin=20, psamples=20, value=0.0):
    """the planted implicit data of DESIGN.md section 20 (BR.planted): ((recall@K, NDCG@K) of the background model's lists from
    the CPU sampler, (recall@K, NDCG@K) of the popularity ranking), both with the training cells left out, on the held-out ones"""
    import background_restatement as BR
    ids, test, tv = BR.planted(seed)
    N, M = 300, 200
    y = np.ones(len(ids))
    mean = BR.all_cells_mean(N, M, y, value)
    rb = value - mean
    resid = ((y - mean) - c0 * rb) / (1.0 - c0)
    rng = np.random.default_rng(1000 + seed)
    S = [np.zeros((N, D)), np.zeros((M, D))]
    mu, Lam = [np.zeros(D), np.zeros(D)], [5.0 * np.eye(D), 5.0 * np.eye(D)]
    draws = []
    for it in range(burnin + psamples):
        for e in (0, 1):
            O, n = S[1 - e], (N, M)[e]
            Le, me, _ = BR.fold(Lam[e], mu[e], [(alpha, c0, rb, O)])
            P, b = BR.row_systems(n, ids[:, [e, 1 - e]], resid, np.full(len(ids), 1.0 - c0), O, alpha, Le, me)
            for i in range(n):
                Li = np.linalg.cholesky(P[i])
                S[e][i] = np.linalg.solve(P[i], b[i]) + np.linalg.solve(Li.T, rng.standard_normal(D))
            mu[e], Lam[e] = BR._normal_wishart(S[e], rng)
        if it >= burnin:
            draws.append((S[0].copy(), S[1].copy()))
    total, _ = score_sum(draws)
    listed, relevant = listed_of(ids, N), relevant_of(test, tv, 0.5, N)
    model = metrics(topk(scores_of(total, psamples, mean), K, listed)[0], relevant)
    pop = metrics(topk(popularity_scores(ids, N, M), K, listed)[0], relevant)
    return (model[0], model[1]), (pop[0], pop[1])
