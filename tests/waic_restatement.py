"""A numpy restatement of WAIC on the training cells for the waic tests.

`Stream` is the running state of bdf_pairs_waic_update as the kernel writes it -- the (M, A) recurrence of lpd_restatement.Stream and
Welford's (mean, M2) of the log-likelihood, with the phases and the draw counter --, `train_bounds` the table that says what kind of
record a training row is, `summary` the end-of-run quantities of bdf_pairs_waic and of result["WAIC"], and `score_chain(...)` a whole
macau() chain on a setWaic relation: the samplers are the run_chain of probit_restatement / censored_restatement /
interval_restatement / ordinal_restatement as they are; the factors and alpha are listened to after every iteration (as
lpd_restatement.chain_draws does), the ordinal chain's edges are read from its trace, and only the scoring is added.
"""
import math

import numpy as np

import censored_restatement as CR
import interval_restatement as IR
import lpd_restatement as LR
import ordinal_restatement as OR
import probit_restatement as PR
from probit_restatement import udot

HIGH = 0.4                        # a cell whose V exceeds this is counted


class Stream:
    """the running state of bdf_pairs_waic_update: phase 0 touches nothing and returns (l, 0); phase 1 starts (M, A, mean, M2) =
    (l, 1, l, 0); phase 2 folds l in: (M, A) as the lpd stream, d = l - mean, mean += d / draws, M2 += d (l - mean).  update returns
    (lppd, V) = (M + log A - log(draws), M2 / (draws - 1)), V = 0 while draws < 2"""

    def __init__(self):
        self.M = self.A = self.mean = self.M2 = None
        self.draws = 0

    def update(self, l, phase):
        l = np.asarray(l, dtype=np.float64)
        if phase == 0:
            return l.copy(), np.zeros_like(l)
        if phase == 1:
            self.M, self.A, self.mean, self.M2, self.draws = l.copy(), np.ones_like(l), l.copy(), np.zeros_like(l), 1
        else:
            self.draws += 1
            Mn = np.maximum(self.M, l)
            self.A = self.A * np.exp(self.M - Mn) + np.exp(l - Mn)
            self.M = Mn
            d = l - self.mean
            self.mean = self.mean + d / float(self.draws)
            self.M2 = self.M2 + d * (l - self.mean)
        return self.lppd(), self.V()

    def lppd(self):
        return self.M + np.log(self.A) - np.log(float(self.draws))

    def V(self):
        return self.M2 / float(self.draws - 1) if self.draws >= 2 else np.zeros_like(self.M2)


def stats(l, lppd, V):
    """the four statistics of one bdf_pairs_waic_update: sum l, sum lppd, sum V, the count of V > 0.4"""
    return np.array([math.fsum(l), math.fsum(lppd), math.fsum(V), float(np.count_nonzero(V > HIGH))])


def train_bounds(kind, values, censor=None, interval=None, codes=None, edges=None):
    """what kind of record every training row is, as (lo, hi) per row or None (no bounds: the density at the stored value, or the
    probit link):
      "gauss", "probit" -> None
      "censored"        -> flag 0: (y, y); +1: (y, +inf); -1: (-inf, y)
      "interval"        -> the relation's bounds as they stand (lo == hi a measurement)
      "ordinal"         -> the level's bin between `edges` (e_1 .. e_{K-1}): fixed edges k + 1/2, or this draw's"""
    y = np.asarray(values, dtype=np.float64)
    if kind in ("gauss", "probit"):
        return None
    if kind == "censored":
        c = np.asarray(censor)
        return np.stack([np.where(c < 0, -np.inf, y), np.where(c > 0, np.inf, y)], axis=1)
    if kind == "interval":
        return np.asarray(interval, dtype=np.float64)
    if kind == "ordinal":
        full = np.concatenate([[-np.inf], np.asarray(edges, dtype=np.float64), [np.inf]])
        return OR.bounds_of(codes, full)
    raise ValueError(kind)


def summary(lppd, V):
    """result["WAIC"] from the per-cell lppd and V: elpd_t = lppd_t - V_t; se = sqrt(n var_t(elpd_t)) with the population variance,
    from the squares about the mean"""
    lppd, V = np.asarray(lppd, dtype=np.float64), np.asarray(V, dtype=np.float64)
    n = len(lppd)
    s_lppd, s_V = math.fsum(lppd), math.fsum(V)
    e = lppd - V
    ss = math.fsum((e - (s_lppd - s_V) / n) ** 2) if n else 0.0
    return {"waic": -2.0 * (s_lppd - s_V), "elpd": s_lppd - s_V, "lppd": s_lppd, "p_waic": s_V, "se": math.sqrt(ss),
            "n_high": int(np.count_nonzero(V > HIGH)), "n": n, "ss": ss}


def chain_draws(kind, ids, values, dims, D, seed, burnin, psamples, alpha=1.0, alpha_sample=False, censor=None, interval=None, K=None,
                sample_edges=True, test_ids=None):
    """the sampler of the relation's kind, once, to iteration burnin + psamples.  Returns (its result, [the factors S after every
    iteration], [alpha of every iteration], [the edges e_1 .. e_{K-1} of every iteration] or None).  The chains keep neither the
    factors nor alpha: they evaluate udot(test_ids, S) at the end of every iteration and draw alpha through oracle.sample_alpha,
    and both are listened to while they run (without test cells the training ids stand in, as an object of their own)."""
    mod = {"gauss": IR, "interval": IR, "censored": CR, "probit": PR, "ordinal": OR}[kind]
    iters = burnin + psamples
    heard = np.array(ids) if test_ids is None else test_ids
    Ss, alphas = [], []
    real_udot, real_alpha = mod.udot, mod.O.sample_alpha

    def udot_heard(i, S):
        if i is heard:
            Ss.append([np.array(s) for s in S])
        return real_udot(i, S)

    def alpha_heard(*a, **k):
        alphas.append(real_alpha(*a, **k))
        return alphas[-1]

    mod.udot, mod.O.sample_alpha = udot_heard, alpha_heard
    try:
        if kind == "probit":
            out = PR.run_chain(ids, values, dims, D, seed, iters, test_ids=heard)
        elif kind == "censored":
            out = CR.run_chain(ids, values, censor, dims, D, seed, iters, alpha=alpha, alpha_sample=alpha_sample, test_ids=heard)
        elif kind == "ordinal":
            out = OR.run_chain(ids, values, dims, D, seed, burnin, psamples, K, alpha=alpha, alpha_sample=alpha_sample, test_ids=heard,
                               sample_edges=sample_edges)
        else:
            out = IR.run_chain(ids, values, interval, dims, D, seed, iters, alpha=alpha, alpha_sample=alpha_sample, test_ids=heard)
    finally:
        mod.udot, mod.O.sample_alpha = real_udot, real_alpha
    if not alpha_sample:
        alphas = [1.0 if kind == "probit" else float(alpha)] * iters
    assert len(Ss) == iters and len(alphas) == iters
    return out, Ss, alphas, (list(out["edges_trace"]) if kind == "ordinal" else None)


def score_chain(kind, ids, values, dims, D, seed, burnin, psamples, alpha=1.0, alpha_sample=False, censor=None, interval=None, K=None,
                sample_edges=True, test_ids=None, test_values=None):
    """macau() on one setWaic relation of `kind` ("gauss" / "probit" / "censored" / "interval" / "ordinal": values are the levels).
    Returns the last iteration's chain state with "waic" (summary), "lppd_t", "V_t", "elpd_trace" (the verbose line's ELPD after
    every iteration, burn-in included) and, with test_values, "LPD" / "lpd_t": the held-out cells scored as measurements"""
    out, Ss, alphas, edges = chain_draws(kind, ids, values, dims, D, seed, burnin, psamples, alpha, alpha_sample, censor, interval, K,
                                         sample_edges, test_ids)
    mean = 0.0 if kind == "probit" else out["mean"]
    y = np.asarray(values, dtype=np.float64)
    bounds = None if kind == "ordinal" else train_bounds(kind, y, censor, interval)
    st, held, trace = Stream(), LR.Stream(), []
    for it, (S, a) in enumerate(zip(Ss, alphas), start=1):
        if kind == "ordinal":
            bounds = train_bounds(kind, y, codes=y, edges=edges[it - 1])
        l = LR.cell_loglik(y, udot(ids, S) + mean, a, bounds, probit=kind == "probit")
        phase = 0 if it <= burnin else (1 if it == burnin + 1 else 2)
        lppd, V = st.update(l, phase)
        trace.append((math.fsum(lppd) - math.fsum(V)) / len(y))
        if test_values is not None:
            held.update(LR.cell_loglik(test_values, udot(test_ids, S) + mean, a, None, probit=kind == "probit"), phase)
    out = dict(out)
    out["elpd_trace"] = trace
    if psamples:
        out["lppd_t"], out["V_t"] = st.lppd(), st.V()
        out["waic"] = summary(out["lppd_t"], out["V_t"])
        if test_values is not None:
            out["lpd_t"] = held.lpd()
            out["LPD"] = float(np.mean(out["lpd_t"]))
    return out


# ---- the quality case: does WAIC on the training half choose the rank that the held-out half chooses? ----------------------------
QUALITY_SHAPE = (60, 40, 3)        # rows, columns, planted rank; half of the cells observed, the other half held out
QUALITY_ALPHA = 4.0                # the planted noise's precision (standard deviation 1 / 2), fixed in both fits
QUALITY_ITERS = (30, 30)           # burn-in, posterior draws


def planted_gauss(seed=0):
    """planted rank-3 Gaussian data on a 60 x 40 matrix: y = u*.v* + eps / 2, a random half of the cells the training table, the
    other half held out.  Returns (ids, y, n_test): the LAST n_test rows are the held-out ones"""
    N1, N2, rank = QUALITY_SHAPE
    rng = np.random.default_rng(seed)
    cells = rng.permutation(N1 * N2)
    ids = np.stack([cells // N2 + 1, cells % N2 + 1], axis=1).astype(np.int64)
    U, V = rng.standard_normal((N1, rank)), rng.standard_normal((N2, rank))
    y = (U[ids[:, 0] - 1] * V[ids[:, 1] - 1]).sum(axis=1) + 0.5 * rng.standard_normal(N1 * N2)
    return ids, y, (N1 * N2) // 2


def quality_fit(D, seed):
    """the restated fit at num_latent = D: (elpd per training cell, held-out LPD, the share of training cells with V > 0.4)"""
    ids, y, n_test = planted_gauss()
    N1, N2, _ = QUALITY_SHAPE
    r = score_chain("gauss", ids[:-n_test], y[:-n_test], [N1, N2], D, seed, QUALITY_ITERS[0], QUALITY_ITERS[1], alpha=QUALITY_ALPHA,
                    test_ids=ids[-n_test:], test_values=y[-n_test:])
    return r["waic"]["elpd"] / r["waic"]["n"], r["LPD"], r["waic"]["n_high"] / r["waic"]["n"]


# (elpd per cell at D = 3) - (at D = 1), and the same gap of the held-out LPD, on the seeds 2, 3, 4 as this restatement computes
# them: test_waic_host.py holds the record to the computation, test_gpu_waic.py the device to the record
QUALITY_SEEDS = (2, 3, 4)
QUALITY_ELPD_GAPS = (3.7189, 3.7046, 3.6896)
QUALITY_LPD_GAPS = (3.5502, 3.5720, 3.5509)
