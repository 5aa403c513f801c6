"""A numpy + scipy restatement of the held-out log predictive density for the lpd tests.

`log_phi`, `lpd_gauss`, `lpd_probit` and `lpd_mass` are the four scalar maps of csrc/lpd.h in the form the header states them (the
same branches at the same switch points, on scipy's erfc), `Stream` the streaming log-sum-exp of bdf_pairs_lpd_update with its
phases, `cell_loglik` the choice of a record's kind, and `score_chain(...)` a whole macau(lpd=True) chain: the samplers are the
run_chain of probit_restatement / interval_restatement (censored_restatement's chain with the interval draw in the place of the
censored one) as they are, and only the scoring of every iteration's draw is added.
"""
import numpy as np
from scipy.special import erfc

import interval_restatement as IR
import probit_restatement as PR
from probit_restatement import udot

HALF_LOG_2PI = 0.91893853320467274178
TAIL = -37.0                      # from here down log Phi takes its asymptotic form


def phi(x):
    return 0.5 * erfc(-np.asarray(x, dtype=np.float64) / 1.4142135623730951)


def log_tail_series(x):
    """log(1 - 1/x^2 + 3/x^4 - ... + 2027025/x^16): eight terms behind the 1"""
    with np.errstate(all="ignore"):
        r = 1.0 / (np.asarray(x, dtype=np.float64) ** 2)
        return np.log1p(r * (-1.0 + r * (3.0 + r * (-15.0 + r * (105.0 + r * (-945.0 + r * (10395.0 + r * (-135135.0 + r * 2027025.0))))))))


def log_phi(x):
    """log Phi(x): log1p(-Phi(-x)) for x >= 0, log(Phi(x)) for -37 < x < 0, the asymptotic form from -37 down"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        up = np.log1p(-phi(-np.maximum(x, 0.0)))
        mid = np.log(phi(np.clip(x, TAIL, 0.0)))
        xt = np.minimum(x, TAIL)
        far = -0.5 * xt * xt - np.log(-xt) - HALF_LOG_2PI + log_tail_series(xt)
    return np.where(x >= 0.0, up, np.where(x > TAIL, mid, far))


def lpd_gauss(y, m, alpha):
    y, m, alpha = (np.asarray(a, dtype=np.float64) for a in (y, m, alpha))
    e = y - m
    return 0.5 * np.log(alpha / 6.283185307179586476925286766559) - 0.5 * alpha * (e * e)


def lpd_probit(y, m):
    y, m = np.asarray(y, dtype=np.float64), np.asarray(m, dtype=np.float64)
    return log_phi(np.where(y > 0.5, m, -m))


def lpd_mass(m, lo, hi, alpha):
    """log(Phi(b) - Phi(a)), a = (lo - m) sqrt(alpha), b = (hi - m) sqrt(alpha); lo < hi, either may be infinite"""
    m, lo, hi, alpha = np.broadcast_arrays(*(np.asarray(t, dtype=np.float64) for t in (m, lo, hi, alpha)))
    ra = np.sqrt(alpha)
    with np.errstate(all="ignore"):
        a, b = (lo - m) * ra, (hi - m) * ra
        reflect = a + b > 0.0                     # False for the NaN of (-inf, +inf)
        a, b = np.where(reflect, -b, a), np.where(reflect, -a, b)
        near = np.log(phi(b) - phi(a))
        bt, at = np.minimum(b, TAIL), np.minimum(a, TAIL)       # (the far branch is taken only where a < b <= -37)
        Lb = log_phi(bt)
        d = 0.5 * (bt - at) * (at + bt) - np.log(at / bt) + (log_tail_series(at) - log_tail_series(bt))
        far = np.where(np.isneginf(a), Lb, Lb + np.log(-np.expm1(d)))
    return np.where(b > TAIL, near, far)


def cell_loglik(y, m, alpha, bounds=None, probit=False):
    """the log-likelihood of every cell's kind of record: probit -> the 0/1 map; bounds None or lower == upper -> the Gaussian
    density at y; lower < upper -> the interval's mass"""
    if probit:
        return lpd_probit(y, m)
    g = lpd_gauss(y, m, alpha)
    if bounds is None:
        return g
    lo, hi = bounds[:, 0], bounds[:, 1]
    open_ = lo != hi
    safe_hi = np.where(open_, hi, lo + 1.0)           # (a placeholder width where the row is exact: not used)
    return np.where(open_, lpd_mass(m, lo, safe_hi, alpha), g)


class Stream:
    """the streaming log-sum-exp of bdf_pairs_lpd_update: phase 0 touches nothing and returns l; phase 1 starts (M, A) = (l, 1);
    phase 2 folds l in; update returns lpd = M + log A - log(draws)"""

    def __init__(self):
        self.M = self.A = None
        self.draws = 0

    def update(self, l, phase):
        l = np.asarray(l, dtype=np.float64)
        if phase == 0:
            return l.copy()
        if phase == 1:
            self.M, self.A, self.draws = l.copy(), np.ones_like(l), 1
        else:
            Mn = np.maximum(self.M, l)
            self.A = self.A * np.exp(self.M - Mn) + np.exp(l - Mn)
            self.M = Mn
            self.draws += 1
        return self.lpd()

    def lpd(self):
        return self.M + np.log(self.A) - np.log(float(self.draws))


def chain_draws(kind, ids, values, dims, D, seed, iters, test_ids, alpha=1.0, alpha_sample=False, bounds=None):
    """the sampler: run_chain of probit_restatement (kind "probit") or interval_restatement ("gauss": bounds None; "interval"), once,
    to iteration `iters`.  Returns (its result, [the factors S after every iteration], [alpha of every iteration]).  run_chain
    keeps neither; it evaluates udot(test_ids, S) at the end of every iteration and draws alpha through oracle.sample_alpha, and
    both are listened to while it runs."""
    mod = PR if kind == "probit" else IR
    Ss, alphas = [], []
    real_udot, real_alpha = mod.udot, mod.O.sample_alpha

    def udot_heard(i, S):
        if i is test_ids:
            Ss.append([np.array(s) for s in S])
        return real_udot(i, S)

    def alpha_heard(*a, **k):
        alphas.append(real_alpha(*a, **k))
        return alphas[-1]

    mod.udot, mod.O.sample_alpha = udot_heard, alpha_heard
    try:
        if kind == "probit":
            out = PR.run_chain(ids, values, dims, D, seed, iters, test_ids=test_ids)
        else:
            out = IR.run_chain(ids, values, bounds, dims, D, seed, iters, alpha=alpha, alpha_sample=alpha_sample, test_ids=test_ids)
    finally:
        mod.udot, mod.O.sample_alpha = real_udot, real_alpha
    if not alpha_sample:
        alphas = [1.0 if kind == "probit" else float(alpha)] * iters
    assert len(Ss) == iters and len(alphas) == iters
    return out, Ss, alphas


def score_chain(kind, ids, values, dims, D, seed, burnin, psamples, test_ids, test_values, alpha=1.0, alpha_sample=False,
                bounds=None, test_bounds=None):
    """macau(lpd=True) on one relation: kind "gauss" (bounds None) / "interval" (bounds (n, 2)) / "probit".  Returns the last
    iteration's chain state with "lpd" (per test cell), "LPD" (its mean), "loglik" (the last draw's per-cell log-likelihood) and
    "lpd_trace" (the mean lpd after every iteration, burn-in included)"""
    out, Ss, alphas = chain_draws(kind, ids, values, dims, D, seed, burnin + psamples, test_ids, alpha, alpha_sample, bounds)
    mean = 0.0 if kind == "probit" else out["mean"]
    st, trace, l = Stream(), [], None
    for it, (S, a) in enumerate(zip(Ss, alphas), start=1):
        l = cell_loglik(test_values, udot(test_ids, S) + mean, a, test_bounds, probit=kind == "probit")
        phase = 0 if it <= burnin else (1 if it == burnin + 1 else 2)
        trace.append(float(np.mean(st.update(l, phase))))
    out = dict(out)
    out["loglik"], out["lpd_trace"] = l, trace
    if psamples:
        out["lpd"] = st.lpd()
        out["LPD"] = float(np.mean(out["lpd"]))
    return out
