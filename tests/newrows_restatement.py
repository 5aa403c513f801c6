"""A numpy restatement of the prediction of cells of NEW rows (setNewRows / setNewTest), line by line from the
formulas, for the newrows tests.

Given one posterior draw (mu, Lambda, beta, V, alpha) of an entity with side information, the factor of a new row with features f is
u* ~ N(uhat, Lambda^-1), uhat = mu + beta' f, and it is integrated out of the cell (i*, j):
  m = mean_value + uhat_i* . v_j,   q_j = v_j' Lambda^-1 v_j  (np.linalg.solve)
  identity link:  y | draw ~ N(m, q_j + 1 / alpha);   probit link:  P(y = 1 | draw) = Phi(m / sqrt(1 + q_j)).
`Stream` is the running state of bdf_newrows_update with its phases, `scalars` the eight sums over the cells with a value, `result`
the (pred, stdev, lpd) of bdf_newrows_result; `planted` the planted Macau data of the end-to-end and quality tests and `gibbs` a
small dense-feature Macau Gibbs sampler in plain numpy (direct beta solve) that the quality figures of the CPU side come from.
"""
import math

import numpy as np

import lpd_restatement as LR


# ---- one draw ---------------------------------------------------------------------------------------------------------------------
def quad(Lambda, V):
    """q_j = v_j' Lambda^-1 v_j for every row of V (M x D)"""
    V = np.asarray(V, dtype=np.float64)
    return np.einsum("md,dm->m", V, np.linalg.solve(np.asarray(Lambda, dtype=np.float64), V.T))


def uhat(mu, beta, F):
    """the conditional mean of the new rows' factors: mu + beta' f per row of F (n* x numF), beta numF x D"""
    return np.asarray(mu, dtype=np.float64)[None, :] + np.asarray(F, dtype=np.float64) @ np.asarray(beta, dtype=np.float64)


def cells(ids, uh, V, q, mean_value):
    """(m, q) per cell; ids (n, 2), 1-based: the new row, then the row of V"""
    i, j = ids[:, 0] - 1, ids[:, 1] - 1
    return mean_value + np.sum(uh[i] * V[j], axis=1), q[j]


def predict(probit, m, q):
    return LR.phi(m / np.sqrt(1.0 + q)) if probit else np.asarray(m, dtype=np.float64).copy()


def loglik(probit, y, m, q, alpha):
    """log p(y | draw) of the cells with a value; NaN where y is NaN"""
    y = np.asarray(y, dtype=np.float64)
    has = ~np.isnan(y)
    ys = np.where(has, y, 0.0)
    l = LR.lpd_probit(ys, m / np.sqrt(1.0 + q)) if probit else LR.lpd_gauss(ys, m, 1.0 / (q + 1.0 / alpha))
    return np.where(has, l, np.nan)


# ---- the running state ------------------------------------------------------------------------------------------------------------
class Stream:
    """Welford's (mean, M2) of the prediction p, the running sum of q and the streaming log-sum-exp (M, A) of l: phase 0 touches
    nothing, phase 1 starts, phase 2 folds a draw in.  update returns (avg, lpd): the running mean after the draw (phase 0: p) and
    M + log A - log(draws) (phase 0: l); lpd is NaN where l is"""

    def __init__(self):
        self.mean = self.M2 = self.sq = self.M = self.A = None
        self.draws = 0

    def update(self, p, q, l, phase):
        p, q, l = (np.asarray(a, dtype=np.float64) for a in (p, q, l))
        if phase == 0:
            return p.copy(), l.copy()
        if phase == 1:
            self.mean, self.M2, self.sq, self.draws = p.copy(), np.zeros_like(p), q.copy(), 1
            self.M, self.A = l.copy(), np.ones_like(l)
        else:
            self.draws += 1
            d = p - self.mean
            self.mean = self.mean + d / self.draws
            self.M2 = self.M2 + d * (p - self.mean)
            self.sq = self.sq + q
            with np.errstate(invalid="ignore"):
                Mn = np.maximum(self.M, l)
                self.A = self.A * np.exp(self.M - Mn) + np.exp(l - Mn)
            self.M = Mn
        return self.mean.copy(), self.lpd()

    def lpd(self):
        return self.M + np.log(self.A) - math.log(float(self.draws))

    def stdev(self, probit):
        if self.draws < 2:
            return np.full_like(self.mean, np.nan)
        return np.sqrt(self.M2 / (self.draws - 1.0) + (0.0 if probit else self.sq / self.draws))


def clamped(x, clamp):
    return np.clip(x, clamp[0], clamp[1]) if len(clamp) else x


def scalars(y, avg, p, lpd, l, clamp, cut, score):
    """bdf_newrows_update's stats_out over the cells with a value (math.fsum: the reference of a fixed-order sum)"""
    has = ~np.isnan(y)
    yy, a, pp = y[has], clamped(avg[has], clamp), clamped(p[has], clamp)
    lab = yy < cut
    return np.array([math.fsum((yy - a) ** 2), math.fsum((yy - pp) ** 2), float(np.sum(lab == (avg[has] < cut))), float(np.sum(lab == (p[has] < cut))),
                     float(has.sum()), math.fsum(lpd[has]) if score else 0.0, math.fsum(l[has]) if score else 0.0, 0.0])


# ---- planted Macau data -----------------------------------------------------------------------------------------------------------
def planted(n_train, n_new, M, numF, D, density, noise, seed, binary=False, signal=1.0):
    """Factors exactly linear in the features plus N(0, 0.1^2): U = F B + 0.1 E for the n_train + n_new rows (B ~ N(0, signal^2 / numF)), V ~ N(0, 1),
    y = U V' + noise eps; `density` of the cells observed.  Returns F_train, F_new, the training table (ids 1-based, values) and
    the new rows' table (every observed cell of a new row, ids 1 ... n_new).  binary: 0/1 features (Bernoulli 0.4)"""
    rng = np.random.default_rng(seed)
    N = n_train + n_new
    F = (rng.random((N, numF)) < 0.4).astype(np.float64) if binary else rng.standard_normal((N, numF))
    Bm = signal * rng.standard_normal((numF, D)) / math.sqrt(numF)
    U = F @ Bm + 0.1 * rng.standard_normal((N, D))
    V = rng.standard_normal((M, D))
    Y = U @ V.T + noise * rng.standard_normal((N, M))
    seen = rng.random((N, M)) < density
    seen[np.arange(n_train), np.arange(n_train) % M] = True                                   # every training row and
    seen[np.arange(M) % n_train, np.arange(M)] = True                                         # ... every column holds a training cell
    i, j = np.nonzero(seen)
    tr = i < n_train
    train = (np.stack([i[tr] + 1, j[tr] + 1], axis=1), Y[i[tr], j[tr]])
    new = (np.stack([i[~tr] - n_train + 1, j[~tr] + 1], axis=1), Y[i[~tr], j[~tr]])
    return F[:n_train], F[n_train:], train, new


# ---- a small Macau Gibbs sampler (dense features, direct beta solve) -----------------------------------------------------------
def _wishart(rng, nu, T):
    """Wishart(nu, T) by Bartlett's decomposition"""
    D = T.shape[0]
    A = np.tril(rng.standard_normal((D, D)), -1)
    A[np.diag_indices(D)] = np.sqrt(rng.chisquare(nu - np.arange(D)))
    LA = np.linalg.cholesky(T) @ A
    return LA @ LA.T


def _normal_wishart(rng, U, mu0, b0, Tinv, nu):
    N = U.shape[0]
    s, S = U.sum(axis=0), U.T @ U
    bN, muN = b0 + N, (b0 * mu0 + s) / (b0 + N)
    T = np.linalg.inv(Tinv + S + b0 * np.outer(mu0, mu0) - bN * np.outer(muN, muN))
    Lam = _wishart(rng, nu + N, 0.5 * (T + T.T))
    mu = muN + np.linalg.solve(np.linalg.cholesky(Lam * bN).T, rng.standard_normal(len(mu0)))
    return mu, Lam


def _rows(rng, ids_own, ids_other, r, Vo, alpha, mu_rows, Lam, N):
    """every row of one entity from its conditional: precision Lam + alpha sum v v', mean from Lam mu_i + alpha sum r v"""
    D = Vo.shape[1]
    out = np.zeros((N, D))
    order = np.argsort(ids_own, kind="stable")
    bounds = np.searchsorted(ids_own[order], np.arange(N + 1))
    for i in range(N):
        sel = order[bounds[i]:bounds[i + 1]]
        Vi = Vo[ids_other[sel]]
        P = Lam + alpha * (Vi.T @ Vi)
        b = Lam @ mu_rows[i] + alpha * (Vi.T @ r[sel])
        L = np.linalg.cholesky(P)
        out[i] = np.linalg.solve(P, b) + np.linalg.solve(L.T, rng.standard_normal(D))
    return out


def gibbs(F, train, F_new, new, M, D, alpha, burnin, psamples, seed, lambda_beta=1.0, nu_lb=1e-3, mu_lb=1.0):
    """Macau on one two-mode relation whose first entity has dense features F (macau.jl's order: rows of both entities with their
    hyperpriors, then beta and lambda_beta), with the new cells `new` predicted behind every posterior draw by the formulas above.
    Returns {"pred", "stdev", "rmse", "ratio", "coverage", "alpha"}: ratio = (cold RMSE) / (RMSE of predicting mean_value),
    coverage the share of held-out values inside pred +- 1.645 sqrt(stdev^2 + 1 / alpha)"""
    rng = np.random.default_rng(seed)
    ids, y = train
    iu, iv = ids[:, 0] - 1, ids[:, 1] - 1
    N, numF = F.shape
    mean = float(y.mean())
    r = y - mean
    U, V = np.zeros((N, D)), np.zeros((M, D))
    mu_u, Lam_u, mu_v, Lam_v = np.zeros(D), 5.0 * np.eye(D), np.zeros(D), 5.0 * np.eye(D)
    beta = np.zeros((numF, D))
    FF = F.T @ F
    lb = float(lambda_beta)
    st = Stream()
    new_ids, new_y = new
    for it in range(1, burnin + psamples + 1):
        uh = F @ beta
        U = _rows(rng, iu, iv, r, V, alpha, mu_u[None, :] + uh, Lam_u, N)
        mu_u, Lam_u = _normal_wishart(rng, U - uh, np.zeros(D), 2.0, np.eye(D) + lb * (beta.T @ beta), D + numF)
        V = _rows(rng, iv, iu, r, U, alpha, np.tile(mu_v, (M, 1)), Lam_v, M)
        mu_v, Lam_v = _normal_wishart(rng, V, np.zeros(D), 2.0, np.eye(D), D)
        Lc = np.linalg.cholesky(np.linalg.inv(Lam_u))
        rhs = F.T @ ((U - mu_u) + rng.standard_normal((N, D)) @ Lc.T) + math.sqrt(lb) * (rng.standard_normal((numF, D)) @ Lc.T)
        beta = np.linalg.solve(FF + lb * np.eye(numF), rhs)
        nux = nu_lb + numF * D
        mux = mu_lb * nux / (nu_lb + mu_lb * np.trace((beta.T @ beta) @ Lam_u))
        lb = rng.gamma(nux / 2.0, 2.0 * mux / nux)
        if it > burnin:
            m, q = cells(new_ids, uhat(mu_u, beta, F_new), V, quad(Lam_u, V), mean)
            st.update(predict(False, m, q), q, loglik(False, new_y, m, q, alpha), 1 if it == burnin + 1 else 2)
    return quality(st.mean, st.stdev(False), new_y, mean, alpha)


def quality(pred, stdev, y, mean_value, alpha):
    has = ~np.isnan(y)
    rmse = math.sqrt(np.mean((y[has] - pred[has]) ** 2))
    base = math.sqrt(np.mean((y[has] - mean_value) ** 2))
    half = 1.645 * np.sqrt(stdev[has] ** 2 + 1.0 / alpha)
    return {"pred": pred, "stdev": stdev, "rmse": rmse, "ratio": rmse / base, "coverage": float(np.mean(np.abs(y[has] - pred[has]) <= half)),
            "alpha": alpha}


# ---- the quality record ----------------------------------------------------------------------------------
QUALITY_SHAPE = dict(n_train=300, n_new=100, M=60, numF=6, D=4, density=0.4, noise=0.3, seed=2024)
QUALITY_ITERS = (50, 100)
QUALITY_ALPHA = 1.0 / 0.09
QUALITY_SEEDS = (1, 2, 3, 4, 5)
# the five CPU chains' figures (gibbs on the seeds above): ratio = (cold RMSE) / (RMSE of predicting mean_value), coverage of
# pred +- 1.645 sqrt(stdev^2 + 1 / alpha); tests/test_newrows_host.py recomputes the first
QUALITY_CPU_RATIOS = (0.16568642, 0.16555984, 0.16550531, 0.16551826, 0.16551248)
QUALITY_CPU_COVERAGE = (0.90806045, 0.90931990, 0.90764064, 0.90973971, 0.91099916)
