"""The convergence diagnostics of DESIGN.md section 32 restated in numpy, vectorised over the series: what csrc/k_diag.hip is held
to.  Not a test module.

For one series x_1 .. x_n (n >= 4): h = n // 2, the two chains are the first h and the last h values (an odd n leaves the middle
one out); W the mean of the chains' variances (divisor h - 1); var+ = W (h - 1) / h + (mean_1 - mean_2)^2 / 2; R-hat =
sqrt(var+ / W); acov_j(t) = (1 / h) sum_i (c_j[i] - mean_j)(c_j[i + t] - mean_j) on the centred values; rho_0 = 1 and rho_t = 1 -
(W - (acov_1(t) + acov_2(t)) / 2) / var+; Geyer's initial monotone sequence P_k = rho_2k + rho_2k+1 for 2k + 1 <= h - 1, up to
the first P_k <= 0, each kept P_k replaced by min(P_k, P_k-1); tau = -1 + 2 sum P_k; cap = 2h log10(2h); ESS = cap if tau <= 0
else min(2h / tau, cap); MCSE = sqrt(var+ / ESS).  A series with W = 0 or a value that is not finite gives three NaN.
"""
import numpy as np


def pair_sums(x):
    """(P, bad, W, varp) of the series in the columns of x (n, cells): P (K, cells) the RAW pair sums P_k = rho_2k + rho_2k+1 for
    every k with 2k + 1 <= h - 1, before the stop and the monotone minimum"""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    h = n // 2
    assert h >= 2, "a split chain needs at least 4 draws"
    bad = ~np.isfinite(x).all(axis=0)
    c = np.stack([x[:h], x[n - h:]])                       # (2, h, cells)
    c = np.where(bad, 0.0, c)
    mean = c.mean(axis=1)
    d = c - mean[:, None, :]
    s2 = (d * d).sum(axis=1) / (h - 1)
    W = s2.mean(axis=0)
    varp = W * (h - 1) / h + (mean[0] - mean[1]) ** 2 / 2.0
    bad |= ~(W > 0.0) | ~np.isfinite(W)
    Ws, vs = np.where(bad, 1.0, W), np.where(bad, 1.0, varp)
    rho = np.ones((h, x.shape[1]))
    for t in range(1, h):
        acov = (d[:, :h - t] * d[:, t:]).sum(axis=1) / h   # (2, cells)
        rho[t] = 1.0 - (Ws - acov.mean(axis=0)) / vs
    K = h // 2                                             # k = 0 .. K - 1: 2k + 1 <= h - 1
    P = rho[0:2 * K:2] + rho[1:2 * K:2]
    return P, bad, np.where(bad, np.nan, W), np.where(bad, np.nan, varp)


def geyer(P):
    """(tau, the kept and replaced P_k with NaN behind the stop) from the raw pair sums"""
    kept = np.full(P.shape, np.nan)
    alive = np.ones(P.shape[1], dtype=bool)
    prev = np.full(P.shape[1], np.inf)
    total = np.zeros(P.shape[1])
    for k in range(P.shape[0]):
        alive &= ~(P[k] <= 0.0)
        pk = np.minimum(P[k], prev)
        kept[k] = np.where(alive, pk, np.nan)
        total += np.where(alive, pk, 0.0)
        prev = np.where(alive, pk, prev)
    return -1.0 + 2.0 * total, kept


def diagnostics(x):
    """(rhat, ess, mcse), one entry per column of x (n, cells); NaN three times for a series without figures"""
    x = np.asarray(x, dtype=np.float64)
    h = x.shape[0] // 2
    P, bad, W, varp = pair_sums(x)
    tau, _ = geyer(P)
    cap = 2 * h * np.log10(2 * h)
    with np.errstate(divide="ignore", invalid="ignore"):
        ess = np.where(tau <= 0.0, cap, np.minimum(2 * h / np.where(tau <= 0.0, 1.0, tau), cap))
        rhat = np.sqrt(varp / W)
        ess = np.where(bad, np.nan, ess)
        mcse = np.sqrt(varp / ess)
    return rhat, ess, mcse


def decisions_clear(x, margin=1e-9):
    """whether no deciding P_k of any series lies within `margin` of zero or of its predecessor (the stop and the monotone minimum
    are discrete: a device sum in another order may only be compared where they are not on the edge), nor 2h / tau of the cap"""
    x = np.asarray(x, dtype=np.float64)
    h = x.shape[0] // 2
    P, bad, _, _ = pair_sums(x)
    tau, kept = geyer(P)
    ok = np.ones(P.shape[1], dtype=bool)
    alive = ~bad
    prev = np.full(P.shape[1], np.inf)
    for k in range(P.shape[0]):
        ok &= ~alive | (np.abs(P[k]) > margin)             # the stop
        alive = alive & ~(P[k] <= 0.0)
        ok &= ~alive | (np.abs(P[k] - prev) > margin)      # the minimum
        prev = np.where(alive, kept[k], prev)
    cap = 2 * h * np.log10(2 * h)
    ok &= bad | (np.abs(tau) > margin)
    with np.errstate(divide="ignore", invalid="ignore"):
        ok &= bad | (tau <= 0.0) | (np.abs(2 * h / tau - cap) > margin * cap)
    return bool(ok.all())


def summary(rhat, ess, rhat_cut, ess_cut):
    """the run's summary over the cells' columns: a cell without figures is counted as constant and is in no other figure"""
    good = ~np.isnan(rhat)
    return {"max_rhat": float(rhat[good].max()) if good.any() else float("nan"), "min_ess": float(ess[good].min()) if good.any() else float("nan"),
            "n_rhat_high": int((rhat[good] > rhat_cut).sum()), "n_ess_low": int((ess[good] < ess_cut).sum()), "n_constant": int((~good).sum())}


def ar1(rng, n, phi, cells=1):
    """stationary AR(1) series with unit innovation variance, (n, cells)"""
    e = rng.standard_normal((n, cells))
    x = np.empty((n, cells))
    x[0] = e[0] / np.sqrt(1.0 - phi * phi)
    for i in range(1, n):
        x[i] = phi * x[i - 1] + e[i]
    return x
