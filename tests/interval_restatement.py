"""A numpy + scipy restatement of the interval-censored noise model for the interval tests.

`draw_z(m, lo, hi, alpha, u)` is the map from a uniform to the latent of one bounded observation that bdf_interval_draw documents
(include/bdf.h; an observation with lo == hi keeps its value, which the callers put back), `uniforms(seed, sweep, rel_tag, n)` the
uniforms it takes from the library's Philox streams (purpose 14, entity 0x800000 | rel_tag, row = observation, pair 0; checked
against oracle.draw in test_interval_host.py), and `run_chain(...)` whole macau() iterations on an interval relation: the chain of
censored_restatement.run_chain, in its order alpha | U,V,z -> z | U,V,alpha -> rows, hyperprior of every entity in turn -> beta of
every entity with features, with the interval draw in the place of the censored one.
"""
import numpy as np
from scipy.special import erfc, log_ndtr, ndtri

from oracle import oracle as O
from censored_restatement import TINY
from probit_restatement import _philox4x32_10, udot

P_INTERVAL = 14


def phi(t):
    """Phi(t) = erfc(-t / sqrt 2) / 2.  scipy's erfc returns 0 once t^2 / 2 exceeds 709.78 (t < -37.68), most of a standard
    deviation before Phi leaves the denormal range (t = -38.5), where the library's erfc still returns the denormal value; a lower
    bound in that band beside an upper bound above it then moves the draw by up to 1e-7 standard deviations.  Below -37.5:
    exp(log Phi), which is good to 1e-13 there (the denormals' own spacing)."""
    t = np.asarray(t, dtype=np.float64)
    far = t < -37.5
    with np.errstate(all="ignore"):
        return np.where(far, np.exp(log_ndtr(np.where(far, t, 0.0))), 0.5 * erfc(-t / 1.4142135623730951))


def draw_z(m, lo, hi, alpha, u, y=None):
    """z ~ N(m, 1 / alpha) truncated to [lo, hi] by inversion from u in (0, 1]; where lo == hi: y (lo itself when y is None)"""
    m, lo, hi, alpha, u = np.broadcast_arrays(*(np.asarray(a, dtype=np.float64) for a in (m, lo, hi, alpha, u)))
    ra = np.sqrt(alpha)
    with np.errstate(all="ignore"):
        a, b = (lo - m) * ra, (hi - m) * ra
        reflect = a + b > 0.0                     # False for the NaN of (-inf, +inf)
        a, b, s = np.where(reflect, -b, a), np.where(reflect, -a, b), np.where(reflect, -1.0, 1.0)
        v, vc = np.where(reflect, 1.0 - u, u), np.where(reflect, u, 1.0 - u)       # vc: the complement of v, from u itself
        Pa = phi(a)
        w = phi(b) - Pa
        p = Pa + v * w
        x = np.where(p < 0.5, ndtri(np.maximum(p, TINY)), -ndtri(np.maximum(phi(-b) + vc * w, TINY)))
        z = np.minimum(np.maximum(m + s * x / ra, lo), hi)
    exact = lo if y is None else np.broadcast_to(np.asarray(y, dtype=np.float64), m.shape)
    return np.where(lo == hi, exact, z)


def uniforms(seed, sweep, rel_tag, n):
    """the uniform of every observation 0 .. n-1: the first double of the block (P_INTERVAL, 0x800000 | rel_tag, row, pair 0)"""
    row = np.arange(n, dtype=np.uint64)
    ent = (0x800000 | int(rel_tag)) & 0xFFFFFF
    c = [row & np.uint64(0xFFFFFFFF), (row >> np.uint64(32)) & np.uint64(0xFFFF), np.full(n, int(sweep), dtype=np.uint64),
         np.full(n, (P_INTERVAL << 24) | ent, dtype=np.uint64)]
    o = _philox4x32_10(c, int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    x = (o[1] << np.uint64(32)) | o[0]
    return ((x >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53


def run_chain(ids, values, bounds, dims, D, seed, iters, alpha=1.0, alpha_sample=False, feats=None, use_ff=True, rel_tag=1,
              test_ids=None, burnin=0, alpha_lambda0=1.0, alpha_nu0=2.0):
    """macau() on ONE interval relation (ids (n, n_modes) 1-based, values, bounds (n, 2) = (lower, upper); bounds None: the
    Gaussian chain on the same row sampler) between len(dims) entities, entity k with the dense side information feats[k] (or
    None): iterations 1 .. iters.  Returns {"S", "mu", "Lam", "beta", "lb", "z", "alpha", "mean"} after the last one and, with
    test_ids, "pred": the mean over iterations burnin + 1 .. iters of udot + mean on those cells."""
    n_modes = len(dims)
    feats = feats or [None] * n_modes
    S = [np.zeros((n, D)) for n in dims]
    mu = [np.zeros(D) for _ in dims]
    Lam = [5.0 * np.eye(D) for _ in dims]
    ofe = [None if F is None else O.Feat.from_dense(np.asarray(F, dtype=np.float64)) for F in feats]
    beta = [None if f is None else np.zeros((f.n, D)) for f in ofe]
    lb = [1.0] * n_modes
    index = O.index_build(ids, list(dims))
    values = np.asarray(values, dtype=np.float64)
    mean = float(np.mean(values))
    z = values.copy()
    linear = np.full(len(values), mean)
    alpha = float(alpha)
    pred = None
    for it in range(1, iters + 1):
        dot = udot(ids, S)
        if alpha_sample:                 # the residual of the previous z (the values themselves before the first draw)
            sse = float(np.sum((values - (dot + linear)) ** 2))
            alpha = O.sample_alpha(alpha_lambda0, alpha_nu0, len(values), sse, seed, it, rel_tag)
        if bounds is not None:           # z | U, V, alpha from the previous iteration's rows
            z = draw_z(dot + mean, bounds[:, 0], bounds[:, 1], alpha, uniforms(seed, it, rel_tag, len(values)), y=values)
            linear = mean + (values - z)
        for j in range(n_modes):
            facs = [None if k == j else S[k] for k in range(n_modes)]
            term = O.Term(ids, values, list(dims), j, alpha, mean, facs, linear_values=linear, index=index)
            if ofe[j] is not None:
                uhat = np.stack([ofe[j].mul(beta[j][:, d]) for d in range(D)], axis=1)
                S[j] = O.sample_rows(D, dims[j], [term], mu[j] + uhat, Lam[j], seed, it, j + 1)
                U, nu, Tinv = S[j] - uhat, D + ofe[j].n, np.eye(D) + beta[j].T @ beta[j] * lb[j]
            else:
                S[j] = O.sample_rows(D, dims[j], [term], mu[j], Lam[j], seed, it, j + 1)
                U, nu, Tinv = S[j], float(D), np.eye(D)
            mu_N, beta_N, T_N, nu_N = O.hyper_params(U, np.zeros(D), 2.0, Tinv, nu)
            mu[j], Lam[j] = O.hyper_draw(mu_N, beta_N, T_N, nu_N, seed, it, j + 1)
        for j in range(n_modes):
            if ofe[j] is not None:
                beta[j], _, _ = O.sample_beta(ofe[j], S[j], mu[j], Lam[j], lb[j], use_ff, None, seed, it, j + 1)
                lb[j] = O.sample_lambda_beta(beta[j], Lam[j], 1e-3, 1.0, seed, it, j + 1)
        if test_ids is not None and it > burnin:
            p = udot(test_ids, S) + mean
            pred = p if pred is None else pred + p
    out = {"S": S, "mu": mu, "Lam": Lam, "beta": beta, "lb": lb, "z": z, "alpha": alpha, "mean": mean}
    if pred is not None:
        out["pred"] = pred / (iters - burnin)
    return out


BIN_EDGES = (-1.5, -0.5, 0.5, 1.5)


def planted_binned(seed=0, N1=300, N2=200, rank=4, n_cells=12000, n_test=3000, edges=BIN_EDGES):
    """planted binned data: the cells and exact values y = u*.v* + eps / 2 of censored_restatement.planted; the last n_test cells
    are held out with their exact values, the training values are reported as their bin's level (the bins between `edges`, open
    at both ends, levels -2 ... 2 for the five default bins: the bin's index minus the middle one's).  Returns (ids, y as reported,
    edges, n_test)"""
    rng = np.random.default_rng(seed)
    cells = rng.choice(N1 * N2, size=n_cells, replace=False)
    ids = np.stack([cells // N2 + 1, cells % N2 + 1], axis=1).astype(np.int64)
    U, V = rng.standard_normal((N1, rank)), rng.standard_normal((N2, rank))
    y = (U[ids[:, 0] - 1] * V[ids[:, 1] - 1]).sum(axis=1) + 0.5 * rng.standard_normal(n_cells)
    e = np.asarray(edges, dtype=np.float64)
    level = np.searchsorted(e, y, side="right") - len(e) / 2.0
    train = np.arange(n_cells) < n_cells - n_test
    return ids, np.where(train, level, y), e, n_test


def bin_bounds(values, edges):
    """(n, 2) bounds of the bins of `values`: bin j is e_j <= v < e_{j+1} with e_0 = -inf and e_K = +inf"""
    e = np.asarray(edges, dtype=np.float64)
    full = np.concatenate([[-np.inf], e, [np.inf]])
    j = np.searchsorted(e, np.asarray(values, dtype=np.float64), side="right")
    return np.stack([full[j], full[j + 1]], axis=1)


def iteration_case(n_modes, with_feat, alpha_sample):
    """the small relation of the whole-iteration test: (ids, values, bounds, dims, D, feats per entity, number of leading test
    cells, alpha, alpha_sample); cells drawn with replacement, so some repeat; about 30 % two-sided rows of width 0.2 ... 2 placed
    off-centre around y, 15 % right-open, 10 % left-open, 5 % (-inf, +inf), the rest exact"""
    rng = np.random.default_rng(60 + n_modes)
    dims = [40, 30, 12][:n_modes]
    n, D, n_test = 900, 8, 100
    ids = np.stack([rng.integers(1, d + 1, n) for d in dims], axis=1).astype(np.int64)
    for k, d in enumerate(dims):
        ids[:d, k] = np.arange(1, d + 1)                  # every id occurs: the entities have exactly dims rows
    y = rng.standard_normal(n)
    pick = rng.random(n)
    width, where = rng.uniform(0.2, 2.0, n), rng.uniform(0.1, 0.9, n)       # y sits at `where` of the way from lower to upper
    lo, hi = y.copy(), y.copy()
    two, right, left, none = pick < 0.3, (pick >= 0.3) & (pick < 0.45), (pick >= 0.45) & (pick < 0.55), (pick >= 0.55) & (pick < 0.6)
    lo[two], hi[two] = (y - where * width)[two], (y + (1.0 - where) * width)[two]
    lo[right], hi[right] = (y - where * width)[right], np.inf
    lo[left], hi[left] = -np.inf, (y + (1.0 - where) * width)[left]
    lo[none], hi[none] = -np.inf, np.inf
    lo[:n_test], hi[:n_test] = y[:n_test], y[:n_test]     # the test cells are measurements
    feats = [None] * n_modes
    if with_feat:
        feats[0] = rng.standard_normal((dims[0], 5))
    return ids, y, np.stack([lo, hi], axis=1), dims, D, feats, n_test, 2.5, bool(alpha_sample)
