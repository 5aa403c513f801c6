"""A numpy + scipy restatement of the censored (Tobit) noise model for the censored tests.

`draw_z(m, y, c, alpha, u)` is the map from a uniform to the latent of one observation that bdf_censored_draw documents
(include/bdf.h), `uniforms(seed, sweep, rel_tag, n)` the uniforms it takes from the library's Philox streams (purpose 13, entity
0x800000 | rel_tag, row = observation, pair 0; checked against oracle.draw in test_censored_host.py), and `run_chain(...)` whole
macau() iterations on a censored relation built from the oracle's row sampler, hyperprior, sample_alpha and beta update in the
library's order: alpha | U,V,z -> z | U,V,alpha -> rows, hyperprior of every entity in turn -> beta of every entity with features.
"""
import numpy as np
from scipy.special import erfc, ndtri

from oracle import oracle as O
from probit_restatement import _philox4x32_10, udot

P_CENSORED = 13
TINY = np.finfo(np.float64).tiny          # DBL_MIN


def phi(t):
    """Phi(t) = erfc(-t / sqrt 2) / 2"""
    return 0.5 * erfc(-np.asarray(t, dtype=np.float64) / 1.4142135623730951)


def draw_z(m, y, c, alpha, u):
    """z ~ N(m, 1 / alpha) truncated to z >= y (c = +1) or z <= y (c = -1) by inversion from u in (0, 1]; c = 0: z = y"""
    m, y, alpha, u = np.broadcast_arrays(*(np.asarray(a, dtype=np.float64) for a in (m, y, alpha, u)))
    c = np.broadcast_to(np.asarray(c), m.shape)
    s = np.where(c > 0, 1.0, -1.0)
    ra = np.sqrt(alpha)
    t = s * (m - y) * ra
    Pt = phi(t)
    lo = phi(-t) + u * Pt
    with np.errstate(all="ignore"):
        x = np.where(lo < 0.5, ndtri(np.maximum(lo, TINY)), -ndtri(np.maximum((1.0 - u) * Pt, TINY)))
    z = m + s * x / ra
    z = y + s * np.maximum(s * (z - y), 0.0)
    return np.where(c == 0, y, z)


def uniforms(seed, sweep, rel_tag, n):
    """the uniform of every observation 0 .. n-1: the first double of the block (P_CENSORED, 0x800000 | rel_tag, row, pair 0)"""
    row = np.arange(n, dtype=np.uint64)
    ent = (0x800000 | int(rel_tag)) & 0xFFFFFF
    c = [row & np.uint64(0xFFFFFFFF), (row >> np.uint64(32)) & np.uint64(0xFFFF), np.full(n, int(sweep), dtype=np.uint64),
         np.full(n, (P_CENSORED << 24) | ent, dtype=np.uint64)]
    o = _philox4x32_10(c, int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    x = (o[1] << np.uint64(32)) | o[0]
    return ((x >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53


def run_chain(ids, values, censor, dims, D, seed, iters, alpha=1.0, alpha_sample=False, feats=None, use_ff=True, rel_tag=1,
              test_ids=None, burnin=0, alpha_lambda0=1.0, alpha_nu0=2.0):
    """macau() on ONE censored relation (ids (n, n_modes) 1-based, values, censor in {-1, 0, +1}; censor None: the Gaussian chain
    on the same row sampler) between len(dims) entities, entity k with the dense side information feats[k] (or None):
    iterations 1 .. iters.  Returns {"S", "mu", "Lam", "beta", "lb", "z", "alpha", "mean"} after the last one and, with
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
        if censor is not None:           # z | U, V, alpha from the previous iteration's rows
            z = draw_z(dot + mean, values, censor, alpha, uniforms(seed, it, rel_tag, len(values)))
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


def planted(seed=0, N1=300, N2=200, rank=4, n_cells=12000, n_test=3000, upper=0.5, lower=-3.0):
    """planted censored data: distinct cells of an N1 x N2 matrix, y = u*.v* + eps / 2 (noise precision 4); the last n_test cells
    are held out with their exact values; training values above `upper` are reported as (upper, +1), those below `lower` as
    (lower, -1).  Returns (ids, y as reported, censor flags (0 on the held-out cells), n_test)"""
    rng = np.random.default_rng(seed)
    cells = rng.choice(N1 * N2, size=n_cells, replace=False)
    ids = np.stack([cells // N2 + 1, cells % N2 + 1], axis=1).astype(np.int64)
    U, V = rng.standard_normal((N1, rank)), rng.standard_normal((N2, rank))
    y = (U[ids[:, 0] - 1] * V[ids[:, 1] - 1]).sum(axis=1) + 0.5 * rng.standard_normal(n_cells)
    c = np.zeros(n_cells, dtype=np.int8)
    train = np.arange(n_cells) < n_cells - n_test
    hi, lo = train & (y > upper), train & (y < lower)
    y, c = np.where(hi, upper, np.where(lo, lower, y)), np.where(hi, 1, np.where(lo, -1, 0)).astype(np.int8)
    return ids, y, c, n_test


def iteration_case(n_modes, with_feat, alpha_sample):
    """the small relation of the whole-iteration test: (ids, values, censor, dims, D, feats per entity, number of leading test
    cells, alpha, alpha_sample); cells drawn with replacement, so some repeat; about 30 % right- and 10 % left-censored"""
    rng = np.random.default_rng(40 + n_modes)
    dims = [40, 30, 12][:n_modes]
    n, D, n_test = 900, 8, 100
    ids = np.stack([rng.integers(1, d + 1, n) for d in dims], axis=1).astype(np.int64)
    for k, d in enumerate(dims):
        ids[:d, k] = np.arange(1, d + 1)                  # every id occurs: the entities have exactly dims rows
    y = rng.standard_normal(n)
    pick = rng.random(n)
    c = np.where(pick < 0.3, 1, np.where(pick < 0.4, -1, 0)).astype(np.int8)
    c[:n_test] = 0                                        # the test cells are measurements
    feats = [None] * n_modes
    if with_feat:
        feats[0] = rng.standard_normal((dims[0], 5))
    return ids, y, c, dims, D, feats, n_test, 2.5, bool(alpha_sample)
