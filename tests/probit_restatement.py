"""A numpy + scipy restatement of the probit noise model for the probit tests.

`draw_z(m, y, u)` is the map from a uniform to the truncated-normal latent that bdf_probit_draw documents (include/bdf.h),
`uniforms(seed, sweep, rel_tag, n)` the uniforms it takes from the library's Philox streams (DESIGN.md "RNG contract": purpose 12,
entity 0x800000 | rel_tag, row = observation, pair 0; checked against oracle.draw in test_probit_host.py), and `run_chain(...)`
whole macau() iterations on a probit relation built from the oracle's row sampler, hyperprior and beta update in the library's
order: z | U,V -> rows, hyperprior of every entity in turn -> beta of every entity with features.
"""
import numpy as np
from scipy.special import erfc, ndtr, ndtri

from oracle import oracle as O

P_PROBIT = 12
TINY = np.finfo(np.float64).tiny          # DBL_MIN


def phi(t):
    """Phi(t) = erfc(-t / sqrt 2) / 2"""
    return 0.5 * erfc(-np.asarray(t, dtype=np.float64) / np.sqrt(2.0))


def draw_z(m, y, u):
    """z ~ N(m, 1) truncated to y's side of 0 (z > 0 for y = 1, z < 0 for y = 0) by inversion from u in (0, 1)"""
    m, y, u = (np.asarray(a, dtype=np.float64) for a in (m, y, u))
    s = np.where(y > 0.5, 1.0, -1.0)
    t = s * m
    Pt = phi(t)
    lo = phi(-t) + u * Pt
    with np.errstate(all="ignore"):
        x = np.where(lo < 0.5, ndtri(np.maximum(lo, TINY)), -ndtri(np.maximum((1.0 - u) * Pt, TINY)))
    z = m + s * x
    return s * np.maximum(s * z, TINY)


def _philox4x32_10(c, k0, k1):
    """Philox4x32-10 on columns of uint64-held 32-bit words; c: (4, n)"""
    M32 = np.uint64(0xFFFFFFFF)
    c = [np.asarray(x, dtype=np.uint64) for x in c]
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return c


def uniforms(seed, sweep, rel_tag, n):
    """the uniform of every observation 0 .. n-1: the first double of the block (P_PROBIT, 0x800000 | rel_tag, row, pair 0)"""
    row = np.arange(n, dtype=np.uint64)
    ent = (0x800000 | int(rel_tag)) & 0xFFFFFF
    c = [row & np.uint64(0xFFFFFFFF), (row >> np.uint64(32)) & np.uint64(0xFFFF), np.full(n, int(sweep), dtype=np.uint64),
         np.full(n, (P_PROBIT << 24) | ent, dtype=np.uint64)]
    o = _philox4x32_10(c, int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    x = (o[1] << np.uint64(32)) | o[0]
    return ((x >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53


def udot(ids, S):
    """sum over the latent dimension of the product of the modes' factor rows; ids 1-based (n, n_modes), S[k]: (N_k, D)"""
    ids = np.asarray(ids, dtype=np.int64)
    p = S[0][ids[:, 0] - 1].copy()
    for k in range(1, len(S)):
        p = p * S[k][ids[:, k] - 1]
    return p.sum(axis=1)


def run_chain(ids, values, dims, D, seed, iters, feats=None, use_ff=True, rel_tag=1, test_ids=None, burnin=0):
    """macau() on ONE probit relation (ids (n, n_modes) 1-based, values 0/1) between len(dims) entities, entity k with the dense
    side information feats[k] (or None): iterations 1 .. iters.  Returns {"S", "mu", "Lam", "beta", "lb", "z"} after the last
    one and, with test_ids, "prob": the mean over iterations burnin + 1 .. iters of Phi(udot) on those cells."""
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
    prob, z = None, None
    for it in range(1, iters + 1):
        # z | U, V from the previous iteration's rows; the rows then see y - base = z with alpha = 1
        z = draw_z(udot(ids, S), values, uniforms(seed, it, rel_tag, len(values)))
        linear = values - z
        for j in range(n_modes):
            facs = [None if k == j else S[k] for k in range(n_modes)]
            term = O.Term(ids, values, list(dims), j, 1.0, 0.0, facs, linear_values=linear, index=index)
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
            p = ndtr(udot(test_ids, S))
            prob = p if prob is None else prob + p
    out = {"S": S, "mu": mu, "Lam": Lam, "beta": beta, "lb": lb, "z": z}
    if prob is not None:
        out["prob"] = prob / (iters - burnin)
    return out


def planted(seed=0, N1=300, N2=200, rank=4, n_cells=12000, n_test=3000):
    """planted probit data: distinct cells of an N1 x N2 matrix, labels 1[u*.v* + eps > 0], the last n_test cells held out"""
    rng = np.random.default_rng(seed)
    cells = rng.choice(N1 * N2, size=n_cells, replace=False)
    ids = np.stack([cells // N2 + 1, cells % N2 + 1], axis=1).astype(np.int64)
    U, V = rng.standard_normal((N1, rank)), rng.standard_normal((N2, rank))
    y = ((U[ids[:, 0] - 1] * V[ids[:, 1] - 1]).sum(axis=1) + rng.standard_normal(n_cells) > 0).astype(np.float64)
    return ids, y, n_test


def iteration_case(n_modes, with_feat):
    """the small relation of the whole-iteration test: (ids, values, dims, D, feats per entity, number of leading test cells);
    cells drawn with replacement, so some repeat"""
    rng = np.random.default_rng(20 + n_modes)
    dims = [40, 30, 12][:n_modes]
    n, D, n_test = 900, 8, 100
    ids = np.stack([rng.integers(1, d + 1, n) for d in dims], axis=1).astype(np.int64)
    for k, d in enumerate(dims):
        ids[:d, k] = np.arange(1, d + 1)                  # every id occurs: the entities have exactly dims rows
    y = (rng.random(n) < 0.45).astype(np.float64)
    feats = [None] * n_modes
    if with_feat:
        feats[0] = rng.standard_normal((dims[0], 5))
    return ids, y, dims, D, feats, n_test
