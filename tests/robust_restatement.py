"""A numpy restatement of the robust (Student-t) noise model and of observation weights for the robust tests.

`gamma_mt(seed, sweep, rel_tag, row, a)` is Marsaglia-Tsang on the two streams bdf_robust_draw documents (include/bdf.h: purposes
16 / 17, entity 0x800000 | rel_tag, row = observation, pair = attempt), one variate at a time on oracle.draw and oracle.normals;
`gamma_variates` the same for many (sweep, row) at once on the vectorised Philox of probit_restatement (held against gamma_mt in
test_robust_host.py).  `draw_omega` is the conditional draw, `row_system` / `sample_row` / `sample_rows` the weighted row system in
numpy (any number of modes; `row_system_terms`: several relations sharing the sampled entity, weighted or not) and the reference's map from the row's normals to the sample (chol(inv(P))' z + inv(P) b), and `run_chain(...)` whole macau()
iterations in the library's order -- omega | U,V,alpha -> alpha | U,V,omega -> rows, hyperprior of every entity in turn -> beta of
every entity with features -- with the hyperprior, beta and alpha taken from the oracle.
"""
import numpy as np

from oracle import oracle as O
from probit_restatement import _philox4x32_10, udot

P_ROW = 1
P_ROBUST_N, P_ROBUST_U = 16, 17
TWO_PI = 6.283185307179586476925286766559


def _entity(rel_tag):
    return (0x800000 | int(rel_tag)) & 0xFFFFFF


def _u01(lo, hi):
    x = (int(hi) << 32) | int(lo)
    return ((x >> 11) + 0.5) * 2.0 ** -53


def gamma_mt(seed, sweep, rel_tag, row, a):
    """Gamma(a, 1), a >= 1, for observation `row`: attempt t takes normal 2 t of (P_ROBUST_N, entity, row) and the uniform of
    (P_ROBUST_U, entity, row, pair t)"""
    assert a >= 1.0
    ent = _entity(rel_tag)
    d = a - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    for t in range(256):
        x = float(O.normals(seed, sweep, P_ROBUST_N, ent, row, 2 * t + 1)[2 * t])
        v = 1.0 + c * x
        if v <= 0.0:
            continue
        v = v * v * v
        o = O.draw(seed, sweep, P_ROBUST_U, ent, row, t)
        u = _u01(o[0], o[1])
        if u < 1.0 - 0.0331 * (x * x) * (x * x):
            return d * v
        if np.log(u) < 0.5 * x * x + d * (1.0 - v + np.log(v)):
            return d * v
    return d


def _blocks(seed, sweep, purpose, ent, row, pair):
    n = len(row)
    c = [row & np.uint64(0xFFFFFFFF), ((row >> np.uint64(32)) & np.uint64(0xFFFF)) | (np.uint64(pair) << np.uint64(16)), sweep,
         np.full(n, (purpose << 24) | ent, dtype=np.uint64)]
    o = _philox4x32_10(c, int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    u1 = (((o[1] << np.uint64(32)) | o[0]) >> np.uint64(11)).astype(np.float64)
    u2 = (((o[3] << np.uint64(32)) | o[2]) >> np.uint64(11)).astype(np.float64)
    return (u1 + 0.5) * 2.0 ** -53, (u2 + 0.5) * 2.0 ** -53


def gamma_variates(seed, sweep, rel_tag, rows, a):
    """gamma_mt for every (sweep[i], rows[i]) at once (sweep: a scalar or an array as long as rows)"""
    assert a >= 1.0
    rows = np.asarray(rows, dtype=np.uint64)
    sweep = np.broadcast_to(np.asarray(sweep, dtype=np.uint64), rows.shape)
    ent = _entity(rel_tag)
    d = a - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    out = np.full(len(rows), d)
    todo = np.arange(len(rows))
    for t in range(256):
        if len(todo) == 0:
            break
        u1, u2 = _blocks(seed, sweep[todo], P_ROBUST_N, ent, rows[todo], t)
        x = np.sqrt(-2.0 * np.log(u1)) * np.cos(TWO_PI * u2)
        v = 1.0 + c * x
        ok = v > 0.0
        v = np.where(ok, v, 1.0) ** 3
        u, _ = _blocks(seed, sweep[todo], P_ROBUST_U, ent, rows[todo], t)
        acc = ok & ((u < 1.0 - 0.0331 * (x * x) * (x * x)) | (np.log(u) < 0.5 * x * x + d * (1.0 - v + np.log(v))))
        out[todo[acc]] = d * v[acc]
        todo = todo[~acc]
    return out


def draw_omega(e, alpha, nu, G):
    """omega | e ~ Gamma((nu + 1) / 2, rate (nu + alpha e^2) / 2) from G ~ Gamma((nu + 1) / 2, 1)"""
    e = np.asarray(e, dtype=np.float64)
    return 2.0 * np.asarray(G, dtype=np.float64) / (nu + alpha * (e * e))


def omegas(seed, sweep, rel_tag, e, alpha, nu):
    """the draw of bdf_robust_draw for the residuals e of observations 0 .. n-1, and sum omega e^2"""
    e = np.asarray(e, dtype=np.float64)
    w = draw_omega(e, alpha, nu, gamma_variates(seed, sweep, rel_tag, np.arange(len(e)), 0.5 * (nu + 1.0)))
    return w, float(np.sum(w * e * e))


# ---- the weighted row system -------------------------------------------------------------------------------------------------
def row_system(ids, values, weights, mode, row, alpha, base, S, mu_i, Lam):
    """P = Lam + alpha sum omega w w', b = Lam mu_i + alpha sum omega (y - base) w over the observations of `row` (0-based) of
    `mode`; w: the Hadamard product of the other modes' factor rows; base: a scalar or one value per observation"""
    ids = np.asarray(ids, dtype=np.int64)
    sel = np.nonzero(ids[:, mode] == row + 1)[0]
    D = len(mu_i)
    w = np.ones((len(sel), D))
    for k in range(ids.shape[1]):
        if k != mode:
            w = w * S[k][ids[sel, k] - 1]
    om = np.asarray(weights, dtype=np.float64)[sel]
    res = np.asarray(values, dtype=np.float64)[sel] - np.broadcast_to(np.asarray(base, dtype=np.float64), (len(values),))[sel]
    P = Lam + alpha * (w * om[:, None]).T @ w
    b = Lam @ mu_i + alpha * (w.T @ (om * res))
    return P, b


def row_system_terms(terms, row, mu_i, Lam):
    """the row system of an entity that several relations share: P = Lam + sum_t alpha_t sum_k omega_k w w', b = Lam mu_i +
    sum_t alpha_t sum_k omega_k (y - base) w; terms: one (ids, values, weights, mode, alpha, base, S) per relation, weights None
    for a relation without them (omega = 1), the rest as row_system takes them (held against the oracle in test_robust_host.py)"""
    D = len(mu_i)
    P, b = np.array(Lam, dtype=np.float64), Lam @ mu_i
    for ids, values, weights, mode, alpha, base, S in terms:
        om = np.ones(len(values)) if weights is None else weights
        Pt, bt = row_system(ids, values, om, mode, row, alpha, base, S, np.zeros(D), np.zeros((D, D)))
        P, b = P + Pt, b + bt
    return P, b


def sample_row(P, b, z):
    """the reference's map (src/sampling.jl:200-212): covar = inv(P), x = chol(covar)' z + covar b (chol upper: its transpose is
    the lower factor)"""
    covar = np.linalg.inv(P)
    covar = 0.5 * (covar + covar.T)
    return np.linalg.cholesky(covar) @ z + covar @ b


def sample_rows(ids, values, weights, dims, mode, alpha, base, S, mu, Lam, seed, sweep, entity_tag):
    """every row of entity `mode`; mu: (D) or (N, D); normals of stream (P_ROW, entity_tag, row)"""
    D = Lam.shape[0]
    out = np.zeros((dims[mode], D))
    for row in range(dims[mode]):
        mu_i = mu[row] if np.ndim(mu) == 2 else mu
        P, b = row_system(ids, values, weights, mode, row, alpha, base, S, mu_i, Lam)
        out[row] = sample_row(P, b, O.normals(seed, sweep, P_ROW, entity_tag, row, D))
    return out


# ---- whole iterations --------------------------------------------------------------------------------------------------------
def run_chain(ids, values, dims, D, seed, iters, alpha=1.0, alpha_sample=False, nu=None, weights=None, feats=None, use_ff=True,
              rel_tag=1, test_ids=None, burnin=0, alpha_lambda0=1.0, alpha_nu0=2.0):
    """macau() on ONE relation (ids (n, n_modes) 1-based) between len(dims) entities, entity k with the dense side information
    feats[k] (or None): nu given: the Student-t model; weights given: known weights; neither: the Gaussian chain on the same row
    sampler.  Iterations 1 .. iters.  Returns {"S", "mu", "Lam", "beta", "lb", "alpha", "mean", "omega"} after the last one,
    "omega_mean" (the mean of omega over iterations burnin + 1 .. iters) and, with test_ids, "pred": the mean over the same
    iterations of udot + mean on those cells."""
    assert nu is None or weights is None
    n_modes = len(dims)
    feats = feats or [None] * n_modes
    S = [np.zeros((n, D)) for n in dims]
    mu = [np.zeros(D) for _ in dims]
    Lam = [5.0 * np.eye(D) for _ in dims]
    ofe = [None if F is None else O.Feat.from_dense(np.asarray(F, dtype=np.float64)) for F in feats]
    beta = [None if f is None else np.zeros((f.n, D)) for f in ofe]
    lb = [1.0] * n_modes
    ids = np.asarray(ids, dtype=np.int64)
    values = np.asarray(values, dtype=np.float64)
    mean = float(np.mean(values))
    alpha = float(alpha)
    omega = np.ones(len(values)) if weights is None else np.asarray(weights, dtype=np.float64)
    pred, omega_sum = None, np.zeros(len(values))
    for it in range(1, iters + 1):
        e = (values - mean) - udot(ids, S)
        if nu is not None:                 # omega | U, V and the previous iteration's alpha
            omega, wsse = omegas(seed, it, rel_tag, e, alpha, nu)
        else:
            wsse = float(np.sum(omega * e * e))
        if alpha_sample:                   # alpha | U, V, omega
            alpha = O.sample_alpha(alpha_lambda0, alpha_nu0, len(values), wsse, seed, it, rel_tag)
        for j in range(n_modes):
            if ofe[j] is not None:
                uhat = np.stack([ofe[j].mul(beta[j][:, d]) for d in range(D)], axis=1)
                S[j] = sample_rows(ids, values, omega, dims, j, alpha, mean, S, mu[j] + uhat, Lam[j], seed, it, j + 1)
                U, nuh, Tinv = S[j] - uhat, D + ofe[j].n, np.eye(D) + beta[j].T @ beta[j] * lb[j]
            else:
                S[j] = sample_rows(ids, values, omega, dims, j, alpha, mean, S, mu[j], Lam[j], seed, it, j + 1)
                U, nuh, Tinv = S[j], float(D), np.eye(D)
            mu_N, beta_N, T_N, nu_N = O.hyper_params(U, np.zeros(D), 2.0, Tinv, nuh)
            mu[j], Lam[j] = O.hyper_draw(mu_N, beta_N, T_N, nu_N, seed, it, j + 1)
        for j in range(n_modes):
            if ofe[j] is not None:
                beta[j], _, _ = O.sample_beta(ofe[j], S[j], mu[j], Lam[j], lb[j], use_ff, None, seed, it, j + 1)
                lb[j] = O.sample_lambda_beta(beta[j], Lam[j], 1e-3, 1.0, seed, it, j + 1)
        if it > burnin:
            omega_sum += omega
            if test_ids is not None:
                p = udot(test_ids, S) + mean
                pred = p if pred is None else pred + p
    out = {"S": S, "mu": mu, "Lam": Lam, "beta": beta, "lb": lb, "alpha": alpha, "mean": mean, "omega": omega,
           "omega_mean": omega_sum / max(iters - burnin, 1)}
    if pred is not None:
        out["pred"] = pred / (iters - burnin)
    return out


def planted(seed=0, N1=150, N2=100, rank=3, n_cells=5000, n_test=1500, sd=0.3, share=0.10, scale=5.0):
    """planted outliers: distinct cells of an N1 x N2 matrix, clean = u*.v*; the LAST n_test cells are held out and keep their
    clean values (they are scored against those); a training cell is clean + sd eps, and a `share` of them get an extra
    N(0, scale^2).  Returns (ids, y, extra (0 where none, and on the held-out cells), n_test)"""
    rng = np.random.default_rng(seed)
    cells = rng.choice(N1 * N2, size=n_cells, replace=False)
    ids = np.stack([cells // N2 + 1, cells % N2 + 1], axis=1).astype(np.int64)
    U, V = rng.standard_normal((N1, rank)), rng.standard_normal((N2, rank))
    clean = (U[ids[:, 0] - 1] * V[ids[:, 1] - 1]).sum(axis=1)
    train = np.arange(n_cells) < n_cells - n_test
    extra = np.where(train & (rng.random(n_cells) < share), scale * rng.standard_normal(n_cells), 0.0)
    y = np.where(train, clean + sd * rng.standard_normal(n_cells) + extra, clean)
    return ids, y, extra, n_test


def iteration_case(n_modes, with_feat, alpha_sample):
    """the small relation of the whole-iteration test: (ids, values, dims, D, feats per entity, number of leading test cells,
    alpha, alpha_sample, weights of the training cells for the setWeights cases); cells drawn with replacement, so some repeat;
    about 8 % of the values are gross outliers"""
    rng = np.random.default_rng(70 + n_modes)
    dims = [40, 30, 12][:n_modes]
    n, D, n_test = 900, 8, 100
    ids = np.stack([rng.integers(1, d + 1, n) for d in dims], axis=1).astype(np.int64)
    for k, d in enumerate(dims):
        ids[:d, k] = np.arange(1, d + 1)                  # every id occurs: the entities have exactly dims rows
    y = rng.standard_normal(n) + np.where(rng.random(n) < 0.08, 6.0 * rng.standard_normal(n), 0.0)
    feats = [None] * n_modes
    if with_feat:
        feats[0] = rng.standard_normal((dims[0], 5))
    weights = np.exp(rng.uniform(np.log(0.05), np.log(20.0), n - n_test))
    return ids, y, dims, D, feats, n_test, 2.5, bool(alpha_sample), weights
