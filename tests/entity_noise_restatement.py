"""A numpy restatement of the per-row noise model (setEntityNoise) for its tests.

A cell whose id in the noise entity's mode is j is observed with precision alpha tau_j, tau_j ~ Gamma(shape, rate) a priori.
`gamma_variates(seed, sweep, rel_tag, rows, a)` is Marsaglia-Tsang on the two streams bdf_entity_noise_draw documents (include/bdf.h:
purposes 19 / 20, entity 0x800000 | rel_tag, row = the noise entity's 0-based row, pair = attempt; a shape below 1 goes through the
boost u^(1/a) of the variate of a + 1, u the uniform of pair 0xffff), on robust_restatement's vectorised Philox blocks, with a shape
per row; `gamma_mt` the same one variate at a time on oracle.draw and oracle.normals.  `draw_tau` is the conditional draw, `taus`
the whole of bdf_entity_noise_draw from the residuals, and `run_chain(...)` whole macau() iterations in the library's order -- tau |
U,V,alpha(previous) -> alpha | U,V,tau -> rows, hyperprior of every entity in turn -> beta of every entity with features -- on
robust_restatement.sample_rows (the weighted row system with omega_k = tau of the cell's row) and the oracle's hyperprior, beta and
alpha, with the held-out log predictive density of every draw (lpd_restatement) under alpha tau of the cell's row.  `planted(seed)`
is the data of the issue's experiment.
"""
import numpy as np

from oracle import oracle as O
import lpd_restatement as LR
import robust_restatement as RR
from probit_restatement import udot

P_NOISE_N, P_NOISE_U = 19, 20
BOOST_PAIR = 0xFFFF


def _u01(lo, hi):
    x = (int(hi) << 32) | int(lo)
    return ((x >> 11) + 0.5) * 2.0 ** -53


def gamma_mt(seed, sweep, rel_tag, row, a):
    """Gamma(a, 1) for row `row`: attempt t takes normal 2 t of (P_NOISE_N, entity, row) and the uniform of (P_NOISE_U, entity, row,
    pair t); a < 1: the variate of a + 1 times u^(1 / a), u the uniform of pair 0xffff"""
    ent = RR._entity(rel_tag)
    boost = 1.0
    if a < 1.0:
        o = O.draw(seed, sweep, P_NOISE_U, ent, row, BOOST_PAIR)
        boost = _u01(o[0], o[1]) ** (1.0 / a)
        a += 1.0
    d = a - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    for t in range(256):
        x = float(O.normals(seed, sweep, P_NOISE_N, ent, row, 2 * t + 1)[2 * t])
        v = 1.0 + c * x
        if v <= 0.0:
            continue
        v = v * v * v
        o = O.draw(seed, sweep, P_NOISE_U, ent, row, t)
        u = _u01(o[0], o[1])
        if u < 1.0 - 0.0331 * (x * x) * (x * x):
            return boost * d * v
        if np.log(u) < 0.5 * x * x + d * (1.0 - v + np.log(v)):
            return boost * d * v
    return boost * d


def gamma_variates(seed, sweep, rel_tag, rows, a):
    """gamma_mt for every (sweep[i], rows[i], a[i]) at once (sweep and a: scalars or arrays as long as rows)"""
    rows = np.asarray(rows, dtype=np.uint64)
    sweep = np.broadcast_to(np.asarray(sweep, dtype=np.uint64), rows.shape)
    a = np.array(np.broadcast_to(np.asarray(a, dtype=np.float64), rows.shape))
    ent = RR._entity(rel_tag)
    boost = np.ones(len(rows))
    low = a < 1.0
    if low.any():
        u, _ = RR._blocks(seed, sweep[low], P_NOISE_U, ent, rows[low], BOOST_PAIR)
        boost[low] = u ** (1.0 / a[low])
        a[low] += 1.0
    d = a - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    out = boost * d
    todo = np.arange(len(rows))
    for t in range(256):
        if len(todo) == 0:
            break
        u1, u2 = RR._blocks(seed, sweep[todo], P_NOISE_N, ent, rows[todo], t)
        x = np.sqrt(-2.0 * np.log(u1)) * np.cos(RR.TWO_PI * u2)
        dd = d[todo]
        v = 1.0 + c[todo] * x
        ok = v > 0.0
        v = np.where(ok, v, 1.0) ** 3
        u, _ = RR._blocks(seed, sweep[todo], P_NOISE_U, ent, rows[todo], t)
        acc = ok & ((u < 1.0 - 0.0331 * (x * x) * (x * x)) | (np.log(u) < 0.5 * x * x + dd * (1.0 - v + np.log(v))))
        out[todo[acc]] = boost[todo[acc]] * dd[acc] * v[acc]
        todo = todo[~acc]
    return out


def draw_tau(G, S, alpha, rate):
    """tau_j | U, V, alpha ~ Gamma(shape + n_j / 2, rate + alpha S_j / 2) from G ~ Gamma(shape + n_j / 2, 1)"""
    return np.asarray(G, dtype=np.float64) / (rate + 0.5 * (alpha * np.asarray(S, dtype=np.float64)))


def row_sums(rows0, N, sq):
    """(n_j, S_j) of every row 0 .. N-1: the cells of each row and the sum of `sq` over them"""
    rows0 = np.asarray(rows0, dtype=np.int64)
    return np.bincount(rows0, minlength=N), np.bincount(rows0, weights=np.asarray(sq, dtype=np.float64), minlength=N)


def taus(seed, sweep, rel_tag, rows0, N, e, alpha, shape, rate):
    """the draw of bdf_entity_noise_draw for the residuals e of cells whose 0-based row in the noise entity is rows0:
    (tau per row, tau of its row per cell, sum_j tau_j S_j, S)"""
    e = np.asarray(e, dtype=np.float64)
    n, S = row_sums(rows0, N, e * e)
    tau = draw_tau(gamma_variates(seed, sweep, rel_tag, np.arange(N), shape + 0.5 * n), S, alpha, rate)
    return tau, tau[np.asarray(rows0, dtype=np.int64)], float(np.sum(tau * S)), S


# ---- whole iterations --------------------------------------------------------------------------------------------------------
def run_chain(ids, values, dims, D, seed, iters, mode=None, shape=2.0, rate=2.0, alpha=1.0, alpha_sample=False, feats=None, use_ff=True,
              rel_tag=1, test_ids=None, test_values=None, burnin=0, alpha_lambda0=1.0, alpha_nu0=2.0):
    """macau() on ONE relation (ids (n, n_modes) 1-based) between len(dims) entities, entity k with the dense side information
    feats[k] (or None).  mode (0-based) given: the rows of that entity carry tau_j ~ Gamma(shape, rate); None: the Gaussian chain on
    the same row sampler.  Iterations 1 .. iters.  Returns {"S", "mu", "Lam", "beta", "lb", "alpha", "mean", "tau"} after the last
    one, "tau_mean" (the mean of tau over iterations burnin + 1 .. iters) and, with test_ids, "pred": the mean over the same
    iterations of udot + mean on those cells; with test_values too, "lpd" (per test cell), "LPD" (its mean): the streaming
    log-sum-exp of every draw's Gaussian log density under alpha tau of the cell's row, phases as macau(lpd=True) takes them."""
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
    N = dims[mode] if mode is not None else 1
    tau, omega = np.ones(N), np.ones(len(values))
    pred, tau_sum, stream = None, np.zeros(N), LR.Stream()
    for it in range(1, iters + 1):
        e = values - (udot(ids, S) + mean)
        if mode is not None:               # tau | U, V and the previous iteration's alpha
            tau, omega, wsse, _ = taus(seed, it, rel_tag, ids[:, mode] - 1, N, e, alpha, shape, rate)
        else:
            wsse = float(np.sum(e * e))
        if alpha_sample:                   # alpha | U, V, tau
            alpha = O.sample_alpha(alpha_lambda0, alpha_nu0, len(values), wsse, seed, it, rel_tag)
        for j in range(n_modes):
            if ofe[j] is not None:
                uhat = np.stack([ofe[j].mul(beta[j][:, d]) for d in range(D)], axis=1)
                S[j] = RR.sample_rows(ids, values, omega, dims, j, alpha, mean, S, mu[j] + uhat, Lam[j], seed, it, j + 1)
                U, nuh, Tinv = S[j] - uhat, D + ofe[j].n, np.eye(D) + beta[j].T @ beta[j] * lb[j]
            else:
                S[j] = RR.sample_rows(ids, values, omega, dims, j, alpha, mean, S, mu[j], Lam[j], seed, it, j + 1)
                U, nuh, Tinv = S[j], float(D), np.eye(D)
            mu_N, beta_N, T_N, nu_N = O.hyper_params(U, np.zeros(D), 2.0, Tinv, nuh)
            mu[j], Lam[j] = O.hyper_draw(mu_N, beta_N, T_N, nu_N, seed, it, j + 1)
        for j in range(n_modes):
            if ofe[j] is not None:
                beta[j], _, _ = O.sample_beta(ofe[j], S[j], mu[j], Lam[j], lb[j], use_ff, None, seed, it, j + 1)
                lb[j] = O.sample_lambda_beta(beta[j], Lam[j], 1e-3, 1.0, seed, it, j + 1)
        if test_ids is not None:
            p = udot(test_ids, S) + mean
            if test_values is not None:
                a_cell = alpha * (tau[np.asarray(test_ids)[:, mode] - 1] if mode is not None else 1.0)
                stream.update(LR.cell_loglik(test_values, p, a_cell), 0 if it <= burnin else (1 if it == burnin + 1 else 2))
            if it > burnin:
                pred = p if pred is None else pred + p
        if it > burnin:
            tau_sum += tau
    out = {"S": S, "mu": mu, "Lam": Lam, "beta": beta, "lb": lb, "alpha": alpha, "mean": mean, "tau": tau,
           "tau_mean": tau_sum / max(iters - burnin, 1)}
    if pred is not None:
        out["pred"] = pred / (iters - burnin)
    if test_values is not None and iters > burnin:
        out["lpd"] = stream.lpd()
        out["LPD"] = float(np.mean(out["lpd"]))
    return out


def planted(seed=0, N1=150, N2=100, rank=3, n_train=4500, n_test=1500, sd_lo=0.1, sd_hi=3.0):
    """planted column noise: distinct cells of an N1 x N2 matrix, clean = u*.v*; column c has noise sd_c, log-uniform in [sd_lo,
    sd_hi]; a training cell is clean + sd_c eps; the LAST n_test cells are held out and keep their clean values (they are scored
    against those).  Returns (ids, y, sd per column, n_test, alpha = 1 / mean(sd^2))"""
    rng = np.random.default_rng(seed)
    n_cells = n_train + n_test
    cells = rng.choice(N1 * N2, size=n_cells, replace=False)
    ids = np.stack([cells // N2 + 1, cells % N2 + 1], axis=1).astype(np.int64)
    U, V = rng.standard_normal((N1, rank)), rng.standard_normal((N2, rank))
    clean = (U[ids[:, 0] - 1] * V[ids[:, 1] - 1]).sum(axis=1)
    sd = np.exp(rng.uniform(np.log(sd_lo), np.log(sd_hi), N2))
    train = np.arange(n_cells) < n_train
    y = np.where(train, clean + sd[ids[:, 1] - 1] * rng.standard_normal(n_cells), clean)
    return ids, y, sd, n_test, float(1.0 / np.mean(sd ** 2))


def quality(pred_noise, pred_gauss, clean, tau_mean, sd):
    """(r, c) of the planted experiment: r = RMSE(noise) / RMSE(Gaussian) against the clean held-out values, c = the correlation
    between the log posterior-mean precision and the log planted precision 1 / sd^2"""
    rmse = lambda p: float(np.sqrt(np.mean((np.asarray(p) - clean) ** 2)))
    return rmse(pred_noise) / rmse(pred_gauss), float(np.corrcoef(np.log(tau_mean), -2.0 * np.log(sd))[0, 1])


def iteration_case(n_modes, with_feat, alpha_sample):
    """the small relation of the whole-iteration test: (ids, values, dims, D, feats per entity, number of leading test cells, alpha,
    alpha_sample, the noise entity's 0-based mode); cells drawn with replacement, so some repeat; the noise entity's rows have
    noise sd between 0.2 and 3"""
    rng = np.random.default_rng(170 + n_modes)
    dims = [40, 30, 12][:n_modes]
    n, D, n_test = 900, 8, 100
    mode = n_modes - 1
    ids = np.stack([rng.integers(1, d + 1, n) for d in dims], axis=1).astype(np.int64)
    for k, d in enumerate(dims):
        ids[:d, k] = np.arange(1, d + 1)                  # every id occurs: the entities have exactly dims rows
    sd = np.exp(rng.uniform(np.log(0.2), np.log(3.0), dims[mode]))
    y = sd[ids[:, mode] - 1] * rng.standard_normal(n)
    feats = [None] * n_modes
    if with_feat:
        feats[0] = rng.standard_normal((dims[0], 5))
    return ids, y, dims, D, feats, n_test, 2.5, bool(alpha_sample), mode
