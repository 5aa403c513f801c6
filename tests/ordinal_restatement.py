"""A numpy restatement of the ordinal probit noise model for the ordinal tests.

`theta`, `propose` and `adapt` are the maps of csrc/ordinal.h in the form the header states them (the same loops in the same
order), `normals` / `uniform` the numbers the step takes from the library's Philox streams (purpose 15, entity 0x800000 | rel_tag:
row 0, normal k for the proposal; row 1, pair 0 for the decision), `step` one Metropolis step on the edges as bdf_ordinal_step
documents it (include/bdf.h) with the log mass of lpd_restatement, and `run_chain` whole macau() iterations on an ordinal relation:
the chain of interval_restatement.run_chain in its order, with the step between alpha and the latent draw -- alpha | U,V,z ->
edges | U,V,alpha -> z | U,V,alpha,edges -> rows, hyperprior of every entity in turn -> beta -- and the scoring of lpd_restatement
on held-out levels under every draw's edges.  Every decision's margin |log u - S| is appended to MARGINS.
"""
import math

import numpy as np

import interval_restatement as IR
import lpd_restatement as LR
from oracle import oracle as O
from probit_restatement import _philox4x32_10, udot

P_ORDINAL = 15
MIN_GAP = 1e-6
MARGINS = []                      # |log u - S| of every decision taken so far (a refused proposal: inf)


def _block(seed, sweep, rel_tag, row, pair):
    ent = (0x800000 | int(rel_tag)) & 0xFFFFFF
    pair = np.atleast_1d(np.asarray(pair, dtype=np.uint64))
    n = len(pair)
    c = [np.full(n, int(row) & 0xFFFFFFFF, dtype=np.uint64), np.uint64((int(row) >> 32) & 0xFFFF) | (pair << np.uint64(16)),
         np.full(n, int(sweep), dtype=np.uint64), np.full(n, (P_ORDINAL << 24) | ent, dtype=np.uint64)]
    return _philox4x32_10(c, int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)


def _u01(lo, hi):
    x = (hi << np.uint64(32)) | lo
    return ((x >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53


def normals(seed, sweep, rel_tag, count):
    """normals 0 .. count-1 of stream (P_ORDINAL, 0x800000 | rel_tag, row 0): normal k is element k % 2 of the Box-Muller pair of
    block k // 2 (u1 from the block's first two words, u2 from its last two; r cos(2 pi u2), r sin(2 pi u2), r = sqrt(-2 log u1))"""
    k = np.arange(count)
    o = _block(seed, sweep, rel_tag, 0, k // 2)
    u1, u2 = _u01(o[0], o[1]), _u01(o[2], o[3])
    r = np.sqrt(-2.0 * np.log(u1))
    return np.where(k % 2 == 1, r * np.sin(2.0 * np.pi * u2), r * np.cos(2.0 * np.pi * u2))


def uniform(seed, sweep, rel_tag):
    """the decision's uniform: the first double of block (P_ORDINAL, 0x800000 | rel_tag, row 1, pair 0)"""
    o = _block(seed, sweep, rel_tag, 1, 0)
    return float(_u01(o[0], o[1])[0])


def start_edges(K):
    """the full table e_0 .. e_K at the chain's start: -inf, 1.5, 2.5, ..., K - 1/2, +inf"""
    return np.concatenate([[-np.inf], np.arange(1, K) + 0.5, [np.inf]])


def theta(e):
    """theta_k = log(g_k / g_{K-2}), k = 1 .. K-3, of the full table e (K + 1 entries)"""
    K = len(e) - 1
    return np.array([math.log((e[k + 1] - e[k]) / (e[K - 1] - e[K - 2])) for k in range(1, K - 2)])


def gaps_from_theta(th, R):
    """the K - 2 gaps of the additive log-ratio coordinates th (K - 3 of them) with sum R"""
    w = np.concatenate([np.exp(th), [1.0]])
    return R * w / w.sum()


def propose(e, sigma, eps):
    """(proposed full table, log Jacobian term, every gap above MIN_GAP) -- bdf_ordinal_propose, loop for loop"""
    K = len(e) - 1
    R = e[K - 1] - e[1]
    th = theta(e)
    sw = 0.0
    for k in range(1, K - 2):
        sw += math.exp(th[k - 1] + sigma * eps[k - 1])
    sw += 1.0
    out = np.array(e, dtype=np.float64)
    ok, acc, lj = True, e[1], 0.0
    for k in range(1, K - 1):
        w = math.exp(th[k - 1] + sigma * eps[k - 1]) if k <= K - 3 else 1.0
        g = R * w / sw
        ok = ok and (g > MIN_GAP)
        lj += (math.log(g) if g > 0.0 else -math.inf) - math.log(e[k + 1] - e[k])
        acc += g
        if k <= K - 3:
            out[k + 1] = acc
    return out, lj, bool(ok)


def adapt(sigma, accepted, i):
    """the step size after the i-th step (i >= 1) of the burn-in"""
    return min(max(math.exp(math.log(sigma) + ((1.0 if accepted else 0.0) - 0.3) / math.sqrt(i)), 1e-8), 10.0)


def mass_terms(m, codes, e, prop, alpha):
    """per cell: log mass of its level's bin under `prop` minus that under `e`; exactly 0 where neither edge moved"""
    K = len(e) - 1
    c = np.asarray(codes, dtype=np.int64)
    moved = (c > 1) & (c < K) & ((e[c - 1] != prop[c - 1]) | (e[c] != prop[c]))
    out = np.zeros(len(c))
    if moved.any():
        mm, cc = np.asarray(m, dtype=np.float64)[moved], c[moved]
        out[moved] = LR.lpd_mass(mm, prop[cc - 1], prop[cc], alpha) - LR.lpd_mass(mm, e[cc - 1], e[cc], alpha)
    return out


class State:
    """the edges (full table), the step size and the counters of one ordinal relation"""

    def __init__(self, K, step=0.1):
        self.K, self.e, self.sigma, self.proposals, self.accepts = int(K), start_edges(K), float(step), 0, 0
        self.last = None

    def step(self, m, codes, alpha, seed, sweep, rel_tag, adapting):
        """one Metropolis step given the cells' means m = udot + mean_value; returns and keeps what it did"""
        eps = normals(seed, sweep, rel_tag, self.K - 3)
        prop, jac, ok = propose(self.e, self.sigma, eps)
        S = (math.fsum(mass_terms(m, codes, self.e, prop, alpha)) + jac) if ok else -math.inf
        lu = math.log(uniform(seed, sweep, rel_tag))
        acc = ok and lu < S
        MARGINS.append(abs(lu - S))
        if acc:
            self.e = prop
        self.proposals += 1
        self.accepts += int(acc)
        if adapting:
            self.sigma = adapt(self.sigma, acc, self.proposals)
        self.last = {"prop": prop, "jac": jac, "ok": ok, "S": S, "log_u": lu, "accepted": bool(acc), "eps": eps}
        return self.last


def bounds_of(codes, e):
    """(n, 2): the bin (e_{y-1}, e_y) of every level y under the full table e"""
    c = np.asarray(codes, dtype=np.int64)
    return np.stack([e[c - 1], e[c]], axis=1)


def run_chain(ids, codes, dims, D, seed, burnin, psamples, K, alpha=1.0, alpha_sample=False, feats=None, use_ff=True, rel_tag=1,
              test_ids=None, test_codes=None, step=0.1, sample_edges=True, alpha_lambda0=1.0, alpha_nu0=2.0):
    """macau(lpd=True) on ONE ordinal relation (ids (n, n_modes) 1-based, codes 1 .. K) between len(dims) entities, entity k with the
    dense side information feats[k] (or None): iterations 1 .. burnin + psamples, the step size adapted during the first burnin.
    Returns the state after the last one ({"S", "mu", "Lam", "beta", "lb", "z", "alpha", "mean"}), "edges_trace" (iterations x
    (K - 1)), "sigma", "accepted" (per iteration) and, with test_ids / test_codes, "pred" (the posterior mean of udot + mean), "lpd"
    (per test cell), "LPD" and "loglik" (the last draw's)."""
    n_modes = len(dims)
    feats = feats or [None] * n_modes
    S = [np.zeros((n, D)) for n in dims]
    mu = [np.zeros(D) for _ in dims]
    Lam = [5.0 * np.eye(D) for _ in dims]
    ofe = [None if F is None else O.Feat.from_dense(np.asarray(F, dtype=np.float64)) for F in feats]
    beta = [None if f is None else np.zeros((f.n, D)) for f in ofe]
    lb = [1.0] * n_modes
    index = O.index_build(ids, list(dims))
    values = np.asarray(codes, dtype=np.float64)
    mean = float(np.mean(values))
    z = values.copy()
    linear = np.full(len(values), mean)
    alpha = float(alpha)
    st = State(K, step)
    pred, stream, trace, accepted, loglik = None, LR.Stream(), [], [], None
    for it in range(1, burnin + psamples + 1):
        dot = udot(ids, S)
        if alpha_sample:                 # the residual of the previous z (the values themselves before the first draw)
            sse = float(np.sum((values - (dot + linear)) ** 2))
            alpha = O.sample_alpha(alpha_lambda0, alpha_nu0, len(values), sse, seed, it, rel_tag)
        if sample_edges:                 # the edges | U, V, alpha with z integrated out
            accepted.append(st.step(dot + mean, codes, alpha, seed, it, rel_tag, it <= burnin)["accepted"])
        trace.append(st.e[1:K].copy())
        bounds = bounds_of(codes, st.e)
        z = IR.draw_z(dot + mean, bounds[:, 0], bounds[:, 1], alpha, IR.uniforms(seed, it, rel_tag, len(values)), y=values)
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
        if test_ids is not None:
            p = udot(test_ids, S) + mean
            if it > burnin:
                pred = p if pred is None else pred + p
            if test_codes is not None:
                tb = bounds_of(test_codes, st.e)
                loglik = LR.lpd_mass(p, tb[:, 0], tb[:, 1], alpha)
                stream.update(loglik, 0 if it <= burnin else (1 if it == burnin + 1 else 2))
    out = {"S": S, "mu": mu, "Lam": Lam, "beta": beta, "lb": lb, "z": z, "alpha": alpha, "mean": mean,
           "edges_trace": np.array(trace), "sigma": st.sigma, "accepted": np.array(accepted, dtype=bool)}
    if pred is not None:
        out["pred"] = pred / psamples
    if test_codes is not None and psamples:
        out["lpd"], out["loglik"] = stream.lpd(), loglik
        out["LPD"] = float(np.mean(out["lpd"]))
    return out


PLANTED_EDGES = (1.5, 2.06, 3.66, 4.22, 5.5)


def planted_ordinal(seed=0, N1=300, N2=200, rank=4, n_cells=12000, n_test=3000, edges=PLANTED_EDGES, scale=0.8):
    """planted six-level data with unevenly spaced cutpoints: distinct cells of an N1 x N2 matrix, the latent 3.5 + scale (u*.v* +
    eps / 2) on the scale of the levels (its noise has the precision 1 / (scale / 2)^2 = 6.25), the level the number of `edges`
    at or below it plus one; the last n_test cells are held out, as levels too.  Returns (ids, levels, n_test)"""
    rng = np.random.default_rng(seed)
    cells = rng.choice(N1 * N2, size=n_cells, replace=False)
    ids = np.stack([cells // N2 + 1, cells % N2 + 1], axis=1).astype(np.int64)
    U, V = rng.standard_normal((N1, rank)), rng.standard_normal((N2, rank))
    t = 3.5 + scale * ((U[ids[:, 0] - 1] * V[ids[:, 1] - 1]).sum(axis=1) + 0.5 * rng.standard_normal(n_cells))
    level = np.searchsorted(np.asarray(edges, dtype=np.float64), t, side="right") + 1.0
    return ids, level, n_test


def iteration_case(n_modes, with_feat, alpha_sample):
    """the small relation of the whole-iteration test: (ids, levels 1 .. 5, dims, D, feats per entity, number of leading test cells,
    alpha, alpha_sample); cells drawn with replacement, so some repeat; the levels are a noisy rank-2 signal cut unevenly"""
    rng = np.random.default_rng(160 + n_modes)
    dims = [40, 30, 12][:n_modes]
    n, D, n_test = 900, 8, 100
    ids = np.stack([rng.integers(1, d + 1, n) for d in dims], axis=1).astype(np.int64)
    for k, d in enumerate(dims):
        ids[:d, k] = np.arange(1, d + 1)                  # every id occurs: the entities have exactly dims rows
    F = [rng.standard_normal((d, 2)) for d in dims]
    t = 3.0 + 0.9 * udot(ids, F) / (1.4 ** (n_modes - 2)) + 0.4 * rng.standard_normal(n)
    level = np.searchsorted(np.array([1.5, 1.9, 3.4, 4.5]), t, side="right") + 1.0
    feats = [None] * n_modes
    if with_feat:
        feats[0] = rng.standard_normal((dims[0], 5))
    return ids, level, dims, D, feats, n_test, 2.5, bool(alpha_sample)


ITERATION_CASES = [(n_modes, with_feat, alpha_sample) for n_modes in (2, 3) for with_feat in (0, 1) for alpha_sample in (0, 1)]
ITERATION_SEED = 91


def restated_iterations():
    """the restated chain (2 + 2 iterations, lpd on the held-out levels) of every case of ITERATION_CASES, by case"""
    out = {}
    for n_modes, with_feat, alpha_sample in ITERATION_CASES:
        ids, lev, dims, D, feats, n_test, alpha, _ = iteration_case(n_modes, with_feat, alpha_sample)
        out[(n_modes, with_feat, alpha_sample)] = run_chain(ids[n_test:], lev[n_test:], dims, D, ITERATION_SEED, 2, 2, 5, alpha=alpha, alpha_sample=alpha_sample,
                                                             feats=feats, test_ids=ids[:n_test], test_codes=lev[:n_test])
    return out


# held-out LPD gain of sampled over fixed edges on planted_ordinal() (D = 8, alpha = 6.25, 60 + 60 iterations), seeds 2, 3, 4, as
# this restatement computes it: test_ordinal_host.py holds the record to the computation, test_gpu_ordinal.py the device to the record
PLANTED_GAINS = (0.1174, 0.1127, 0.1219)


def planted_gain(seed, D=8, burnin=60, psamples=60, alpha=6.25):
    ids, lev, n_test = planted_ordinal()
    r = [run_chain(ids[:-n_test], lev[:-n_test], [300, 200], D, seed, burnin, psamples, 6, alpha=alpha, test_ids=ids[-n_test:],
                   test_codes=lev[-n_test:], sample_edges=se)["LPD"] for se in (True, False)]
    return r[0] - r[1]


STEP_N = 1003                     # cells of a step-parity case: no multiple of 8 or 256
STEP_ALPHA = 4.0
STEP_SWEEPS = (5, 6, 7, 8)        # four steps in a row: the first two adapt the step size, the last two do not
STEP_START = 0.3


def step_case(D, n_modes, K):
    """a relation for the step-parity test: (ids 1-based, factors, mean_value, levels); STEP_N cells of a [37, 23, 11] tensor, some
    of them the same cell; the levels are those of udot + mean + noise under unevenly spaced edges, and level K // 2 + 1 is empty
    (its cells are reported one level lower), as are the outer levels the means do not reach when K = 16"""
    rng = np.random.default_rng(3000 + 100 * D + 10 * n_modes + K)
    dims = [37, 23, 11][:n_modes]
    ids = np.stack([rng.integers(1, d + 1, STEP_N) for d in dims], axis=1)
    ids[1::7] = ids[0]
    S = [rng.standard_normal((d, D)) for d in dims]
    S[0] *= (min(K, 8) - 1) / 4.0 / np.std(udot(ids, S))
    mean = (K + 1) / 2.0
    g = rng.uniform(0.3, 1.0, K - 2)
    true = np.concatenate([[1.5], 1.5 + np.cumsum(g * (K - 2.0) / g.sum())])
    codes = np.searchsorted(true, udot(ids, S) + mean + 0.5 * rng.standard_normal(STEP_N), side="right") + 1
    codes[codes == K // 2 + 1] = K // 2
    return ids, S, mean, codes.astype(np.int8), dims


def step_sequence(D, n_modes, K, rel_tag=1, seed=1234):
    """the restated steps of a step-parity case: a list of what State.step returns for the sweeps STEP_SWEEPS, each with the
    state after it ("e", "sigma", "proposals", "accepts")"""
    ids, S, mean, codes, _ = step_case(D, n_modes, K)
    m = udot(ids, S) + mean
    st, out = State(K, STEP_START), []
    for k, sweep in enumerate(STEP_SWEEPS):
        got = dict(st.step(m, codes, STEP_ALPHA, seed, sweep, rel_tag, k < 2))
        got.update(e=st.e.copy(), sigma=st.sigma, proposals=st.proposals, accepts=st.accepts)
        out.append(got)
    return out
