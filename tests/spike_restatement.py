"""A numpy restatement of the spike-and-slab prior of an entity's rows for the spike tests.

    u_id = s_id w_id,  s_id ~ Bernoulli(pi_d),  w_id ~ N(0, 1 / tau_d),  pi_d ~ Beta(incl_a, incl_b),  tau_d ~ Gamma(shape, rate)

`sweep_row` is the row step from (P, c, u_prev, z, U, state): the D-step coordinate sweep over (s_d, w_d) with w_d integrated out
of the inclusion odds; `sweep_rows` the same for many rows at once.  Both also return the near-tie margin, the smallest
|U_d - sigma(lo)| they met: a decision closer than rounding can carry is not one the device has to reproduce.  `hyper_draw` is
the hyper step (Marsaglia-Tsang on the streams 21 / 22 that include/bdf.h documents for bdf_spike_hyper, on oracle.oracle's Philox
and normals).  `run_chain` is whole macau() iterations over several relations in the library's order -- alpha of every relation
that samples it, then rows and hyper step of every entity in turn, then beta of every entity with features -- with the
Normal-Wishart entities' steps as robust_restatement.run_chain restates them (its row_system and sample_row, the oracle's
hyperprior, beta and alpha).
"""
import math

import numpy as np

from oracle import oracle as O
from probit_restatement import udot
import robust_restatement as RR

P_ROW = 1
P_SPIKE_N, P_SPIKE_U, P_SPIKE = 21, 22, 23


def initial_state(D):
    """pi = 1/2, tau = 1 and their logit / log: (4, D)"""
    return np.stack([np.full(D, 0.5), np.ones(D), np.zeros(D), np.zeros(D)])


def sweep_row(P, c, u_prev, z, U, state):
    """one row -> (u, margin).  state: (4, D) rows pi, tau, logit pi, log tau.  For d = 0 .. D-1 in order:
    lambda = P_dd, m = (c_d - sum_{k != d} P_dk u_k) / lambda, lo = logit pi_d + (log tau_d - log lambda) / 2 + lambda m^2 / 2,
    s = [U_d < 1 / (1 + exp(-lo))], u_d = s (m + z_d / sqrt(lambda))"""
    D = len(c)
    u = [float(x) for x in u_prev]
    margin = math.inf
    for d in range(D):
        lam = float(P[d][d])
        m = (float(c[d]) - sum(float(P[d][k]) * u[k] for k in range(D) if k != d)) / lam
        lo = float(state[2][d]) + 0.5 * (float(state[3][d]) - math.log(lam)) + 0.5 * lam * m * m
        p = 1.0 / (1.0 + math.exp(-lo)) if lo > -700.0 else 0.0
        margin = min(margin, abs(float(U[d]) - p))
        u[d] = m + float(z[d]) / math.sqrt(lam) if float(U[d]) < p else 0.0
    return np.array(u), margin


def sweep_rows(P, c, u_prev, z, U, state, dtype=np.float64):
    """the sweep of N independent rows: P (N, D, D), c, u_prev, z, U (N, D) -> (u (N, D) float64, margin)"""
    P, c, z = np.asarray(P, dtype=dtype), np.asarray(c, dtype=dtype), np.asarray(z, dtype=dtype)
    U = np.asarray(U, dtype=np.float64)
    logit, logtau = np.asarray(state[2], dtype=dtype), np.asarray(state[3], dtype=dtype)
    u = np.array(u_prev, dtype=dtype)
    N, D = c.shape
    margin = np.inf
    half = dtype(0.5)
    with np.errstate(over="ignore"):
        for d in range(D):
            lam = P[:, d, d]
            m = (c[:, d] - (np.einsum("nk,nk->n", P[:, d, :], u) - lam * u[:, d])) / lam
            lo = logit[d] + half * (logtau[d] - np.log(lam)) + half * lam * m * m
            p = 1.0 / (1.0 + np.exp(-lo))
            if N:
                margin = min(margin, float(np.min(np.abs(U[:, d] - p.astype(np.float64)))))
            s = U[:, d] < p
            u[:, d] = np.where(s, m + z[:, d] / np.sqrt(lam), dtype(0.0))
    return np.asarray(u, dtype=np.float64) if dtype is np.float64 else u, margin


_u01 = RR._u01


def gamma_on(seed, sweep, entity, g, a):
    """Gamma(a, 1) of variate g of bdf_spike_hyper: attempt t takes normal 2 t of (P_SPIKE_N, entity, g) and the uniform of
    (P_SPIKE_U, entity, g, pair t); a < 1: the variate of a + 1 times u^(1 / a), u the uniform of pair 0xffff"""
    boost = 1.0
    if a < 1.0:
        o = O.draw(seed, sweep, P_SPIKE_U, entity, g, 0xFFFF)
        boost = _u01(o[0], o[1]) ** (1.0 / a)
        a += 1.0
    d = a - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    for t in range(256):
        x = float(O.normals(seed, sweep, P_SPIKE_N, entity, g, 2 * t + 1)[2 * t])
        v = 1.0 + c * x
        if v <= 0.0:
            continue
        v = v * v * v
        o = O.draw(seed, sweep, P_SPIKE_U, entity, g, t)
        uu = _u01(o[0], o[1])
        if uu < 1.0 - 0.0331 * (x * x) * (x * x):
            return boost * d * v
        if np.log(uu) < 0.5 * x * x + d * (1.0 - v + np.log(v)):
            return boost * d * v
    return boost * d


def hyper_draw_nq(n, q, N, incl_a, incl_b, shape, rate, seed, sweep, entity_tag):
    """the hyper step from the counts n_d and the sums of squares q_d -> state (4, D)"""
    D = len(n)
    st = np.zeros((4, D))
    for d in range(D):
        g1 = gamma_on(seed, sweep, entity_tag, 3 * d, incl_a + n[d])
        g2 = gamma_on(seed, sweep, entity_tag, 3 * d + 1, incl_b + (N - n[d]))
        g3 = gamma_on(seed, sweep, entity_tag, 3 * d + 2, shape + 0.5 * n[d])
        tau = g3 / (rate + 0.5 * q[d])
        st[:, d] = g1 / (g1 + g2), tau, np.log(g1) - np.log(g2), np.log(tau)
    return st


def hyper_draw(S, incl_a, incl_b, shape, rate, seed, sweep, entity_tag):
    """the hyper step from the rows S (N, D)"""
    S = np.asarray(S, dtype=np.float64)
    return hyper_draw_nq(np.count_nonzero(S, axis=0), np.sum(S * S, axis=0), S.shape[0], incl_a, incl_b, shape, rate, seed, sweep, entity_tag)


def uniforms(seed, sweep, entity_tag, N, D):
    """U (N, D): bdf_u01 of words x and y of block (P_SPIKE, entity_tag, row, pair d)"""
    rows = np.arange(N, dtype=np.uint64)
    sw = np.full(N, sweep, dtype=np.uint64)
    return np.stack([RR._blocks(seed, sw, P_SPIKE, int(entity_tag) & 0xFFFFFF, rows, d)[0] for d in range(D)], axis=1) if N else np.zeros((0, D))


def normals(seed, sweep, entity_tag, N, D):
    return np.stack([O.normals(seed, sweep, P_ROW, entity_tag, row, D) for row in range(N)]) if N else np.zeros((0, D))


def row_systems(terms, N, D, Lam, mu):
    """P (N, D, D) and b (N, D) of every row of an entity: Lam + sum_t alpha_t sum omega w w' and Lam mu_i + sum_t alpha_t sum
    omega (y - base) w; terms as robust_restatement.row_system_terms takes them (held against it in tests/test_spike_host.py);
    mu: (D) or (N, D)"""
    P = np.broadcast_to(np.asarray(Lam, dtype=np.float64), (N, D, D)).copy()
    b = np.broadcast_to(np.asarray(mu, dtype=np.float64), (N, D)) @ np.asarray(Lam, dtype=np.float64).T
    b = b.copy()
    for ids, values, weights, mode, alpha, base, S in terms:
        ids = np.asarray(ids, dtype=np.int64)
        w = np.ones((len(ids), D))
        for k in range(ids.shape[1]):
            if k != mode:
                w = w * S[k][ids[:, k] - 1]
        om = np.ones(len(ids)) if weights is None else np.asarray(weights, dtype=np.float64)
        res = np.asarray(values, dtype=np.float64) - np.broadcast_to(np.asarray(base, dtype=np.float64), (len(ids),))
        rows = ids[:, mode] - 1
        np.add.at(P, rows, alpha * om[:, None, None] * w[:, :, None] * w[:, None, :])
        np.add.at(b, rows, alpha * (om * res)[:, None] * w)
    return P, b


def run_chain(relations, dims, D, seed, iters, spike, feats=None, burnin=0, test_ids=None, use_ff=True, alpha_lambda0=1.0,
              alpha_nu0=2.0):
    """macau() iterations 1 .. iters.  relations: a list of dicts {"ids" (n, modes) 1-based, "values", "entities" (the entity
    index of every mode), "alpha", "alpha_sample", "weights" (None or per cell)}; dims: rows per entity; spike: {entity index:
    (incl_a, incl_b, shape, rate)}; feats: dense side information per entity or None.  test_ids: cells of relation 0.
    Returns {"S", "mu", "Lam", "state" (per spike entity), "alpha", "mean", "margin", and over iterations burnin + 1 .. iters the
    means "inclusion", "precision", "activity", "row_inclusion" per spike entity and "pred"}"""
    n_ent = len(dims)
    feats = feats or [None] * n_ent
    S = [np.zeros((n, D)) for n in dims]
    mu = [np.zeros(D) for _ in dims]
    Lam = [5.0 * np.eye(D) for _ in dims]
    ofe = [None if F is None else O.Feat.from_dense(np.asarray(F, dtype=np.float64)) for F in feats]
    beta = [None if f is None else np.zeros((f.n, D)) for f in ofe]
    lb = [1.0] * n_ent
    state = {j: initial_state(D) for j in spike}
    acc = {j: {"inclusion": np.zeros(D), "precision": np.zeros(D), "activity": np.zeros(D), "row_inclusion": np.zeros((dims[j], D))} for j in spike}
    rels = []
    for r in relations:
        ids, vals = np.asarray(r["ids"], dtype=np.int64), np.asarray(r["values"], dtype=np.float64)
        rels.append({"ids": ids, "values": vals, "entities": list(r["entities"]), "alpha": float(r.get("alpha", 1.0)),
                     "alpha_sample": bool(r.get("alpha_sample", False)), "weights": r.get("weights"), "mean": float(np.mean(vals))})
    margin, pred, kept = np.inf, None, 0
    for it in range(1, iters + 1):
        for ri, r in enumerate(rels):
            if r["alpha_sample"]:
                e = (r["values"] - r["mean"]) - udot(r["ids"], [S[k] for k in r["entities"]])
                om = np.ones(len(e)) if r["weights"] is None else np.asarray(r["weights"], dtype=np.float64)
                r["alpha"] = O.sample_alpha(alpha_lambda0, alpha_nu0, len(e), float(np.sum(om * e * e)), seed, it, ri + 1)
        for j in range(n_ent):
            terms = [(r["ids"], r["values"], r["weights"], r["entities"].index(j), r["alpha"], r["mean"], [S[k] for k in r["entities"]])
                     for r in rels if j in r["entities"]]
            z = normals(seed, it, j + 1, dims[j], D)
            if j in spike:
                st = state[j]
                P, c = row_systems(terms, dims[j], D, np.diag(st[1]), np.zeros(D))
                S[j], m = sweep_rows(P, c, S[j], z, uniforms(seed, it, j + 1, dims[j], D), st)
                margin = min(margin, m)
                state[j] = hyper_draw(S[j], *spike[j], seed, it, j + 1)
                continue
            if ofe[j] is not None:
                uhat = np.stack([ofe[j].mul(beta[j][:, d]) for d in range(D)], axis=1)
                P, b = row_systems(terms, dims[j], D, Lam[j], mu[j] + uhat)
                S[j] = np.stack([RR.sample_row(P[i], b[i], z[i]) for i in range(dims[j])])
                Uc, nuh, Tinv = S[j] - uhat, D + ofe[j].n, np.eye(D) + beta[j].T @ beta[j] * lb[j]
            else:
                P, b = row_systems(terms, dims[j], D, Lam[j], mu[j])
                S[j] = np.stack([RR.sample_row(P[i], b[i], z[i]) for i in range(dims[j])])
                Uc, nuh, Tinv = S[j], float(D), np.eye(D)
            mu_N, beta_N, T_N, nu_N = O.hyper_params(Uc, np.zeros(D), 2.0, Tinv, nuh)
            mu[j], Lam[j] = O.hyper_draw(mu_N, beta_N, T_N, nu_N, seed, it, j + 1)
        for j in range(n_ent):
            if ofe[j] is not None:
                beta[j], _, _ = O.sample_beta(ofe[j], S[j], mu[j], Lam[j], lb[j], use_ff, None, seed, it, j + 1)
                lb[j] = O.sample_lambda_beta(beta[j], Lam[j], 1e-3, 1.0, seed, it, j + 1)
        if it > burnin:
            kept += 1
            for j in spike:
                nz = S[j] != 0
                acc[j]["inclusion"] += state[j][0]
                acc[j]["precision"] += state[j][1]
                acc[j]["activity"] += nz.sum(axis=0) / float(dims[j])
                acc[j]["row_inclusion"] += nz
            if test_ids is not None:
                p = udot(np.asarray(test_ids, dtype=np.int64), [S[k] for k in rels[0]["entities"]]) + rels[0]["mean"]
                pred = p if pred is None else pred + p
    out = {"S": S, "mu": mu, "Lam": Lam, "state": state, "alpha": [r["alpha"] for r in rels], "mean": [r["mean"] for r in rels],
           "margin": margin, "beta": beta, "lb": lb,
           "spike": {j: {k: v / max(kept, 1) for k, v in acc[j].items()} for j in spike}}
    if pred is not None:
        out["pred"] = pred / kept
    return out


def planted(seed=0, N1=150, N2=40, rank=3, share=0.5, sd=0.3):
    """the planted run: distinct cells of an N1 x N2 matrix of rank `rank`, a `share` of them observed with noise sd; a fifth of the
    observed cells (the last ones) are held out and keep their noisy values.  -> (ids, y, n_test)"""
    rng = np.random.default_rng(seed)
    n = int(round(share * N1 * N2))
    cells = rng.choice(N1 * N2, size=n, replace=False)
    ids = np.stack([cells // N2 + 1, cells % N2 + 1], axis=1).astype(np.int64)
    U, V = rng.standard_normal((N1, rank)), rng.standard_normal((N2, rank))
    y = (U[ids[:, 0] - 1] * V[ids[:, 1] - 1]).sum(axis=1) + sd * rng.standard_normal(n)
    return ids, y, n // 5


# ---- the inputs of the row-launch test (tests/test_gpu_spike.py (a)); the host test checks their near-tie margins on the CPU ----
ROW_COUNTS = (0, 1, 3, 4, 5, 63, 64, 65, 300)      # rows 0 .. 8 of the sampled entity hold exactly these many observations
ROW_DS = (1, 5, 16, 17, 32, 33, 64)
ROW_SEED, ROW_TAG = 1234, 5                         # the session context's seed; the entity tag of the launches


def row_cases():
    """(D, n_modes, mode, variant): every D and mode plain, and at D = 17 and 64 on mode 0 of the matrix the variants"""
    out = [(D, n_modes, mode, "plain") for D in ROW_DS for n_modes in (2, 3) for mode in range(n_modes)]
    return out + [(D, 2, 0, v) for D in (17, 64) for v in ("two_terms", "weights", "unit", "alpha_dev")]


def row_case(D, n_modes, mode, variant):
    """dims [37, 23] or [37, 23, 11]; rows 0 .. 8 of entity `mode` planted with ROW_COUNTS observations, the others with 2 .. 20;
    u_current with exact zeros; pi from 1e-6 to 1 - 1e-6 (evenly in the logit), tau from 0.5 to 50 (evenly in the log).
    -> {"dims", "N", "rels": [(ids, values, weights | None, alpha)], "facs", "u_current", "state", "sweep"}"""
    rng = np.random.default_rng([D, n_modes, mode, sorted(("plain", "two_terms", "weights", "unit", "alpha_dev")).index(variant)])
    dims = [37, 23, 11][:n_modes]
    N = dims[mode]
    counts = list(ROW_COUNTS) + [int(x) for x in rng.integers(2, 21, N - len(ROW_COUNTS))]

    def relation():
        rows = np.repeat(np.arange(1, N + 1), counts)
        rows = rows[rng.permutation(len(rows))]
        ids = np.stack([rows if k == mode else rng.integers(1, d + 1, len(rows)) for k, d in enumerate(dims)], axis=1).astype(np.int64)
        for k, d in enumerate(dims):                 # every id of the other modes occurs: the relation has exactly dims rows
            if k != mode:
                ids[:d, k] = np.arange(1, d + 1)
        return ids, rng.standard_normal(len(rows))

    rels = []
    for t in range(2 if variant == "two_terms" else 1):
        ids, vals = relation()
        w = None
        if variant == "weights":
            w = np.exp(rng.uniform(np.log(0.05), np.log(20.0), len(vals)))
        if variant == "unit":
            w = np.ones(len(vals))
        rels.append((ids, vals, w, [1.3, 0.7][t]))
    facs = [0.5 * rng.standard_normal((d, D)) for d in dims]
    u = rng.standard_normal((N, D)) * (rng.random((N, D)) < 0.7)
    lg = np.linspace(np.log(1e-6) - np.log1p(-1e-6), np.log1p(-1e-6) - np.log(1e-6), D) if D > 1 else np.array([0.3])
    tau = np.exp(np.linspace(np.log(0.5), np.log(50.0), D)) if D > 1 else np.array([2.0])
    state = np.stack([1.0 / (1.0 + np.exp(-lg)), tau, lg, np.log(tau)])
    sweep = 7000 + 10 * D + 3 * n_modes + mode + 100 * len(variant)
    return {"dims": dims, "N": N, "rels": rels, "facs": facs, "u_current": u, "state": state, "sweep": sweep}


def row_case_reference(case, D, mode, P=None, c=None, z=None, U=None, dtype=np.float64):
    """the restated launch of a case: (u, margin); P, c, z, U default to the numpy row systems and the oracle's streams"""
    N = case["N"]
    if P is None:
        terms = [(ids, vals, w, mode, alpha, float(np.mean(vals)), case["facs"]) for ids, vals, w, alpha in case["rels"]]
        P, c = row_systems(terms, N, D, np.diag(case["state"][1]), np.zeros(D))
    z = normals(ROW_SEED, case["sweep"], ROW_TAG, N, D) if z is None else z
    U = uniforms(ROW_SEED, case["sweep"], ROW_TAG, N, D) if U is None else U
    return sweep_rows(P, c, case["u_current"], z, U, case["state"], dtype)


# ---- the models of the whole-iteration test (tests/test_gpu_spike.py (c)) -----------------------------------------------------
CHAIN_SEED, CHAIN_D = 91, 8
CHAIN_MODELS = ("matrix", "tensor", "gfa", "alpha", "feat")


def chain_model(name):
    """-> (dims per entity, relations [{"ids", "values", "entities", "alpha", "alpha_sample"}], spike {entity: params}, feats per
    entity, n_test: the leading cells of relation 0 held out)"""
    rng = np.random.default_rng(500 + CHAIN_MODELS.index(name))

    def cells(dims, n):
        ids = np.stack([rng.integers(1, d + 1, n) for d in dims], axis=1).astype(np.int64)
        for k, d in enumerate(dims):
            ids[:d, k] = np.arange(1, d + 1)
        return ids, rng.standard_normal(n)

    n_test, feats = 60, None
    if name == "tensor":
        dims, ents = [30, 20, 9], [[0, 1, 2]]
        spike = {1: (1.0, 1.0, 1.0, 1.0)}
    elif name == "gfa":             # two views share the Normal-Wishart entity 0; each has a spike-and-slab column entity of its own
        dims, ents = [40, 17, 12], [[0, 1], [0, 2]]
        spike = {1: (1.0, 1.0, 1.0, 1.0), 2: (2.0, 0.5, 1.5, 0.5)}
    else:
        dims, ents = [40, 25], [[0, 1]]
        spike = {1: (1.0, 1.0, 1.0, 1.0)}
        if name == "feat":
            feats = [rng.standard_normal((dims[0], 4)), None]
    rels = []
    for e in ents:
        ids, vals = cells([dims[k] for k in e], 700)
        rels.append({"ids": ids, "values": vals, "entities": e, "alpha": 2.5, "alpha_sample": name == "alpha"})
    return dims, rels, spike, feats, n_test
