"""A numpy + scipy restatement of the non-negative prior of an entity's rows for the nonneg tests.

    u_id ~ N(0, 1 / tau_d) truncated to u_id >= 0,  tau_d ~ Gamma(shape, rate)

`draw_u(m, lam, U)` is the scalar map of csrc/nonneg.h: censored_restatement.draw_z at bound 0 for t = m sqrt(lam) >= -37, the
leading term of the tail below it.  `sweep_row` is the row step from (P, c, u_prev, U): D dependent truncated-normal draws in
order; `sweep_rows` the same for many rows at once.  Both also return the branch margin, the smallest |t + 37| they met: the two
branches differ by 7e-4 relative at the seam, so a t closer to it than rounding can carry is not one the device has to
reproduce.  `hyper_draw` is the hyper step (Marsaglia-Tsang on the streams 26 / 27 that include/bdf.h documents for
bdf_nonneg_hyper, on oracle.oracle's Philox and normals).  `run_chain` is whole macau() iterations over several relations in the
library's order -- alpha of every relation that samples it, then rows and hyper step of every entity in turn, then beta of every
entity with features -- with the Normal-Wishart and the spike-and-slab entities' steps as spike_restatement.run_chain restates
them.
"""
import math

import numpy as np
from scipy.special import ndtri as _ndtri

from oracle import oracle as O
from probit_restatement import udot
import censored_restatement as CR
import robust_restatement as RR
import spike_restatement as SR

P_NONNEG, P_NONNEG_N, P_NONNEG_U = 25, 26, 27
TAIL = -37.0                 # BDF_NONNEG_TAIL

_u01 = RR._u01


def draw_u(m, lam, U):
    """u ~ N(m, 1 / lam) truncated to u >= 0 by inversion from U in (0, 1]: with s = sqrt(lam), t = m s -- t >= -37:
    censored_restatement.draw_z at bound 0, c = +1, precision lam; t < -37: y = sqrt(t^2 - 2 log U), u = -2 log U / ((y - t) s)"""
    m, lam, U = np.broadcast_arrays(*(np.asarray(a, dtype=np.float64) for a in (m, lam, U)))
    s = np.sqrt(lam)
    t = m * s
    far = t < TAIL
    with np.errstate(all="ignore"):
        near = CR.draw_z(np.where(far, 0.0, m), 0.0, 1, lam, U)
        L = -2.0 * np.log(U)
        tail = L / ((np.sqrt(t * t + L) - t) * s)
    return np.maximum(np.where(far, tail, near), 0.0)


def draw_u1(m, lam, U):
    """draw_u for three floats, on math's erfc / log / sqrt and scipy's ndtri: the same formulas (the invariance test's chain
    makes 600,000 draws one after the other; tests/test_nonneg_host.py holds the two against each other)"""
    s = math.sqrt(lam)
    t = m * s
    if t < TAIL:
        L = -2.0 * math.log(U)
        return max(L / ((math.sqrt(t * t + L) - t) * s), 0.0)
    Pt = 0.5 * math.erfc(-t / 1.4142135623730951)
    lo = 0.5 * math.erfc(t / 1.4142135623730951) + U * Pt
    x = float(_ndtri(max(lo, CR.TINY))) if lo < 0.5 else -float(_ndtri(max((1.0 - U) * Pt, CR.TINY)))
    return max(m + x / s, 0.0)


def sweep_row(P, c, u_prev, U):
    """one row -> (u, margin).  For d = 0 .. D-1 in order: lambda = P_dd, m = (c_d - sum_{k != d} P_dk u_k) / lambda,
    u_d = draw_u(m, lambda, U_d)"""
    D = len(c)
    u = [float(x) for x in u_prev]
    margin = math.inf
    for d in range(D):
        lam = float(P[d][d])
        m = (float(c[d]) - sum(float(P[d][k]) * u[k] for k in range(D) if k != d)) / lam
        margin = min(margin, abs(m * math.sqrt(lam) - TAIL))
        u[d] = draw_u1(m, lam, float(U[d]))
    return np.array(u), margin


def sweep_rows(P, c, u_prev, U, with_t=False):
    """the sweep of N independent rows: P (N, D, D), c, u_prev, U (N, D) -> (u (N, D), margin[, t (N, D): every t met])"""
    P, c, U = np.asarray(P, dtype=np.float64), np.asarray(c, dtype=np.float64), np.asarray(U, dtype=np.float64)
    u = np.array(u_prev, dtype=np.float64)
    N, D = c.shape
    margin = np.inf
    ts = np.zeros((N, D))
    for d in range(D):
        lam = P[:, d, d]
        m = (c[:, d] - (np.einsum("nk,nk->n", P[:, d, :], u) - lam * u[:, d])) / lam
        ts[:, d] = m * np.sqrt(lam)
        if N:
            margin = min(margin, float(np.min(np.abs(ts[:, d] - TAIL))))
        u[:, d] = draw_u(m, lam, U[:, d])
    return (u, margin, ts) if with_t else (u, margin)


def gamma_on(seed, sweep, entity, g, a):
    """Gamma(a, 1), a >= 1, of variate g of bdf_nonneg_hyper: attempt t takes normal 2 t of (P_NONNEG_N, entity, g) and the uniform
    of (P_NONNEG_U, entity, g, pair t)"""
    assert a >= 1.0
    d = a - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    for t in range(256):
        x = float(O.normals(seed, sweep, P_NONNEG_N, entity, g, 2 * t + 1)[2 * t])
        v = 1.0 + c * x
        if v <= 0.0:
            continue
        v = v * v * v
        o = O.draw(seed, sweep, P_NONNEG_U, entity, g, t)
        uu = _u01(o[0], o[1])
        if uu < 1.0 - 0.0331 * (x * x) * (x * x):
            return d * v
        if np.log(uu) < 0.5 * x * x + d * (1.0 - v + np.log(v)):
            return d * v
    return d


def hyper_draw_q(q, N, shape, rate, seed, sweep, entity_tag):
    """the hyper step from the sums of squares q_d -> tau (D): G_d ~ Gamma(shape + N / 2), tau_d = G_d / (rate + q_d / 2)"""
    return np.array([gamma_on(seed, sweep, entity_tag, d, shape + 0.5 * N) / (rate + 0.5 * q[d]) for d in range(len(q))])


def hyper_draw(S, shape, rate, seed, sweep, entity_tag):
    """the hyper step from the rows S (N, D)"""
    S = np.asarray(S, dtype=np.float64)
    return hyper_draw_q(np.sum(S * S, axis=0), S.shape[0], shape, rate, seed, sweep, entity_tag)


def uniforms(seed, sweep, entity_tag, N, D, row_begin=0):
    """U (N, D): bdf_u01 of words x and y of block (P_NONNEG, entity_tag, row_begin + row, pair d)"""
    rows = np.arange(row_begin, row_begin + N, dtype=np.uint64)
    sw = np.full(N, sweep, dtype=np.uint64)
    return np.stack([RR._blocks(seed, sw, P_NONNEG, int(entity_tag) & 0xFFFFFF, rows, d)[0] for d in range(D)], axis=1) if N else np.zeros((0, D))


def run_chain(relations, dims, D, seed, iters, nonneg, spike=None, feats=None, burnin=0, test_ids=None, use_ff=True, alpha_lambda0=1.0,
              alpha_nu0=2.0):
    """macau() iterations 1 .. iters.  relations: a list of dicts {"ids" (n, modes) 1-based, "values", "entities" (the entity
    index of every mode), "alpha", "alpha_sample", "weights" (None or per cell)}; dims: rows per entity; nonneg: {entity index:
    (shape, rate)}; spike: {entity index: (incl_a, incl_b, shape, rate)}; feats: dense side information per entity or None.
    A relation ALL of whose entities are non-negative is not centred (mean 0).  test_ids: cells of relation 0.
    Returns {"S", "mu", "Lam", "tau" (per non-negative entity), "state" (per spike entity), "alpha", "mean", "margin" (the branch
    margin), "spike_margin", and over iterations burnin + 1 .. iters the means "precision" and "factors" per non-negative entity
    and "pred"}"""
    n_ent = len(dims)
    spike = spike or {}
    feats = feats or [None] * n_ent
    S = [np.zeros((n, D)) for n in dims]
    mu = [np.zeros(D) for _ in dims]
    Lam = [5.0 * np.eye(D) for _ in dims]
    ofe = [None if F is None else O.Feat.from_dense(np.asarray(F, dtype=np.float64)) for F in feats]
    beta = [None if f is None else np.zeros((f.n, D)) for f in ofe]
    lb = [1.0] * n_ent
    tau = {j: np.ones(D) for j in nonneg}
    state = {j: SR.initial_state(D) for j in spike}
    acc = {j: {"precision": np.zeros(D), "factors": np.zeros((dims[j], D))} for j in nonneg}
    rels = []
    for r in relations:
        ids, vals = np.asarray(r["ids"], dtype=np.int64), np.asarray(r["values"], dtype=np.float64)
        mean = 0.0 if all(k in nonneg for k in r["entities"]) else float(np.mean(vals))
        rels.append({"ids": ids, "values": vals, "entities": list(r["entities"]), "alpha": float(r.get("alpha", 1.0)),
                     "alpha_sample": bool(r.get("alpha_sample", False)), "weights": r.get("weights"), "mean": mean})
    margin, spike_margin, pred, kept = np.inf, np.inf, None, 0
    for it in range(1, iters + 1):
        for ri, r in enumerate(rels):
            if r["alpha_sample"]:
                e = (r["values"] - r["mean"]) - udot(r["ids"], [S[k] for k in r["entities"]])
                om = np.ones(len(e)) if r["weights"] is None else np.asarray(r["weights"], dtype=np.float64)
                r["alpha"] = O.sample_alpha(alpha_lambda0, alpha_nu0, len(e), float(np.sum(om * e * e)), seed, it, ri + 1)
        for j in range(n_ent):
            terms = [(r["ids"], r["values"], r["weights"], r["entities"].index(j), r["alpha"], r["mean"], [S[k] for k in r["entities"]])
                     for r in rels if j in r["entities"]]
            if j in nonneg:
                P, c = SR.row_systems(terms, dims[j], D, np.diag(tau[j]), np.zeros(D))
                S[j], m = sweep_rows(P, c, S[j], uniforms(seed, it, j + 1, dims[j], D))
                margin = min(margin, m)
                tau[j] = hyper_draw(S[j], *nonneg[j], seed, it, j + 1)
                continue
            z = SR.normals(seed, it, j + 1, dims[j], D)
            if j in spike:
                st = state[j]
                P, c = SR.row_systems(terms, dims[j], D, np.diag(st[1]), np.zeros(D))
                S[j], m = SR.sweep_rows(P, c, S[j], z, SR.uniforms(seed, it, j + 1, dims[j], D), st)
                spike_margin = min(spike_margin, m)
                state[j] = SR.hyper_draw(S[j], *spike[j], seed, it, j + 1)
                continue
            if ofe[j] is not None:
                uhat = np.stack([ofe[j].mul(beta[j][:, d]) for d in range(D)], axis=1)
                P, b = SR.row_systems(terms, dims[j], D, Lam[j], mu[j] + uhat)
                S[j] = np.stack([RR.sample_row(P[i], b[i], z[i]) for i in range(dims[j])])
                Uc, nuh, Tinv = S[j] - uhat, D + ofe[j].n, np.eye(D) + beta[j].T @ beta[j] * lb[j]
            else:
                P, b = SR.row_systems(terms, dims[j], D, Lam[j], mu[j])
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
            for j in nonneg:
                acc[j]["precision"] += tau[j]
                acc[j]["factors"] += S[j]
            if test_ids is not None:
                p = udot(np.asarray(test_ids, dtype=np.int64), [S[k] for k in rels[0]["entities"]]) + rels[0]["mean"]
                pred = p if pred is None else pred + p
    out = {"S": S, "mu": mu, "Lam": Lam, "tau": tau, "state": state, "alpha": [r["alpha"] for r in rels], "mean": [r["mean"] for r in rels],
           "margin": margin, "spike_margin": spike_margin, "beta": beta, "lb": lb,
           "nonneg": {j: {k: v / max(kept, 1) for k, v in acc[j].items()} for j in nonneg}}
    if pred is not None:
        out["pred"] = pred / kept
    return out


def planted(seed=0, N1=150, N2=40, rank=3, share=0.5, sd=0.3):
    """the planted run: distinct cells of an N1 x N2 matrix of rank `rank` with NON-NEGATIVE factors (|N(0, 1)| entries), a `share`
    of them observed with noise sd; a fifth of the observed cells (the last ones) are held out and keep their noisy values.
    -> (ids, y, n_test)"""
    rng = np.random.default_rng(seed)
    n = int(round(share * N1 * N2))
    cells = rng.choice(N1 * N2, size=n, replace=False)
    ids = np.stack([cells // N2 + 1, cells % N2 + 1], axis=1).astype(np.int64)
    U, V = np.abs(rng.standard_normal((N1, rank))), np.abs(rng.standard_normal((N2, rank)))
    y = (U[ids[:, 0] - 1] * V[ids[:, 1] - 1]).sum(axis=1) + sd * rng.standard_normal(n)
    return ids, y, n // 5


def planted_chain(chain_seed, iters=300, burnin=200, D=8):
    """the restated chain on the planted data, both entities non-negative with the defaults, alpha = 1 / 0.09 -> (held-out RMSE,
    the mean square of every component of the 40-row entity's posterior-mean factors, ascending)"""
    ids, y, n_test = planted()
    n = len(y)
    rel = {"ids": ids[:n - n_test], "values": y[:n - n_test], "entities": [0, 1], "alpha": 1.0 / 0.09}
    out = run_chain([rel], [150, 40], D, chain_seed, iters, {0: (1.0, 1.0), 1: (1.0, 1.0)}, burnin=burnin, test_ids=ids[n - n_test:])
    rmse = float(np.sqrt(np.mean((out["pred"] - y[n - n_test:]) ** 2)))
    return rmse, np.sort(np.mean(out["nonneg"][1]["factors"] ** 2, axis=0))


# ---- the inputs of the sweep test (tests/test_gpu_nonneg.py (a)); the host test checks their branch margins on the CPU ----------
SWEEP_DS = (1, 5, 16, 17, 32, 33, 64)
SWEEP_ROWS = (1, 63, 64, 65, 200)
SWEEP_SEED, SWEEP_TAG, SWEEP_ROW_BEGIN = SR.ROW_SEED, 6, 1000      # the test context's seed; the entity tag; the first row's id
SWEEP_TARGETS = (12.0, 0.3, -15.0, -50.0)                          # t > 8, |t| < 1, t in (-36, -5), t < -37


def sweep_case(D, n_rows):
    """crafted systems: P = diag(0.5 .. 4) + A A' with A = 0.3 N(0, 1) / sqrt(D) (D x D), c_id = target sqrt(P_dd) with the four
    targets of SWEEP_TARGETS dealt to the elements (i + d) mod 4, so that the elements between them meet the four classes of t;
    u_current = |N(0, 1)| / 2 with exact zeros.  -> {"P", "c", "u_current", "sweep"}"""
    rng = np.random.default_rng([26, D, n_rows])
    A = 0.3 * rng.standard_normal((n_rows, D, D)) / np.sqrt(D)
    P = np.einsum("nij,nkj->nik", A, A)
    P = 0.5 * (P + np.transpose(P, (0, 2, 1)))
    P[:, np.arange(D), np.arange(D)] += np.exp(rng.uniform(np.log(0.5), np.log(4.0), (n_rows, D)))
    cls = (np.arange(n_rows)[:, None] + np.arange(D)[None, :]) % 4
    c = np.asarray(SWEEP_TARGETS)[cls] * np.sqrt(P[:, np.arange(D), np.arange(D)]) * rng.uniform(0.9, 1.1, (n_rows, D))
    u = 0.5 * np.abs(rng.standard_normal((n_rows, D))) * (rng.random((n_rows, D)) < 0.8)
    return {"P": P, "c": c, "u_current": u, "sweep": 9000 + 10 * D + n_rows}


def t_classes(t):
    """how many of the t met fall into the four classes"""
    t = np.asarray(t)
    return [int(np.sum(t > 8)), int(np.sum(np.abs(t) < 1)), int(np.sum((t > -36) & (t < -5))), int(np.sum(t < TAIL))]


def row_case(D, n_modes, mode, variant):
    """spike_restatement.row_case with what this prior needs of it: tau (its state's second row) and a NON-NEGATIVE u_current"""
    case = SR.row_case(D, n_modes, mode, variant)
    return dict(case, tau=case["state"][1].copy(), u_current=np.abs(case["u_current"]))


ROW_TAG = SR.ROW_TAG


# ---- the models of the whole-iteration test (tests/test_gpu_nonneg.py (d)) -------------------------------------------------------
CHAIN_SEED, CHAIN_D = 92, 8
CHAIN_MODELS = ("semi", "both", "tensor", "alpha", "feat", "spike")


def chain_model(name):
    """-> (dims per entity, relations [{"ids", "values", "entities", "alpha", "alpha_sample"}], nonneg {entity: (shape, rate)}, spike
    {entity: params}, feats per entity, n_test: the leading cells of relation 0 held out).  The values are |N(0, 1)|: non-negative
    data, as the uncentred model of "both" wants them"""
    rng = np.random.default_rng(600 + CHAIN_MODELS.index(name))

    def cells(dims, n):
        ids = np.stack([rng.integers(1, d + 1, n) for d in dims], axis=1).astype(np.int64)
        for k, d in enumerate(dims):
            ids[:d, k] = np.arange(1, d + 1)
        return ids, np.abs(rng.standard_normal(n))

    n_test, feats, spike = 60, None, {}
    if name == "tensor":
        dims, ents = [30, 20, 9], [[0, 1, 2]]
        nonneg = {1: (1.0, 1.0)}
    elif name == "both":
        dims, ents = [40, 25], [[0, 1]]
        nonneg = {0: (1.0, 1.0), 1: (2.0, 0.5)}
    elif name == "spike":           # one relation between a spike-and-slab and a non-negative entity
        dims, ents = [40, 25], [[0, 1]]
        spike, nonneg = {0: (1.0, 1.0, 1.0, 1.0)}, {1: (1.0, 1.0)}
    else:
        dims, ents = [40, 25], [[0, 1]]
        nonneg = {1: (1.0, 1.0)}
        if name == "feat":
            feats = [rng.standard_normal((dims[0], 4)), None]
    rels = []
    for e in ents:
        ids, vals = cells([dims[k] for k in e], 700)
        rels.append({"ids": ids, "values": vals, "entities": e, "alpha": 2.5, "alpha_sample": name == "alpha"})
    return dims, rels, nonneg, spike, feats, n_test
