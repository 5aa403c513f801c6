"""A numpy restatement of a relation's row and column biases (setBias) for their tests.

With B the biased modes, y_k = mean + sum over m in B of b^m_(id_m(k)) + udot_k + eps_k, b^m_j ~ N(0, 1 / lambda_m) and lambda_m ~
Gamma(shape_m, rate_m).  `normals(seed, sweep, rel_tag, rows, mode)` are the rows' normals on the stream bdf_bias_draw documents
(include/bdf.h: purpose 28, entity 0x800000 | rel_tag, row = the biased entity's 0-based row, normal = the 0-based mode) and
`gamma_variates(seed, sweep, rel_tag, modes, a)` Marsaglia-Tsang on purposes 29 / 30 (row = the 0-based mode, pair = attempt; a
shape below 1 goes through the boost u^(1/a) of the variate of a + 1, u the uniform of pair 0xffff), both on robust_restatement's
vectorised Philox blocks; `normal_one` and `gamma_mt` the same one at a time on oracle.normals and oracle.draw.  `row_conditional`
is (mean_j, prec_j) of a mode's rows, `draw_rows` and `draw_lambda` the two conditional draws, `base` what the step leaves the rows
and the pairs, `step` the whole of bdf_bias_draw from the residuals, and `run_chain(...)` whole macau() iterations in the library's
order -- biases and their precisions | U,V,alpha(previous) -> alpha | U,V,b -> rows, hyperprior of every entity in turn -> beta of
every entity with features -- on robust_restatement.sample_rows (the rows see the values less the cell's biases: base = mean + the
biases) and the oracle's hyperprior, beta and alpha, with the predictions, the held-out log predictive density (lpd_restatement)
and WAIC (waic_restatement) of every draw.  `planted(seed)` is the data of the issue's experiment.
"""
import numpy as np

from oracle import oracle as O
import lpd_restatement as LR
import robust_restatement as RR
import waic_restatement as WR
from probit_restatement import udot

P_BIAS, P_BIAS_N, P_BIAS_U = 28, 29, 30
BOOST_PAIR = 0xFFFF


def normal_one(seed, sweep, rel_tag, row, mode):
    """z of row `row` of biased mode `mode` (0-based): normal `mode` of stream (P_BIAS, entity, row)"""
    return float(O.normals(seed, sweep, P_BIAS, RR._entity(rel_tag), row, mode + 1)[mode])


def normals(seed, sweep, rel_tag, rows, mode):
    """normal_one for every row at once: element mode % 2 of pair mode // 2"""
    rows = np.asarray(rows, dtype=np.uint64)
    sw = np.broadcast_to(np.asarray(sweep, dtype=np.uint64), rows.shape)
    u1, u2 = RR._blocks(seed, sw, P_BIAS, RR._entity(rel_tag), rows, mode // 2)
    r = np.sqrt(-2.0 * np.log(u1))
    return r * (np.sin(RR.TWO_PI * u2) if mode % 2 else np.cos(RR.TWO_PI * u2))


def normals_reduced(seed, sweep, rel_tag, rows, mode):
    """`normals` with the angle reduced in u, exactly, before it is scaled by 2 pi, as bdf_sincos2pi does: q = rint(4 u), x = 2 pi
    (u - q / 4) in [-pi / 4, pi / 4] and the quadrant.  cos(2 pi u) of the ROUNDED product 2 pi u is off by an ulp of the angle -- up
    to 4e-16 absolute, which near a zero of the cosine is any relative error (u = 0.7501944: 2.3e-13).  For thousands of rows, where
    some row without cells draws such a normal and its bias is nothing but z / sqrt(lambda)."""
    rows = np.asarray(rows, dtype=np.uint64)
    sw = np.broadcast_to(np.asarray(sweep, dtype=np.uint64), rows.shape)
    u1, u2 = RR._blocks(seed, sw, P_BIAS, RR._entity(rel_tag), rows, mode // 2)
    q = np.rint(4.0 * u2)
    x = RR.TWO_PI * (u2 - 0.25 * q)                        # (the difference is exact)
    sx, cx = np.sin(x), np.cos(x)
    iq = q.astype(np.int64) & 3
    s = np.where(iq == 0, sx, np.where(iq == 1, cx, np.where(iq == 2, -sx, -cx)))
    c = np.where(iq == 0, cx, np.where(iq == 1, -sx, np.where(iq == 2, -cx, sx)))
    return np.sqrt(-2.0 * np.log(u1)) * (s if mode % 2 else c)


def gamma_mt(seed, sweep, rel_tag, mode, a):
    """Gamma(a, 1) for biased mode `mode`: attempt t takes normal 2 t of (P_BIAS_N, entity, mode) and the uniform of (P_BIAS_U, entity,
    mode, pair t); a < 1: the variate of a + 1 times u^(1 / a), u the uniform of pair 0xffff"""
    ent = RR._entity(rel_tag)
    boost = 1.0
    if a < 1.0:
        o = O.draw(seed, sweep, P_BIAS_U, ent, mode, BOOST_PAIR)
        boost = RR._u01(o[0], o[1]) ** (1.0 / a)
        a += 1.0
    d = a - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    for t in range(256):
        x = float(O.normals(seed, sweep, P_BIAS_N, ent, mode, 2 * t + 1)[2 * t])
        v = 1.0 + c * x
        if v <= 0.0:
            continue
        v = v * v * v
        o = O.draw(seed, sweep, P_BIAS_U, ent, mode, t)
        u = RR._u01(o[0], o[1])
        if u < 1.0 - 0.0331 * (x * x) * (x * x):
            return boost * d * v
        if np.log(u) < 0.5 * x * x + d * (1.0 - v + np.log(v)):
            return boost * d * v
    return boost * d


def gamma_variates(seed, sweep, rel_tag, modes, a):
    """gamma_mt for every (modes[i], a[i]) at once"""
    rows = np.asarray(modes, dtype=np.uint64)
    sweep = np.broadcast_to(np.asarray(sweep, dtype=np.uint64), rows.shape)
    a = np.array(np.broadcast_to(np.asarray(a, dtype=np.float64), rows.shape))
    ent = RR._entity(rel_tag)
    boost = np.ones(len(rows))
    low = a < 1.0
    if low.any():
        u, _ = RR._blocks(seed, sweep[low], P_BIAS_U, ent, rows[low], BOOST_PAIR)
        boost[low] = u ** (1.0 / a[low])
        a[low] += 1.0
    d = a - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    out = boost * d
    todo = np.arange(len(rows))
    for t in range(256):
        if len(todo) == 0:
            break
        u1, _u2 = RR._blocks(seed, sweep[todo], P_BIAS_N, ent, rows[todo], t)
        x = np.sqrt(-2.0 * np.log(u1)) * np.cos(RR.TWO_PI * _u2)
        dd = d[todo]
        v = 1.0 + c[todo] * x
        ok = v > 0.0
        v = np.where(ok, v, 1.0) ** 3
        u, _ = RR._blocks(seed, sweep[todo], P_BIAS_U, ent, rows[todo], t)
        acc = ok & ((u < 1.0 - 0.0331 * (x * x) * (x * x)) | (np.log(u) < 0.5 * x * x + dd * (1.0 - v + np.log(v))))
        out[todo[acc]] = boost[todo[acc]] * dd[acc] * v[acc]
        todo = todo[~acc]
    return out


def others_off(e, ids, biases, mode):
    """r_k = e_k less the current biases of the biased modes other than `mode`, subtracted in rising mode order; biases: {mode0: b}"""
    r = np.array(e, dtype=np.float64)
    for m in sorted(biases):
        if m != mode:
            r = r - biases[m][np.asarray(ids, dtype=np.int64)[:, m] - 1]
    return r


def row_sums(rows0, N, r):
    """(n_j, S_j) of every row 0 .. N-1"""
    rows0 = np.asarray(rows0, dtype=np.int64)
    return np.bincount(rows0, minlength=N), np.bincount(rows0, weights=np.asarray(r, dtype=np.float64), minlength=N)


def row_conditional(S, n, alpha, lam):
    """(mean_j, prec_j) of b_j | rest: prec_j = lambda + alpha n_j, mean_j = alpha S_j / prec_j; a row without cells: its prior"""
    prec = lam + alpha * np.asarray(n, dtype=np.float64)
    return alpha * np.asarray(S, dtype=np.float64) / prec, prec


def draw_rows(S, n, alpha, lam, z):
    """b_j = alpha S_j / prec_j + z_j / sqrt(prec_j)"""
    mean, prec = row_conditional(S, n, alpha, lam)
    return mean + np.asarray(z, dtype=np.float64) / np.sqrt(prec)


def draw_lambda(G, rate, sum_b2):
    """lambda | b ~ Gamma(shape + N / 2, rate + sum b^2 / 2) from G ~ Gamma(shape + N / 2, 1)"""
    return G / (rate + 0.5 * sum_b2)


def base(ids, biases, mean):
    """mean + the biases of every cell, added in rising mode order"""
    ids = np.asarray(ids, dtype=np.int64)
    out = np.full(len(ids), float(mean))
    for m in sorted(biases):
        out = out + biases[m][ids[:, m] - 1]
    return out


def step(seed, sweep, rel_tag, ids, dims, e, alpha, spec, biases, lam):
    """bdf_bias_draw from the residuals e = y - (udot + mean): spec {mode0: (shape, rate)}, biases {mode0: b} and lam {mode0: lambda}
    as the step finds them -> (biases, lam) as it leaves them.  Every mode's rows read the lambda the step found"""
    ids = np.asarray(ids, dtype=np.int64)
    biases = {m: np.array(b, dtype=np.float64) for m, b in biases.items()}
    lam_out = dict(lam)
    for m in sorted(spec):
        N = dims[m]
        n, S = row_sums(ids[:, m] - 1, N, others_off(e, ids, biases, m))
        biases[m] = draw_rows(S, n, alpha, lam[m], normals(seed, sweep, rel_tag, np.arange(N), m))
        shape, rate = spec[m]
        G = float(gamma_variates(seed, sweep, rel_tag, [m], shape + 0.5 * N)[0])
        lam_out[m] = draw_lambda(G, rate, float(np.sum(biases[m] * biases[m])))
    return biases, lam_out


# ---- whole iterations --------------------------------------------------------------------------------------------------------
def run_chain(ids, values, dims, D, seed, iters, spec=None, alpha=1.0, alpha_sample=False, feats=None, use_ff=True, rel_tag=1,
              test_ids=None, test_values=None, burnin=0, waic=False, train_pred=False, alpha_lambda0=1.0, alpha_nu0=2.0):
    """macau() on ONE relation (ids (n, n_modes) 1-based) between len(dims) entities, entity k with the dense side information
    feats[k] (or None).  spec {mode0: (shape, rate)}: the rows of those entities carry biases; None or empty: the Gaussian chain on
    the same row sampler.  Iterations 1 .. iters.  Returns {"S", "mu", "Lam", "beta", "lb", "alpha", "mean", "bias", "lambda"} after
    the last one, "bias_mean" and "lambda_mean" (their means over iterations burnin + 1 .. iters) and, with test_ids, "pred" and
    "stdev": the mean and the sample sd over the same iterations of udot + mean + biases on those cells; with test_values too, "lpd"
    (per test cell) and "LPD"; waic: "WAIC" (waic_restatement.summary) over the training cells; train_pred: "train_pred", the mean
    prediction of the training cells; "full": the mean over the same iterations of every cell's prediction (two or three modes)."""
    n_modes = len(dims)
    spec = dict(spec or {})
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
    biases = {m: np.zeros(dims[m]) for m in spec}
    lam = {m: spec[m][0] / spec[m][1] for m in spec}
    omega = np.ones(len(values))
    n_post = max(iters - burnin, 1)
    pred = pred2 = tpred = full = None
    b_sum, l_sum = {m: np.zeros(dims[m]) for m in spec}, {m: 0.0 for m in spec}
    stream, wstream = LR.Stream(), WR.Stream()
    for it in range(1, iters + 1):
        ud = udot(ids, S)
        if spec:                           # the biases and their precisions | U, V and the previous iteration's alpha
            biases, lam = step(seed, it, rel_tag, ids, dims, values - (ud + mean), alpha, spec, biases, lam)
        lin = base(ids, biases, mean)
        if alpha_sample:                   # alpha | U, V, b
            r = values - (ud + lin)
            alpha = O.sample_alpha(alpha_lambda0, alpha_nu0, len(values), float(np.sum(r * r)), seed, it, rel_tag)
        for j in range(n_modes):
            if ofe[j] is not None:
                uhat = np.stack([ofe[j].mul(beta[j][:, d]) for d in range(D)], axis=1)
                S[j] = RR.sample_rows(ids, values, omega, dims, j, alpha, lin, S, mu[j] + uhat, Lam[j], seed, it, j + 1)
                U, nuh, Tinv = S[j] - uhat, D + ofe[j].n, np.eye(D) + beta[j].T @ beta[j] * lb[j]
            else:
                S[j] = RR.sample_rows(ids, values, omega, dims, j, alpha, lin, S, mu[j], Lam[j], seed, it, j + 1)
                U, nuh, Tinv = S[j], float(D), np.eye(D)
            mu_N, beta_N, T_N, nu_N = O.hyper_params(U, np.zeros(D), 2.0, Tinv, nuh)
            mu[j], Lam[j] = O.hyper_draw(mu_N, beta_N, T_N, nu_N, seed, it, j + 1)
        for j in range(n_modes):
            if ofe[j] is not None:
                beta[j], _, _ = O.sample_beta(ofe[j], S[j], mu[j], Lam[j], lb[j], use_ff, None, seed, it, j + 1)
                lb[j] = O.sample_lambda_beta(beta[j], Lam[j], 1e-3, 1.0, seed, it, j + 1)
        phase = 0 if it <= burnin else (1 if it == burnin + 1 else 2)
        if test_ids is not None:
            p = udot(test_ids, S) + base(test_ids, biases, mean)
            if test_values is not None:
                stream.update(LR.cell_loglik(test_values, p, alpha), phase)
            if it > burnin:
                pred, pred2 = (p, p * p) if pred is None else (pred + p, pred2 + p * p)
        if waic or train_pred:
            pt = udot(ids, S) + lin
            if waic:
                wstream.update(LR.cell_loglik(values, pt, alpha), phase)
            if train_pred and it > burnin:
                tpred = pt if tpred is None else tpred + pt
        if it > burnin:
            for m in spec:
                b_sum[m] += biases[m]
                l_sum[m] += lam[m]
            if n_modes <= 3:
                f = np.einsum("id,jd->ij", S[0], S[1]) if n_modes == 2 else np.einsum("id,jd,kd->ijk", S[0], S[1], S[2])
                f = f + mean
                for m in sorted(biases):
                    f = f + biases[m].reshape([-1 if k == m else 1 for k in range(n_modes)])
                full = f if full is None else full + f
    out = {"S": S, "mu": mu, "Lam": Lam, "beta": beta, "lb": lb, "alpha": alpha, "mean": mean, "bias": biases, "lambda": lam,
           "bias_mean": {m: b_sum[m] / n_post for m in spec}, "lambda_mean": {m: l_sum[m] / n_post for m in spec}}
    if pred is not None:
        k = iters - burnin
        out["pred"] = pred / k
        out["stdev"] = np.sqrt(np.maximum((pred2 - out["pred"] ** 2 * k) / (k - 1), 0.0)) if k >= 3 else np.full(len(pred), np.nan)
    if test_values is not None and iters > burnin:
        out["lpd"] = stream.lpd()
        out["LPD"] = float(np.mean(out["lpd"]))
    if waic and iters > burnin:
        out["WAIC"] = WR.summary(wstream.lppd(), wstream.V())
    if tpred is not None:
        out["train_pred"] = tpred / n_post
    if full is not None:
        out["full"] = full / n_post
    return out


def planted(seed=0, N1=150, N2=100, rank=3, n_train=4500, n_test=1500, sd_load=0.5, sd_bias=1.0, sd_noise=0.3):
    """planted biases: distinct cells of an N1 x N2 matrix, y = a_i + b_j + u*_i.v*_j + noise, loadings of sd sd_load, a and b of sd
    sd_bias; the LAST n_test cells are held out.  Returns (ids, y, a, b, n_test, alpha = 1 / sd_noise^2)"""
    rng = np.random.default_rng(seed)
    n_cells = n_train + n_test
    cells = rng.choice(N1 * N2, size=n_cells, replace=False)
    ids = np.stack([cells // N2 + 1, cells % N2 + 1], axis=1).astype(np.int64)
    U, V = sd_load * rng.standard_normal((N1, rank)), sd_load * rng.standard_normal((N2, rank))
    a, b = sd_bias * rng.standard_normal(N1), sd_bias * rng.standard_normal(N2)
    y = a[ids[:, 0] - 1] + b[ids[:, 1] - 1] + (U[ids[:, 0] - 1] * V[ids[:, 1] - 1]).sum(axis=1) + sd_noise * rng.standard_normal(n_cells)
    return ids, y, a, b, n_test, float(1.0 / sd_noise ** 2)


def centred_rms(est, truth):
    """the rms error of est against truth, both centred (the shift between two biased modes and the mean is not identified)"""
    est, truth = np.asarray(est, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    return float(np.sqrt(np.mean(((est - est.mean()) - (truth - truth.mean())) ** 2)))


def iteration_case(n_modes, with_feat, alpha_sample):
    """the small relation of the whole-iteration test: (ids, values, dims, D-independent feats per entity, number of leading test
    cells, alpha, alpha_sample): 37 x 23 (x 11), 800 cells drawn with replacement (some repeat), the first 200 held out; planted row
    biases of sd 1 in every mode"""
    rng = np.random.default_rng(270 + n_modes)
    dims = [37, 23, 11][:n_modes]
    n, n_test = 800, 200
    ids = np.stack([rng.integers(1, d + 1, n) for d in dims], axis=1).astype(np.int64)
    for k, d in enumerate(dims):
        ids[n_test:n_test + d, k] = np.arange(1, d + 1)   # every id occurs among the training cells: the entities have exactly dims rows
    y = 0.5 * rng.standard_normal(n)
    for k, d in enumerate(dims):
        y = y + rng.standard_normal(d)[ids[:, k] - 1]
    feats = [None] * n_modes
    if with_feat:
        feats[0] = rng.standard_normal((dims[0], 5))
    return ids, y, dims, feats, n_test, 2.5, bool(alpha_sample)
