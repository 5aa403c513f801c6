"""A numpy restatement of the Polya-Gamma noise models for the logit / count tests.

`Cursor` is the cursor bdf_pg_draw documents (include/bdf.h: purpose 18, entity 0x800000 | rel_tag, row = observation, one block per
request, pair = 0, 1, 2, ...) on oracle.draw and oracle.normals; `jstar(z, cur)` Devroye's sampler of J*(1, z) as csrc/pg.h states it,
line for line, `pg(b, c, cur)` the draw of PG(b, c).  Both also return the smallest relative margin of every accept / reject
decision they took: a flipped decision gives another variate outright, so a test that compares two implementations of the sampler
picks streams whose decisions are not close calls.  `draw_pg(psi, b, seed, sweep, rel_tag)` is the same for many observations at once
on a vectorised Philox (held against the scalar form in test_pg_host.py).  `b_of` / `kappa_of` / `linear_of` are the models' maps,
`moments` the mean and variance of PG(b, c) as the header evaluates them, `link` the two prediction links, and `run_chain(...)`
whole macau() iterations in the library's order -- omega | U,V -> rows, hyperprior of every entity in turn -> beta of every entity
with features -- on robust_restatement's weighted row system, with the hyperprior and beta taken from the oracle.
"""
import math

import numpy as np
from scipy.special import erfc

from oracle import oracle as O
from probit_restatement import _philox4x32_10, udot
import robust_restatement as RR

P_PG = 18
T = 0.64
SUM_MAX = 170
TRIES = 256
TERMS = 64
SERIES_BELOW = 0.25
TWO_PI = 6.283185307179586476925286766559
PI = np.pi
TINY = np.finfo(np.float64).tiny
HALF_LOG_2PI = 0.91893853320467274178
INF = float("inf")


def _entity(rel_tag):
    return (0x800000 | int(rel_tag)) & 0xFFFFFF


def _u01(lo, hi):
    x = (int(hi) << 32) | int(lo)
    return ((x >> 11) + 0.5) * 2.0 ** -53


# ---- the normal CDF and its logarithm as csrc/lpd.h states them ---------------------------------------------------------------------
def phi(x):
    return 0.5 * erfc(-np.asarray(x, dtype=np.float64) / 1.4142135623730951)


def log_phi(x):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        up = np.log1p(-phi(-np.maximum(x, 0.0)))
        mid = np.log(phi(np.clip(x, -37.0, 0.0)))
        xt = np.minimum(x, -37.0)
        r = 1.0 / (xt * xt)
        ser = np.log1p(r * (-1.0 + r * (3.0 + r * (-15.0 + r * (105.0 + r * (-945.0 + r * (10395.0 + r * (-135135.0 + r * 2027025.0))))))))
        far = -0.5 * xt * xt - np.log(-xt) - HALF_LOG_2PI + ser
    return np.where(x >= 0.0, up, np.where(x > -37.0, mid, far))


# ---- the models' maps ---------------------------------------------------------------------------------------------------------------
def b_of(model, y, r):
    y = np.asarray(y, dtype=np.float64)
    return np.ones_like(y) if model == 1 else y + np.asarray(r, dtype=np.float64)


def kappa_of(model, y, r):
    y = np.asarray(y, dtype=np.float64)
    return y - 0.5 if model == 1 else 0.5 * (y - np.asarray(r, dtype=np.float64))


def linear_of(mean, y, kappa, omega):
    return mean + (np.asarray(y, dtype=np.float64) - kappa / omega)


def link(model, psi, r=0.0):
    """the prediction links: 2 logistic (stable on both sides), 3 counts r exp(min(psi, 700)); model 1 -> link 2, model 2 -> link 3"""
    psi = np.asarray(psi, dtype=np.float64)
    with np.errstate(all="ignore"):
        if model == 1:
            e = np.exp(-np.abs(psi))
            return np.where(psi >= 0.0, 1.0 / (1.0 + e), e / (1.0 + e))
        return np.asarray(r, dtype=np.float64) * np.exp(np.minimum(psi, 700.0))


def moments(b, a):
    """mean and variance of PG(b, c), a = |c|: in terms of e^-a, and by the series below SERIES_BELOW"""
    b, a = np.broadcast_arrays(np.asarray(b, dtype=np.float64), np.asarray(a, dtype=np.float64))
    e = np.exp(-a)
    d = (1.0 + e) * (1.0 + e)
    x2, a2 = 0.25 * a * a, a * a
    Tq = 1.0 + x2 * (-1.0 / 3.0 + x2 * (2.0 / 15.0 + x2 * (-17.0 / 315.0 + x2 * (62.0 / 2835.0 + x2 * (-1382.0 / 155925.0 +
         x2 * (21844.0 / 6081075.0 + x2 * (-929569.0 / 638512875.0)))))))
    G = 1.0 / 6.0 + a2 * (1.0 / 120.0 + a2 * (1.0 / 5040.0 + a2 * (1.0 / 362880.0 + a2 * (1.0 / 39916800.0 +
        a2 * (1.0 / 6227020800.0 + a2 * (1.0 / 1307674368000.0))))))
    with np.errstate(all="ignore"):
        m_big = b / (2.0 * a) * ((1.0 - e) / (1.0 + e))
        v_big = b / (2.0 * a * a * a) * (((1.0 - e) * (1.0 + e) - 2.0 * a * e) / d)
    small = a < SERIES_BELOW
    return np.where(small, 0.25 * b * Tq, m_big), np.where(small, b * G * e / d, v_big)


def coef(n, x):
    """a_n(x) of the alternating series, on either side of T"""
    x = np.asarray(x, dtype=np.float64)
    h = n + 0.5
    k = PI * h
    with np.errstate(all="ignore"):
        w = 2.0 / (PI * x)
        left = k * (w * np.sqrt(w)) * np.exp(-2.0 * h * h / x)
        right = k * np.exp(-0.5 * k * k * x)
    return np.where(x <= T, left, right)


def tilt(z):
    """K, p, q of a draw at tilt z"""
    z = np.asarray(z, dtype=np.float64)
    K = PI * PI / 8.0 + 0.5 * z * z
    with np.errstate(all="ignore"):
        p = PI / (2.0 * K) * np.exp(-K * T)
        q = 2.0 * np.exp(-z) * (phi((T * z - 1.0) / 0.8) + np.exp(2.0 * z + log_phi(-(T * z + 1.0) / 0.8)))
    return K, p, q


def _rel(x, ref):
    """the relative margin |x - ref| / |ref| of a decision between x and ref (both 0: no close call)"""
    if x == ref:
        return INF if ref == 0.0 else 0.0
    return abs(x - ref) / abs(ref) if ref != 0.0 else INF


# ---- one observation at a time, on the oracle's Philox --------------------------------------------------------------------------------
# (coef, tilt and log Phi once more on Python floats: a chain of single draws spends its time here)
def _phi1(x):
    return 0.5 * math.erfc(-x / 1.4142135623730951)


def _log_phi1(x):
    if x >= 0.0:
        return math.log1p(-_phi1(-x))
    if x > -37.0:
        return math.log(_phi1(x))
    r = 1.0 / (x * x)
    ser = math.log1p(r * (-1.0 + r * (3.0 + r * (-15.0 + r * (105.0 + r * (-945.0 + r * (10395.0 + r * (-135135.0 + r * 2027025.0))))))))
    return -0.5 * x * x - math.log(-x) - HALF_LOG_2PI + ser


def _exp1(x):
    return math.exp(x) if x > -745.2 else 0.0


def _coef1(n, x):
    h = n + 0.5
    k = PI * h
    if x <= T:
        w = 2.0 / (PI * x)
        return k * (w * math.sqrt(w)) * _exp1(-2.0 * h * h / x)
    return k * _exp1(-0.5 * k * k * x)


def _tilt1(z):
    K = PI * PI / 8.0 + 0.5 * z * z
    p = PI / (2.0 * K) * _exp1(-K * T)
    q = 2.0 * _exp1(-z) * (_phi1((T * z - 1.0) / 0.8) + _exp1(2.0 * z + _log_phi1(-(T * z + 1.0) / 0.8)))
    return K, p, q


class Cursor:
    def __init__(self, seed, sweep, rel_tag, row):
        self.seed, self.sweep, self.ent, self.row, self.pair = int(seed), int(sweep), _entity(rel_tag), int(row), 0

    def _block(self):
        o = O.draw(self.seed, self.sweep, P_PG, self.ent, self.row, self.pair & 0xFFFF)
        self.pair += 1
        return o

    def uniform(self):
        o = self._block()
        return _u01(o[0], o[1])

    def expo(self):
        return -math.log(self.uniform())

    def expo2(self):
        o = self._block()
        return -math.log(_u01(o[0], o[1])), -math.log(_u01(o[2], o[3]))

    def normal(self):
        p = self.pair & 0xFFFF
        self.pair += 1
        return float(O.normals(self.seed, self.sweep, P_PG, self.ent, self.row, 2 * p + 1)[2 * p])


def jstar(z, cur):
    """X ~ J*(1, z) and the smallest decision margin"""
    K, p, q = _tilt1(z)
    X, margin = T, INF
    for _ in range(TRIES):
        u = cur.uniform()
        margin = min(margin, _rel(u * (p + q), p))
        if u * (p + q) < p:
            X = T + cur.expo() / K
        elif T * z < 1.0:
            for _c in range(TRIES):
                E, F = cur.expo2()
                margin = min(margin, _rel(E * E, 2.0 * F / T))
                if E * E > 2.0 * F / T:
                    continue
                g = 1.0 + T * E
                X = T / (g * g)
                v, a = cur.uniform(), _exp1(-0.5 * z * z * X)
                margin = min(margin, _rel(v, a))
                if v <= a:
                    break
        else:
            mu = 1.0 / z
            for _c in range(TRIES):
                N = cur.normal()
                Y = N * N
                X = mu + 0.5 * mu * mu * Y - 0.5 * mu * math.sqrt(4.0 * mu * Y + (mu * Y) * (mu * Y))
                v = cur.uniform()
                margin = min(margin, _rel(v, mu / (mu + X)))
                if v > mu / (mu + X):
                    X = mu * mu / X
                margin = min(margin, _rel(X, T))
                if X <= T:
                    break
            X = min(X, T)
        S = _coef1(0, X)
        y = cur.uniform() * S
        accept = True
        for n in range(1, TERMS):
            if n & 1:
                S -= _coef1(n, X)
                margin = min(margin, _rel(y, S))
                if y <= S:
                    break
            else:
                S += _coef1(n, X)
                margin = min(margin, _rel(y, S))
                if y > S:
                    accept = False
                    break
        if accept:
            return float(X), margin
    return float(X), margin


def pg(b, c, cur):
    """omega ~ PG(b, c), b a positive integer: the sum of b variates J*(1, |c| / 2) / 4 up to 170, the moment-matched normal above"""
    a = abs(float(c))
    if b > SUM_MAX:
        m, v = moments(float(b), a)
        return max(float(m) + float(np.sqrt(v)) * cur.normal(), TINY), INF
    s, margin = 0.0, INF
    for _ in range(int(b)):
        X, mg = jstar(0.5 * a, cur)
        s += X
        margin = min(margin, mg)
    return max(0.25 * s, TINY), margin


# ---- many observations at once --------------------------------------------------------------------------------------------------------
class Cursors:
    """one cursor per observation: rows[i] at sweep[i]; a request names the observations that take their next block"""

    def __init__(self, seed, sweep, rel_tag, rows):
        self.rows = np.asarray(rows, dtype=np.uint64)
        self.sweep = np.broadcast_to(np.asarray(sweep, dtype=np.uint64), self.rows.shape)
        self.pair = np.zeros(len(self.rows), dtype=np.uint64)
        self.k0, self.k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
        self.w = np.uint64((P_PG << 24) | _entity(rel_tag))
        self.margin = np.full(len(self.rows), INF)

    def _blocks(self, idx):
        row, pair = self.rows[idx], self.pair[idx] & np.uint64(0xFFFF)
        self.pair[idx] += np.uint64(1)
        c = [row & np.uint64(0xFFFFFFFF), ((row >> np.uint64(32)) & np.uint64(0xFFFF)) | (pair << np.uint64(16)), self.sweep[idx],
             np.full(len(idx), self.w, dtype=np.uint64)]
        o = _philox4x32_10(c, self.k0, self.k1)
        u1 = (((o[1] << np.uint64(32)) | o[0]) >> np.uint64(11)).astype(np.float64)
        u2 = (((o[3] << np.uint64(32)) | o[2]) >> np.uint64(11)).astype(np.float64)
        return (u1 + 0.5) * 2.0 ** -53, (u2 + 0.5) * 2.0 ** -53

    def uniform(self, idx):
        return self._blocks(idx)[0]

    def expo(self, idx):
        return -np.log(self._blocks(idx)[0])

    def expo2(self, idx):
        u1, u2 = self._blocks(idx)
        return -np.log(u1), -np.log(u2)

    def normal(self, idx):
        u1, u2 = self._blocks(idx)
        return np.sqrt(-2.0 * np.log(u1)) * np.cos(TWO_PI * u2)

    def decide(self, idx, x, ref):
        """record the margins of the decisions between x and ref"""
        with np.errstate(all="ignore"):
            m = np.abs(x - ref) / np.abs(ref)
        m = np.where(ref == 0.0, INF, m)
        np.minimum.at(self.margin, idx, m)


def _jstar_many(z, K, p, q, X, cur, idx):
    """one variate J*(1, z[i]) for every observation i in idx; X: the observations' last candidates (what stands at a bound)"""
    todo = np.asarray(idx)
    out = np.zeros(len(z))
    for _ in range(TRIES):
        if len(todo) == 0:
            break
        u = cur.uniform(todo)
        cur.decide(todo, u * (p[todo] + q[todo]), p[todo])
        right = u * (p[todo] + q[todo]) < p[todo]
        ir = todo[right]
        if len(ir):
            X[ir] = T + cur.expo(ir) / K[ir]
        small = ~right & (T * z[todo] < 1.0)
        pend = todo[small]
        for _c in range(TRIES):
            if len(pend) == 0:
                break
            E, F = cur.expo2(pend)
            cur.decide(pend, E * E, 2.0 * F / T)
            ok = ~(E * E > 2.0 * F / T)
            io = pend[ok]
            g = 1.0 + T * E[ok]
            X[io] = T / (g * g)
            v, a = cur.uniform(io), np.exp(-0.5 * z[io] * z[io] * X[io])
            cur.decide(io, v, a)
            fin = np.zeros(len(pend), dtype=bool)
            fin[ok] = v <= a
            pend = pend[~fin]
        pend = todo[~right & ~(T * z[todo] < 1.0)]
        il = pend
        for _c in range(TRIES):
            if len(pend) == 0:
                break
            mu = 1.0 / z[pend]
            N = cur.normal(pend)
            Y = N * N
            x = mu + 0.5 * mu * mu * Y - 0.5 * mu * np.sqrt(4.0 * mu * Y + (mu * Y) * (mu * Y))
            v = cur.uniform(pend)
            cur.decide(pend, v, mu / (mu + x))
            x = np.where(v > mu / (mu + x), mu * mu / x, x)
            cur.decide(pend, x, np.full(len(pend), T))
            X[pend] = x
            pend = pend[~(x <= T)]
        X[il] = np.minimum(X[il], T)
        x = X[todo]
        S = coef(0, x)
        y = cur.uniform(todo) * S
        state = np.zeros(len(todo), dtype=np.int8)          # 0 undecided, 1 accepted, 2 refused
        for n in range(1, TERMS):
            und = state == 0
            if not und.any():
                break
            a = coef(n, x[und])
            if n & 1:
                S[und] -= a
                cur.decide(todo[und], y[und], S[und])
                hit = y[und] <= S[und]
                state[np.nonzero(und)[0][hit]] = 1
            else:
                S[und] += a
                cur.decide(todo[und], y[und], S[und])
                hit = y[und] > S[und]
                state[np.nonzero(und)[0][hit]] = 2
        acc = state != 2
        out[todo[acc]] = x[acc]
        todo = todo[~acc]
    out[todo] = X[todo]                                      # (after TRIES refused proposals the last one is returned)
    return out


def draw_pg(psi, b, seed, sweep, rel_tag, rows=None):
    """omega_k ~ PG(b_k, psi_k) for observations rows[k] (default 0 .. n-1) at `sweep` (a scalar or one per observation) -> (omega,
    the smallest decision margin of every observation)"""
    psi = np.asarray(psi, dtype=np.float64)
    b = np.broadcast_to(np.asarray(b, dtype=np.float64), psi.shape)
    n = len(psi)
    cur = Cursors(seed, sweep, rel_tag, np.arange(n) if rows is None else rows)
    a = np.abs(psi)
    omega = np.zeros(n)
    big = np.nonzero(b > SUM_MAX)[0]
    if len(big):
        m, v = moments(b[big], a[big])
        omega[big] = np.maximum(m + np.sqrt(v) * cur.normal(big), TINY)
    z = 0.5 * a
    K, p, q = tilt(z)
    s, X = np.zeros(n), np.full(n, T)
    small = b <= SUM_MAX
    for i in range(int(b[small].max()) if small.any() else 0):
        idx = np.nonzero(small & (b > i))[0]
        s[idx] += _jstar_many(z, K, p, q, X, cur, idx)[idx]
        X[idx] = T                                           # (every variate starts from X = t)
    omega[small] = np.maximum(0.25 * s[small], TINY)
    return omega, cur.margin


# ---- whole iterations ------------------------------------------------------------------------------------------------------------------
def run_chain(ids, values, dims, D, seed, iters, model, r=0, offset=0.0, feats=None, use_ff=True, rel_tag=1, test_ids=None, burnin=0):
    """macau() on ONE logit (model 1) or count (model 2, dispersion r) relation (ids (n, n_modes) 1-based) between len(dims) entities,
    entity k with the dense side information feats[k] (or None).  Iterations 1 .. iters, each omega | U,V -> U | omega,V -> V |
    omega,U.  Returns {"S", "mu", "Lam", "beta", "lb", "omega", "linear", "margin"} after the last one ("margin": the smallest decision
    margin of all draws) and, with test_ids, "pred": the mean over iterations burnin + 1 .. iters of the link of udot + offset."""
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
    bb, kappa = b_of(model, values, r), kappa_of(model, values, r)
    pred, margin = None, INF
    omega = linear = None
    for it in range(1, iters + 1):
        psi = udot(ids, S) + offset
        omega, mg = draw_pg(psi, bb, seed, it, rel_tag)
        margin = min(margin, float(mg.min()))
        linear = linear_of(offset, values, kappa, omega)
        for j in range(n_modes):
            if ofe[j] is not None:
                uhat = np.stack([ofe[j].mul(beta[j][:, d]) for d in range(D)], axis=1)
                S[j] = RR.sample_rows(ids, values, omega, dims, j, 1.0, linear, S, mu[j] + uhat, Lam[j], seed, it, j + 1)
                U, nuh, Tinv = S[j] - uhat, D + ofe[j].n, np.eye(D) + beta[j].T @ beta[j] * lb[j]
            else:
                S[j] = RR.sample_rows(ids, values, omega, dims, j, 1.0, linear, S, mu[j], Lam[j], seed, it, j + 1)
                U, nuh, Tinv = S[j], float(D), np.eye(D)
            mu_N, beta_N, T_N, nu_N = O.hyper_params(U, np.zeros(D), 2.0, Tinv, nuh)
            mu[j], Lam[j] = O.hyper_draw(mu_N, beta_N, T_N, nu_N, seed, it, j + 1)
        for j in range(n_modes):
            if ofe[j] is not None:
                beta[j], _, _ = O.sample_beta(ofe[j], S[j], mu[j], Lam[j], lb[j], use_ff, None, seed, it, j + 1)
                lb[j] = O.sample_lambda_beta(beta[j], Lam[j], 1e-3, 1.0, seed, it, j + 1)
        if it > burnin and test_ids is not None:
            pr = link(model, udot(test_ids, S) + offset, r)
            pred = pr if pred is None else pred + pr
    out = {"S": S, "mu": mu, "Lam": Lam, "beta": beta, "lb": lb, "omega": omega, "linear": linear, "margin": margin}
    if pred is not None:
        out["pred"] = pred / (iters - burnin)
    return out


# ---- the cases the tests share ---------------------------------------------------------------------------------------------------------
def planted(kind, seed=0, N1=150, N2=100, rank=3, n_cells=5000, n_test=1500, r=5, scale=0.7, shift=-0.5):
    """planted data: distinct cells of an N1 x N2 matrix, psi* = scale u*.v* + shift with standard normal u*, v*; counts: y ~ NB(r, sigma(psi*)) with mean
    r e^psi*; logit: y ~ Bernoulli(sigma(psi*)).  The LAST n_test cells are held out.  Returns (ids, y, psi*, n_test)"""
    rng = np.random.default_rng(seed)
    cells = rng.choice(N1 * N2, size=n_cells, replace=False)
    ids = np.stack([cells // N2 + 1, cells % N2 + 1], axis=1).astype(np.int64)
    U, V = rng.standard_normal((N1, rank)), rng.standard_normal((N2, rank))
    psi = scale * (U[ids[:, 0] - 1] * V[ids[:, 1] - 1]).sum(axis=1) + shift
    if kind == "counts":
        # NB(r, p): a Poisson whose rate is Gamma(r, scale e^psi)
        y = rng.poisson(rng.gamma(r, np.exp(psi))).astype(np.float64)
    else:
        y = (rng.random(n_cells) < link(1, psi)).astype(np.float64)
    return ids, y, psi, n_test


def iteration_case(n_modes, with_feat, model):
    """the small relation of the whole-iteration test: (ids, values, dims, D, feats per entity, number of leading test cells, r,
    offset); about 600 cells drawn with replacement, so some repeat"""
    rng = np.random.default_rng(90 + n_modes + 10 * model)
    dims = [30, 24, 10][:n_modes]
    n, D, n_test = 600, 4, 60
    ids = np.stack([rng.integers(1, d + 1, n) for d in dims], axis=1).astype(np.int64)
    for k, d in enumerate(dims):
        ids[:d, k] = np.arange(1, d + 1)                  # every id occurs: the entities have exactly dims rows
    if model == 1:
        y, r, offset = (rng.random(n) < 0.4).astype(np.float64), 0, -0.2
    else:
        y, r, offset = rng.poisson(rng.gamma(3, 0.8, n)).astype(np.float64), 3, 0.1
    feats = [None] * n_modes
    if with_feat:
        feats[0] = rng.standard_normal((dims[0], 5))
    return ids, y, dims, D, feats, n_test, r, offset
