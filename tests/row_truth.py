"""Exact answers for the latent-row samplers (host only: numpy and mpmath, never the device).

The CPU oracle follows the reference's words -- inv(P) by LU, then chol(inv(P)) -- and loses about 4 D kappa u at cond(P) ~ 1e8, so
it cannot say how accurate a row kernel is there.  This module states the two maps in mpmath instead:

  the reference's map   x = chol(inv(P)) z + inv(P) b (lower chol).  With J the index reversal and J P J = R R' the lower Cholesky,
                        chol(inv(P)) = J R^-T J: inv(P) = J R^-T R^-1 J = (J R^-T J)(J R^-T J)', and J R^-T J is lower triangular with a
                        positive diagonal.  So x = J R^-T (J z + R^-1 J b): one Cholesky and two triangular solves, no inverse.
  the low-rank map      Lambda = L L',  wt_o = sqrt(alpha_o) L^-1 w_o,  e0 = L' mu + u,  G = I + Wt Wt',
                        tau = G^-1 (rt - Wt e0 - delta),  x = L^-T (e0 + Wt' tau)      (k_rows_lr.hip, orc_sample_row_lowrank)

with P = Lambda + sum alpha_o w_o w_o', b = Lambda mu + sum alpha_o (y_o - mean) w_o formed in mpmath from the float64 inputs (every
float64 is an exact mpf), the observations in the index's order (by row, then the caller's order), alpha_o = alpha omega_o.

The yardsticks are the same algorithms in float64 on the CPU: for the reference's map numpy's P and b, np.linalg.cholesky of the
reversed P and the same solves; for the low-rank map the oracle's sample_row_lowrank.  check() holds a sampler to the derived forward
bound 8 D kappa u and to 16 times the yardstick's own error.

The cases are fixed by their parameters (a seed derived from them) and their arrays are read-only.
"""
import zlib

import numpy as np
from mpmath import mp, mpf

U = 2.0 ** -52
DPS = 40

# kind -> (alpha, fewest observations of a row, most); None: depends on D (see _count_range)
KINDS = ("plain", "prior", "alpha", "collinear", "weights", "long")
LONG_ROWS = (65, 150, 300)
# cond_2(P) every row of a kind must lie in (conditions on the inputs, asserted on the host)
KAPPA_RANGE = {"plain": (1.0, 1e3), "prior": (1e4, 1e9), "alpha": (1e6, 1e10), "collinear": (1e6, 1e10)}


def _count_range(kind, D):
    """observations per row of a kind.  `prior` rows take at most min(5, (D - 1) // 3): k observations lift k directions, and by
    Cauchy's interlacing the smallest eigenvalue of P is then at most the (k + 1)-th smallest of Lambda, 10^(-6 + 6 k / (D - 1));
    that is 1e-4 or less -- cond_2(P) of 1e4 or more, whatever the items -- for k <= (D - 1) / 3."""
    return {"plain": (0, 60), "prior": (0, min(5, (D - 1) // 3)), "alpha": (1, D - 1), "collinear": (D, 60), "weights": (10, 40),
            "long": (min(LONG_ROWS), max(LONG_ROWS))}[kind]


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.flags.writeable = False
    return a


class TermData:
    """one relation of the sampled entity (mode 0 of a two-mode relation): ids (nnz, 2) 1-based and sorted by row, values, the
    opposite entity's factors V (M, D), alpha, mean, obs_precision (nnz) or None"""

    def __init__(self, ids, vals, V, alpha, mean, omega=None):
        self.ids, self.vals, self.V = _frozen(ids.astype(np.int64)), _frozen(vals), _frozen(V)
        self.alpha, self.mean = float(alpha), float(mean)
        self.omega = None if omega is None else _frozen(omega)
        self.M = V.shape[0]


class Case:
    def __init__(self, key, kind, D, N, Lam, mu, mu_rows, terms):
        self.key, self.kind, self.D, self.N = key, kind, D, N
        self.Lam, self.mu, self.mu_rows, self.terms = _frozen(Lam), _frozen(mu), _frozen(mu_rows), terms
        self.counts = _frozen(sum(np.bincount(t.ids[:, 0] - 1, minlength=N) for t in terms))
        # the index's order: by row, then the caller's (COO) order
        self._order = [np.argsort(t.ids[:, 0], kind="stable") for t in terms]
        self._ptr = [np.concatenate([[0], np.cumsum(np.bincount(t.ids[:, 0] - 1, minlength=N))]) for t in terms]

    def row_obs(self, row):
        """the observations of a row, term after term, each in the index's order: W (n, D) gathered factors, alpha (n) the term's
        alpha, omega (n) the observation's precision weight (1 without), y (n) values, base (n) the term's mean -- the float64 inputs
        themselves, no arithmetic done on them"""
        W, al, om, y, base = [np.zeros((0, self.D))], [np.zeros(0)], [np.zeros(0)], [np.zeros(0)], [np.zeros(0)]
        for t, order, ptr in zip(self.terms, self._order, self._ptr):
            o = order[ptr[row]:ptr[row + 1]]
            W.append(t.V[t.ids[o, 1] - 1])
            al.append(np.full(len(o), t.alpha))
            om.append(np.ones(len(o)) if t.omega is None else t.omega[o])
            y.append(t.vals[o])
            base.append(np.full(len(o), t.mean))
        return tuple(np.concatenate(v) for v in (W, al, om, y, base))

    def row_obs_f64(self, row):
        """(W, a = alpha omega, r = y - mean) in float64: what a float64 sampler starts from"""
        W, al, om, y, base = self.row_obs(row)
        return W, al * om, y - base

    def row_obs_mp(self, row):
        """(columns of W, a, r) in mpmath: the product and the difference exact up to the working precision"""
        W, al, om, y, base = self.row_obs(row)
        return [_v(W[:, j]) for j in range(self.D)], [p * q for p, q in zip(_v(al), _v(om))], [p - q for p, q in zip(_v(y), _v(base))]

    def mean_of(self, row, per_row):
        return self.mu_rows[row] if per_row else self.mu


def _plain_lambda(rng, D):
    A = rng.standard_normal((D, D))
    return A @ A.T / D + np.eye(D)


def prior_lambda(rng, D):
    """eigenvalues logspace(-6, 0, D) in a random orthogonal basis, symmetric to the last bit"""
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    L = (Q * np.logspace(-6, 0, D)) @ Q.T
    return (L + L.T) / 2


def _rows_of(rng, counts, M, same=False):
    """ids (nnz, 2) with counts[i] distinct items in row i, sorted by row; same: every row lists the same items (a block)"""
    rows = np.repeat(np.arange(1, len(counts) + 1), counts)
    if same:
        assert len(set(counts)) == 1
        items = np.tile(np.sort(rng.choice(M, size=counts[0], replace=False)) + 1, len(counts))
    else:
        items = np.concatenate([rng.choice(M, size=c, replace=False) + 1 for c in counts] + [np.zeros(0, dtype=np.int64)])
    return np.stack([rows, items], axis=1).astype(np.int64)


_CASES = {}


def make_case(kind, D, N, nobs=None, second=False, M=None, block=False, short_row=None):
    """The case of a kind (module docstring of the table: tests/test_gpu_row_conditioning.py) at D with N rows; nobs = (lo, hi) narrows the
    kind's observations per row to what a kernel takes; second: one more relation on the entity (0 .. 20 observations, alpha 0.7,
    mean -0.3, factors of its own); block: nobs = (nv, nv) and every row lists the same nv items (bdf_sample_block's users); short_row: the
    middle row has that many observations instead."""
    key = (kind, D, N, nobs, second, M, block, short_row)
    if key in _CASES:
        return _CASES[key]
    assert kind in KINDS
    rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
    M = M or (320 if kind == "long" else 60)
    lo, hi = _count_range(kind, D)
    if nobs is not None:
        lo, hi = max(lo, nobs[0]), min(hi, nobs[1])
    hi = min(hi, M)
    assert lo <= hi, (key, lo, hi)
    if kind == "long":
        counts = np.array([LONG_ROWS[i % 3] for i in range(N)])
    else:
        counts = rng.integers(lo, hi + 1, N)
        counts[0], counts[N - 1] = lo, hi
        if short_row is not None:
            counts[N // 2] = short_row
    assert not block or lo == hi
    Lam = prior_lambda(rng, D) if kind == "prior" else _plain_lambda(rng, D)
    alpha = {"plain": 2.0, "prior": 2.0, "alpha": 1e7, "collinear": 1e5, "weights": 1.0, "long": 2.0}[kind]
    if kind == "collinear":
        # every item is v up to 1e-3: v's entries have magnitude 2 .. 3, so that alpha n |v|^2 is at least 1e6 at D = 3
        v = rng.uniform(2.0, 3.0, D) * rng.choice([-1.0, 1.0], D)
        V = np.outer(np.ones(M), v) + 1e-3 * rng.standard_normal((M, D))
    else:
        V = 0.5 * rng.standard_normal((M, D))
    if kind == "alpha":
        # A row has fewer than D observations, so some x is orthogonal to all of them and lambda_min(P) <= lambda_max(Lambda), while
        # lambda_max(P) >= alpha |w|^2 for any of its items w: cond_2(P) >= alpha |w|^2 / lambda_max(Lambda).  Items shorter than
        # sqrt(lambda_max(Lambda) / 5) are stretched to that length (at D = 3 about half of them are), which makes it 2e6 or more
        # whatever the seed.
        floor = np.sqrt(np.linalg.eigvalsh(Lam)[-1] / 5)
        norms = np.linalg.norm(V, axis=1)
        V = V * np.maximum(1.0, floor / norms)[:, None]
    c2 = None
    if second:
        # (a `prior` row's observations are counted over both relations: the second one takes some of the first one's)
        c2 = rng.integers(0, counts + 1) if kind == "prior" else rng.integers(0, 21, N)
        if kind == "prior":
            counts = counts - c2
    ids = _rows_of(rng, counts, M, same=block)
    vals = rng.standard_normal(len(ids)) + 0.25
    omega = np.exp(rng.uniform(np.log(1e-6), np.log(1e6), len(ids))) if kind == "weights" else None
    if omega is not None:
        omega[0], omega[-1] = 1e-6, 1e6
    terms = [TermData(ids, vals, V, alpha, 0.25, omega)]
    if second:
        ids2 = _rows_of(rng, c2, 45)
        terms.append(TermData(ids2, rng.standard_normal(len(ids2)) - 0.3, 0.5 * rng.standard_normal((45, D)), 0.7, -0.3))
    case = Case(key, kind, D, N, Lam, rng.standard_normal(D), rng.standard_normal((N, D)), terms)
    _CASES[key] = case
    return case


# ---- mpmath: exact float64 -> mpf, Cholesky and the two triangular solves on lists (mp.fdot keeps the inner loops in libmp) ------------
def _v(a):
    return [mpf(float(x)) for x in a]


def _m(A):
    return [_v(r) for r in A]


def chol_mp(A):
    """lower Cholesky factor of a symmetric positive definite list-of-lists matrix (rows of the lower triangle are read)"""
    n = len(A)
    L = [[mpf(0)] * n for _ in range(n)]
    for j in range(n):
        Lj = L[j][:j]
        s = A[j][j] - mp.fdot(Lj, Lj)
        if not s > 0:
            raise ArithmeticError("matrix is not positive definite")
        d = mp.sqrt(s)
        L[j][j] = d
        for i in range(j + 1, n):
            L[i][j] = (A[i][j] - mp.fdot(L[i][:j], Lj)) / d
    return L


def solve_lower(L, c):
    """y with L y = c"""
    y = []
    for i in range(len(c)):
        y.append((c[i] - mp.fdot(L[i][:i], y)) / L[i][i])
    return y


def solve_lower_t(L, c):
    """t with L' t = c"""
    n = len(c)
    t = [mpf(0)] * n
    for i in range(n - 1, -1, -1):
        t[i] = (c[i] - mp.fdot([L[k][i] for k in range(i + 1, n)], t[i + 1:])) / L[i][i]
    return t


def exact_system(case, row, per_row):
    """(P as a list of lists, b as a list) of a row in mpmath at the working precision"""
    D = case.D
    Wc, am, rm = case.row_obs_mp(row)
    Lam, mu = _m(case.Lam), _v(case.mean_of(row, per_row))
    aWc = [[x * y for x, y in zip(am, col)] for col in Wc]
    P = [[None] * D for _ in range(D)]
    for i in range(D):
        for j in range(i + 1):
            P[i][j] = P[j][i] = Lam[i][j] + mp.fdot(aWc[i], Wc[j])
    b = [mp.fdot(Lam[i], mu) + mp.fdot(aWc[i], rm) for i in range(D)]
    return P, b


def ref_sample_from(R, b, z):
    """x = J R^-T (J z + R^-1 J b) with R the lower Cholesky factor of J P J"""
    y = solve_lower(R, b[::-1])
    zr = _v(z)[::-1]
    return solve_lower_t(R, [p + q for p, q in zip(y, zr)])[::-1]


def ref_sample_literal(P, b, z):
    """the reference's words in mpmath: covar = inv(P), x = chol(covar) z + covar b with the lower factor"""
    D = len(b)
    C = mp.inverse(mp.matrix(P))
    C = (C + C.T) / 2
    Lc = mp.cholesky(C)
    x = Lc * mp.matrix(_v(z)) + C * mp.matrix(b)
    return [x[i] for i in range(D)]


def lowrank_sample_exact(case, row, per_row, z, L=None):
    """the low-rank map of a row in mpmath; z: D + n float64 normals (u, then delta in the observations' order)"""
    D = case.D
    Wc, am, rm = case.row_obs_mp(row)
    n = len(am)
    L = chol_mp(_m(case.Lam)) if L is None else L
    mu, zz = _v(case.mean_of(row, per_row)), _v(z)
    sa = [mp.sqrt(x) for x in am]
    Wt = [[s * x for x in solve_lower(L, [Wc[d][o] for d in range(D)])] for o, s in enumerate(sa)]
    rt = [s * x for s, x in zip(sa, rm)]
    e0 = [mp.fdot([L[i][d] for i in range(d, D)], mu[d:]) + zz[d] for d in range(D)]
    q = e0
    if n:
        G = [[(1 if i == j else 0) + mp.fdot(Wt[i], Wt[j]) for j in range(n)] for i in range(n)]
        LG = chol_mp(G)
        rho = [rt[i] - mp.fdot(Wt[i], e0) - zz[D + i] for i in range(n)]
        tau = solve_lower_t(LG, solve_lower(LG, rho))
        q = [e0[d] + mp.fdot([Wt[o][d] for o in range(n)], tau) for d in range(D)]
    return solve_lower_t(L, q)


def _f64(x):
    return np.array([float(t) for t in x])


class Truth:
    """per case: the exact factors of every row's reversed P (they do not depend on the prior mean or the normals), the float64 P and
    kappa, and the exact samples for given normals"""
    _cache = {}

    @classmethod
    def of(cls, case, dps=DPS):
        k = (case.key, dps)
        if k not in cls._cache:
            cls._cache[k] = cls(case, dps)
        return cls._cache[k]

    def __init__(self, case, dps):
        self.case, self.dps = case, dps
        self.R, self.kappa, self.min_pivot, self.max_P = [], np.zeros(case.N), np.zeros(case.N), np.zeros(case.N)
        self._b, self._L, self._samples = {}, None, {}
        with mp.workdps(dps):
            for row in range(case.N):
                P, _ = exact_system(case, row, False)
                R = chol_mp([r[::-1] for r in P[::-1]])
                self.R.append(R)
                P64 = np.array([[float(x) for x in r] for r in P])
                self.kappa[row] = np.linalg.cond(P64)
                self.max_P[row] = np.abs(P64).max()
                self.min_pivot[row] = float(min(R[i][i] for i in range(case.D)) ** 2)

    def rhs(self, row, per_row):
        """b of a row in mpmath (cached; under the truth's precision)"""
        if (row, per_row) not in self._b:
            self._b[(row, per_row)] = exact_system_rhs(self.case, row, per_row)
        return self._b[(row, per_row)]

    def ref_samples(self, z, per_row):
        """the exact sample of the reference's map for the normals z (N, D), rounded to float64; cached per (z, per_row)"""
        k = ("ref", per_row, z.tobytes())
        if k not in self._samples:
            with mp.workdps(self.dps):
                self._samples[k] = _frozen(np.stack([_f64(ref_sample_from(self.R[row], self.rhs(row, per_row), z[row]))
                                                     for row in range(self.case.N)]))
        return self._samples[k]

    def lowrank_samples(self, zs, per_row):
        """the exact sample of the low-rank map; zs: per row its D + n normals; cached"""
        k = ("lr", per_row, b"".join(np.asarray(z).tobytes() for z in zs))
        if k not in self._samples:
            with mp.workdps(self.dps):
                if self._L is None:
                    self._L = chol_mp(_m(self.case.Lam))
                self._samples[k] = _frozen(np.stack([_f64(lowrank_sample_exact(self.case, row, per_row, zs[row], self._L))
                                                     for row in range(self.case.N)]))
        return self._samples[k]

    def lowrank_kappa(self):
        """max(cond_2(Lambda), cond_2(G)) per row: what the low-rank map's error follows"""
        case = self.case
        kl = np.linalg.cond(case.Lam)
        Lc = np.linalg.cholesky(case.Lam)
        out = np.zeros(case.N)
        for row in range(case.N):
            W, a, _ = case.row_obs_f64(row)
            Wt = np.linalg.solve(Lc, W.T).T * np.sqrt(a)[:, None] if len(a) else np.zeros((0, case.D))
            out[row] = max(kl, np.linalg.cond(np.eye(len(a)) + Wt @ Wt.T) if len(a) else 1.0)
        return out


def exact_system_rhs(case, row, per_row):
    Wc, am, rm = case.row_obs_mp(row)
    Lam, mu = _m(case.Lam), _v(case.mean_of(row, per_row))
    return [mp.fdot(Lam[i], mu) + mp.fdot([x * y for x, y in zip(am, Wc[i])], rm) for i in range(case.D)]


# ---- the float64 yardsticks (CPU) ---------------------------------------------------------------------------------------------------------
def system_f64(case, row, per_row):
    W, a, r = case.row_obs_f64(row)
    P = case.Lam + (W * a[:, None]).T @ W
    b = case.Lam @ case.mean_of(row, per_row) + W.T @ (a * r)
    return P, b


def _solve_lower_f64(L, c):
    y = np.zeros(len(c))
    for i in range(len(c)):
        y[i] = (c[i] - L[i, :i] @ y[:i]) / L[i, i]
    return y


def _solve_lower_t_f64(L, c):
    n = len(c)
    t = np.zeros(n)
    for i in range(n - 1, -1, -1):
        t[i] = (c[i] - L[i + 1:, i] @ t[i + 1:]) / L[i, i]
    return t


def ref_sample_f64(P, b, z):
    """the yardstick of the reference's map: a plain float64 Cholesky of the reversed P and the same two solves"""
    R = np.linalg.cholesky(P[::-1, ::-1])
    return _solve_lower_t_f64(R, _solve_lower_f64(R, b[::-1]) + z[::-1])[::-1]


def ref_yardstick(case, z, per_row):
    return np.stack([ref_sample_f64(*system_f64(case, row, per_row), z[row]) for row in range(case.N)])


def oracle_term(O, t, N, D):
    return O.Term(t.ids, t.vals, [N, t.M], 0, t.alpha, t.mean, [None, t.V])


def lowrank_yardstick(O, case, zs, per_row):
    """the oracle's own sample_row_lowrank: the algorithm the kernel follows, in float64"""
    assert all(t.omega is None for t in case.terms)
    ot = [oracle_term(O, t, case.N, case.D) for t in case.terms]
    return np.stack([O.sample_row_lowrank(case.D, ot, row, case.mean_of(row, per_row), case.Lam, zs[row]) for row in range(case.N)])


def oracle_samples(O, case, z, per_row):
    """the oracle's literal route (inv by LU, chol of the inverse) on the same normals: printed beside the yardstick, never the judge"""
    assert all(t.omega is None for t in case.terms)
    ot = [oracle_term(O, t, case.N, case.D) for t in case.terms]
    return np.stack([O.sample_row(case.D, ot, row, case.mean_of(row, per_row), case.Lam, z[row])[0] for row in range(case.N)])


# ---- the check ---------------------------------------------------------------------------------------------------------------------------
def row_errors(x, truth):
    """max |x - truth| / max |truth| per row"""
    return np.abs(x - truth).max(axis=1) / np.abs(truth).max(axis=1)


def derived_bound(D, kappa, n=0):
    """the forward bound 8 D kappa u; (8 D + n) kappa u for rows of n > 64 observations, whose P carries n u from its own sum"""
    n = np.asarray(n)
    return (8 * D + np.where(n > 64, n, 0)) * np.asarray(kappa) * U


def figures(D, kappa, x, truth):
    """worst error / (D kappa u) over the rows: the figure the tests print"""
    return float((row_errors(x, truth) / (D * np.asarray(kappa) * U)).max())


def check(what, D, kappa, x, truth, yard, n=0):
    """The two assertions on the rows x (rows, D) of a sampler against the exact rows `truth`, with the float64 yardstick's rows `yard`
    on the same inputs; kappa per row (or one number), n observations per row (or one number).
      derived bound        max |x - truth| / max |truth| <= 8 D kappa u per row ((8 D + n) kappa u for n > 64)
      against the yardstick  the worst error over the rows <= 16 max(the yardstick's worst error over the same rows, D u)
    Prints the worst error / (D kappa u) of x and of the yardstick; returns the two figures."""
    x, truth, yard = np.asarray(x), np.asarray(truth), np.asarray(yard)
    kappa = np.broadcast_to(np.asarray(kappa, dtype=np.float64), (len(truth),))
    assert np.all(np.isfinite(x)), what
    err, yerr = row_errors(x, truth), row_errors(yard, truth)
    bound = derived_bound(D, kappa, n)
    fx, fy = float((err / (D * kappa * U)).max()), float((yerr / (D * kappa * U)).max())
    print(f"{what}: kappa up to {kappa.max():.3g}; worst error / (D kappa u): sampler {fx:.3g}, yardstick {fy:.3g}; "
          f"worst error: sampler {err.max():.3g}, yardstick {yerr.max():.3g}")
    worst = int(np.argmax(err / bound))
    assert np.all(err <= bound), (what, "derived bound", worst, err[worst], bound[worst])
    assert err.max() <= 16 * max(yerr.max(), D * U), (what, "16 x yardstick", err.max(), yerr.max(), D * U)
    return fx, fy


# ---- |L^-1 v|^2 (bdf_newrows_quad) --------------------------------------------------------------------------------------------------------
def quad_exact(Lam, V, dps=DPS):
    """q_j = |L^-1 v_j|^2, Lambda = L L', in mpmath, rounded to float64"""
    with mp.workdps(dps):
        L = chol_mp(_m(Lam))
        out = []
        for v in V:
            t = solve_lower(L, _v(v))
            out.append(float(mp.fdot(t, t)))
    return np.array(out)


def quad_f64(Lam, V):
    """the float64 route: numpy's Cholesky, a forward substitution per row, the squares added"""
    L = np.linalg.cholesky(Lam)
    return np.array([float(np.sum(_solve_lower_f64(L, v) ** 2)) for v in V])


# ---- the cases of tests/test_gpu_row_conditioning.py (the host test holds the same ones to their conditions) -----------------------------
def n_rows(D):
    """26 rows (no multiple of four: the last wave of the four-rows-to-a-wave kernels is ragged); 7 at D >= 48, where a row's truth costs most"""
    return 26 if D < 48 else 7


def lr_limit(D):
    return min(16, D // 2)


def lr32_limit(D):
    return min(32, D // 2)


def route_cases():
    """[(route, kind, D, nobs | None, second)]: every kind a route can take at each of its D"""
    out = []
    for D in (8, 16, 24, 33, 64):
        out += [("k1", k, D, None, False) for k in ("plain", "prior", "alpha", "collinear", "long") if not (k == "collinear" and D > 60)]
    for D in (8, 24, 64):
        out += [("k1", k, D, None, True) for k in ("plain", "prior", "alpha", "collinear") if not (k == "collinear" and D > 60)]
        out += [("k1", "weights", D, None, False), ("k1", "weights", D, None, True)]
    for D in (3, 8, 16):
        # (at D = 3 a `prior` row keeps cond_2(P) >= 1e4 only without observations, and an entity without any is no relation)
        out += [("k1s", k, D, (0, 48), False) for k in ("plain", "prior", "alpha", "collinear") if not (k == "prior" and D == 3)]
    for D in (17, 24, 32):
        out += [("k1c", k, D, None, False) for k in ("plain", "prior", "alpha", "collinear", "long")]
    out += [("k1c_noimage", k, 32, None, False) for k in ("plain", "prior", "alpha", "collinear", "long")]
    for D in (24, 32, 48, 64):
        out += [("lr", k, D, (0, lr_limit(D)), False) for k in ("plain", "prior", "alpha")]
    for D in (48, 64):
        out += [("lr32", k, D, (17, lr32_limit(D)), False) for k in ("plain", "alpha")]       # (and one short row: case_of)
    return out


def case_of(route, kind, D, nobs, second):
    """lr32: the library switches the low-rank sampler on for an entity only if it has a row of at most min(16, D / 2) observations,
    so one row of 8 stands among the rows of 17 and more"""
    return make_case(kind, D, n_rows(D), nobs=nobs, second=second, short_row=8 if route == "lr32" else None)


def block_cases():
    """[(kind, D, nv, nu)]: bdf_sample_block's users share their nv items; a kind is taken where nv lies in its range"""
    out = []
    for D in (8, 24, 64):
        for nv in (1, 7, 9, 40):
            for nu in (1, 5):
                for kind in ("plain", "prior", "alpha", "collinear"):
                    lo, hi = _count_range(kind, D)
                    if lo <= nv <= hi:
                        out.append((kind, D, nv, nu))
    return out
