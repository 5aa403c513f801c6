"""The row samplers on ill-conditioned systems against exact solves (tests/row_truth.py).

The other GPU tests compare the row kernels with the CPU oracle at 1e-8 on systems with cond(P) of a few hundred; the oracle itself
(inv by LU, chol of the inverse) is off by 1e-5 at cond(P) ~ 1e8, so neither says how accurate a kernel is.  Here every row path
-- K1 (k_sample_rows.hip: whole rows, split rows, two relations, obs_precision), K1s (k_rows_small.hip), K1c (k_rows_col.hip, with
and without the gather image), K1-lr and lr32 (k_rows_lr.hip) and bdf_sample_block (k_block.hip) -- takes one launch per case with
its routing forced and checked (bdf_ctx_rows_dispatch), and its rows are held to the exact sample of the same map in mpmath:

  derived bound          max |x - truth| / max |truth| <= 8 D kappa u per row ((8 D + n) kappa u at n > 64 observations)
  against the yardstick  the worst error over the case's rows <= 16 max(the float64 CPU yardstick's worst error, D u)

kappa = cond_2(P) for the reference's map, max(cond_2(Lambda), cond_2(G)) for the low-rank map.  The kinds (row_truth.make_case):

  plain      Lambda = A A'/D + I, alpha 2, 0 .. 60 observations            cond_2(P) <= 1e3
  prior      Lambda's eigenvalues logspace(-6, 0, D), alpha 2, 0 .. 5     1e4 .. 1e9
  alpha      plain Lambda, alpha 1e7, 1 .. D - 1 observations              1e6 .. 1e10
  collinear  alpha 1e5, D .. 60 observations of items v + 1e-3 N(0, 1)      1e6 .. 1e10
  weights    alpha 1, 10 .. 40 observations, obs_precision log-uniform in 1e-6 .. 1e6 (K1 only)
  long       rows of 65, 150 and 300 observations of 320 items: K1 splits them (item size 64), K1c spans waves

each with a shared and with a per-row prior mean.  Beside them: the dump (bdf_row_system) against the exact P and c componentwise,
bdf_newrows_quad with the `prior` Lambda, and the not-positive-definite flag of every row path.  Every test prints the worst
error / (D kappa u) of the device and of the yardstick ("accuracy of the row samplers").
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import row_truth as T

pytestmark = pytest.mark.gpu

SEED = 1234
SWEEP = 3
GUARD = 16
_tags = itertools.count(7000)          # a tag of its own per launch: the dispatch report of one (tag, sweep) adds up


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


@pytest.fixture(scope="module")
def rctx(B):
    """a context of this file's own: the routing it forces never reaches the other files' launches"""
    c = B.Context(seed=SEED)
    yield c
    c.close()


def _route(ctx, route):
    if route == "k1":
        ctx.set_small_rows(0, 8192); ctx.set_lowrank(0, 0); ctx.set_col_rows(0)
    elif route == "k1s":
        ctx.set_small_rows(48, 0)
    elif route in ("k1c", "k1c_noimage"):
        ctx.set_col_rows(64); ctx.set_lowrank(0, 0); ctx.set_gather_image(0 if route == "k1c_noimage" else 1)
    elif route in ("lr", "lr32"):
        ctx.set_lowrank(-1, 0)
    else:
        raise ValueError(route)


def _restore(ctx):
    ctx.set_small_rows(48, 8192); ctx.set_lowrank(-1, 8192); ctx.set_col_rows(-1); ctx.set_gather_image(1)


def _dispatched(route, case, disp):
    """every row went to the kernel the test is named for"""
    N = case.N
    want = {"k1": "k1", "k1s": "small", "k1c": "col", "k1c_noimage": "col", "lr": "lowrank", "lr32": "lowrank"}[route]
    assert disp is not None and disp[want] == N and sum(disp[k] for k in ("lowrank", "small", "col", "k1")) == N, (route, disp)
    if case.kind == "long":
        if route == "k1":
            assert disp["k1_items"] > N, disp                  # rows of more than 64 observations in pieces
        else:
            assert disp["col_waves"] > -(-N // 4), disp        # a row of 300 observations spans waves at pieces of 64


class Dev:
    """a case on the device: its relations, factors and weights, the terms of one launch"""

    def __init__(self, B, ctx, case, Lam=None):
        from bdf_amd._lib import Term
        self.ctx, self.case, self.rels, self.keep = ctx, case, [], []
        self.terms = (Term * len(case.terms))()
        for k, t in enumerate(case.terms):
            dr = B.DeviceRelation(ctx, B.IndexedDF((np.array(t.ids), np.array(t.vals)), [case.N, t.M]))
            V = ctx.tensor(np.array(t.V))
            om = ctx.tensor(np.array(t.omega)) if t.omega is not None else None
            self.rels.append(dr)
            self.keep += [V, om]
            self.terms[k].rel, self.terms[k].mode, self.terms[k].alpha, self.terms[k].mean_value = dr.handle, 0, t.alpha, t.mean
            self.terms[k].factors[1] = V.data_ptr()
            self.terms[k].obs_precision = om.data_ptr() if om is not None else None
        self.Lam = ctx.tensor(np.array(case.Lam if Lam is None else Lam))
        self.mu = {False: ctx.tensor(np.array(case.mu)), True: ctx.tensor(np.array(case.mu_rows))}

    def sample(self, per_row, tag):
        """one launch of bdf_sample_rows at sweep SWEEP -> (return code, the out tensor with GUARD rows of NaN behind its N)"""
        from bdf_amd._lib import lib
        case, ctx = self.case, self.ctx
        out = ctx.tensor(np.full((case.N + GUARD, case.D), np.nan))
        ctx.set_sweep(SWEEP)
        rc = lib().bdf_sample_rows(ctx.handle, case.D, case.N, len(self.terms), self.terms, _p(self.mu[per_row]), int(per_row), _p(self.Lam),
                                   tag, 0, 1, _p(out), None)
        return rc, out

    def normals(self, tag):
        """the D normals of every row's stream (BDF_P_ROW, tag, row) at sweep SWEEP, from the device (bdf_normals)"""
        from bdf_amd._lib import check, lib
        z = self.ctx.zeros(self.case.N, self.case.D)
        self.ctx.set_sweep(SWEEP)
        check(lib().bdf_normals(self.ctx.handle, 1, tag, 0, self.case.N, self.case.D, _p(z)))
        self.ctx.sync()
        return z.cpu().numpy()

    def close(self):
        for dr in self.rels:
            dr.close()


_NAN_BITS = np.array([np.nan]).view(np.int64)[0]


def _guard_untouched(out):
    g = out[-GUARD:]
    assert np.isnan(g).all() and np.all(g.view(np.int64) == _NAN_BITS)


def _run_case(B, O, ctx, route, case, what):
    """both prior means of a case through one forced route: dispatch, guard rows, the two assertions of row_truth.check"""
    from bdf_amd._lib import check
    tr = T.Truth.of(case)
    lowrank = route in ("lr", "lr32")
    kappa = tr.lowrank_kappa() if lowrank else tr.kappa
    dev = Dev(B, ctx, case)
    figs = []
    try:
        _route(ctx, route)
        for per_row in (False, True):
            tag = next(_tags)
            rc, out_t = dev.sample(per_row, tag)
            check(rc)
            ctx.sync()
            out = out_t.cpu().numpy()
            _dispatched(route, case, ctx.rows_dispatch(tag))
            assert ctx.rows_unfinished() == 0
            _guard_untouched(out)
            if lowrank:
                zs = [O.lowrank_normals(SEED, SWEEP, tag, row, case.D, int(case.counts[row])) for row in range(case.N)]
                exact, yard = tr.lowrank_samples(zs, per_row), T.lowrank_yardstick(O, case, zs, per_row)
            else:
                z = dev.normals(tag)
                exact, yard = tr.ref_samples(z, per_row), T.ref_yardstick(case, z, per_row)
            figs.append(T.check(f"{what} {'per-row' if per_row else 'shared'} mean", case.D, kappa, out[:case.N], exact, yard, case.counts))
    finally:
        _restore(ctx)
        dev.close()
    return figs


_ROUTES = T.route_cases()


@pytest.mark.parametrize("route,kind,D,nobs,second", _ROUTES,
                         ids=[f"{r}-{k}-{D}{'-two' if s else ''}" for r, k, D, _, s in _ROUTES])
def test_rows_against_exact_samples(B, O, rctx, route, kind, D, nobs, second):
    """one launch per prior mean through the forced route; the rows against the exact sample of the same map"""
    case = T.case_of(route, kind, D, nobs, second)
    if route == "lr32":
        rest = np.delete(case.counts, case.N // 2)          # (one short row switches the low-rank sampler on: row_truth.case_of)
        assert rest.min() >= 17 and rest.max() <= T.lr32_limit(D) and case.counts[case.N // 2] <= T.lr_limit(D)
    if route == "lr":
        assert case.counts.max() <= T.lr_limit(D)
    if route == "k1" and kind == "long":
        ctx = B.Context(seed=SEED)         # (an item size, once chosen, stays with its context: one of this test's own)
        ctx.set_item_size(64)
        try:
            _run_case(B, O, ctx, route, case, f"{route} {kind} D={D}")
        finally:
            ctx.close()
    else:
        _run_case(B, O, rctx, route, case, f"{route} {kind} D={D}{' two relations' if second else ''}")


_BLOCKS = T.block_cases()


@pytest.mark.parametrize("kind,D,nv,nu", _BLOCKS, ids=[f"{k}-{D}-{nv}-{nu}" for k, D, nv, nu in _BLOCKS])
def test_block_against_exact_samples(B, O, rctx, kind, D, nv, nu):
    """bdf_sample_block: nu users who share their nv items and one factorisation, against the exact sample of every user"""
    from bdf_amd._lib import check, lib
    import torch
    case = T.make_case(kind, D, nu, nobs=(nv, nv), block=True)
    t = case.terms[0]
    tr = T.Truth.of(case)
    ctx, tag = rctx, next(_tags)
    items = t.ids[:nv, 1] - 1
    Y = (t.vals - t.mean).reshape(nu, nv)                  # (nu, nv) in C order == nv x nu column-major; Yma is the value without its mean
    vx, Y_t, V_t = ctx.tensor(np.array(items), dtype=torch.int32), ctx.tensor(Y), ctx.tensor(np.array(t.V))
    mu_t, Lam_t = ctx.tensor(np.array(case.mu)), ctx.tensor(np.array(case.Lam))
    out_t = ctx.tensor(np.full((nu + GUARD, D), np.nan))
    z_t = ctx.zeros(nu, D)
    ctx.set_sweep(SWEEP)
    check(lib().bdf_sample_block(ctx.handle, D, nu, nv, _p(vx), _p(Y_t), _p(V_t), t.alpha, _p(mu_t), _p(Lam_t), tag, _p(out_t)))
    check(lib().bdf_normals(ctx.handle, 1, tag, 0, nu, D, _p(z_t)))
    ctx.sync()
    out, z = out_t.cpu().numpy(), z_t.cpu().numpy()
    _guard_untouched(out)
    T.check(f"block {kind} D={D} nv={nv} nu={nu}", D, tr.kappa, out[:nu], tr.ref_samples(z, False), T.ref_yardstick(case, z, False), nv)


@pytest.mark.parametrize("kind", ["alpha", "weights"])
@pytest.mark.parametrize("D", [8, 24, 64])
def test_dumped_system_is_the_exact_one(B, rctx, kind, D):
    """bdf_row_system against the exact P and c, componentwise, by the bound of an n-term sum:
    |P_dev - P| <= (n + 2) u (|Lambda| + sum alpha_o |w_o| |w_o|'),  |c_dev - c| <= (D + n + 2) u (|Lambda| |mu| + sum alpha_o |r_o| |w_o|)
    (c has the D terms of Lambda mu before its n): a kernel's error in the sample is then the solve's, not the accumulation's."""
    from bdf_amd._lib import check, lib
    from mpmath import mp
    case = T.case_of("k1", kind, D, None, False)
    dev = Dev(B, rctx, case)
    try:
        for per_row in (False, True):
            P_t, c_t = rctx.zeros(case.N, D, D), rctx.zeros(case.N, D)
            check(lib().bdf_row_system(rctx.handle, D, case.N, len(dev.terms), dev.terms, _p(dev.mu[per_row]), int(per_row), _p(dev.Lam), _p(P_t), _p(c_t)))
            rctx.sync()
            P, c = P_t.cpu().numpy(), c_t.cpu().numpy()
            worst_P = worst_c = 0.0
            for row in range(case.N):
                with mp.workdps(T.DPS):
                    Pe, ce = T.exact_system(case, row, per_row)
                    dP = np.array([[float(abs(mp.mpf(float(P[row][j][i])) - Pe[i][j])) for j in range(D)] for i in range(D)])
                    dc = np.array([float(abs(mp.mpf(float(c[row][i])) - ce[i])) for i in range(D)])
                W, a, r = case.row_obs_f64(row)
                n = len(a)
                bP = (n + 2) * T.U * (np.abs(case.Lam) + (np.abs(W) * a[:, None]).T @ np.abs(W))
                bc = (D + n + 2) * T.U * (np.abs(case.Lam) @ np.abs(case.mean_of(row, per_row)) + np.abs(W).T @ (a * np.abs(r)))
                worst_P, worst_c = max(worst_P, (dP / bP).max()), max(worst_c, (dc / bc).max())
                assert np.all(dP <= bP) and np.all(dc <= bc), (row, (dP / bP).max(), (dc / bc).max())
            print(f"dump {kind} D={D} per_row={per_row}: worst |P_dev - P| / bound {worst_P:.3g}, worst |c_dev - c| / bound {worst_c:.3g}")
    finally:
        dev.close()


@pytest.mark.parametrize("D", [5, 16, 33, 64])
def test_quad_with_an_ill_conditioned_lambda(B, rctx, D):
    """bdf_newrows_quad, q = |L^-1 v|^2 of M = 17 rows with the `prior` Lambda (cond 1e6): |q_dev - q| / q <= 8 D cond_2(Lambda) u against
    mpmath, and within 16 times the float64 numpy route's own error (or D u)"""
    from bdf_amd._lib import check, lib
    rng = np.random.default_rng(4000 + D)
    Lam, V = T.prior_lambda(rng, D), 0.5 * rng.standard_normal((17, D))
    q_t = rctx.tensor(np.full(17 + GUARD, np.nan))
    Lam_t, V_t = rctx.tensor(Lam), rctx.tensor(V)
    check(lib().bdf_newrows_quad(rctx.handle, D, 17, _p(Lam_t), _p(V_t), _p(q_t)))
    rctx.sync()
    q = q_t.cpu().numpy()
    _guard_untouched(q)
    T.check(f"quad D={D}", D, np.linalg.cond(Lam), q[:17, None], T.quad_exact(Lam, V)[:, None], T.quad_f64(Lam, V)[:, None])


# ---- the not-positive-definite flag of every row path ----------------------------------------------------------------------------------
def _late_bad_lambda(D):
    """one eigenvalue of -1e-3 among positive ones (1 .. 2) in a random basis: every leading block but the last few is positive
    definite, so the bad pivot comes late"""
    rng = np.random.default_rng(900 + D)
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    ev = np.linspace(1.0, 2.0, D)
    ev[D // 2] = -1e-3
    L = (Q * ev) @ Q.T
    return (L + L.T) / 2


def _first_bad_pivot(A):
    """index of the first pivot that is not positive when A is factored without pivoting"""
    A = A.copy()
    for k in range(len(A)):
        if not A[k, k] > 0:
            return k
        A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k], A[k + 1:, k]) / A[k, k]
    return None


@pytest.mark.parametrize("route,D,nobs", [("k1", 24, None), ("k1", 48, None), ("k1s", 8, (0, 48)), ("k1c", 24, None), ("lr", 24, (0, 12))],
                         ids=["k1-24", "k1-48", "k1s-8", "k1c-24", "lr-24"])
@pytest.mark.parametrize("bad", ["negative", "late"])
def test_not_positive_definite_is_reported_by_every_path(B, O, rctx, route, D, nobs, bad):
    """Lambda = -1e6 I on the `plain` case's rows, and a Lambda with one eigenvalue of -1e-3 on rows without observations (an entity
    whose last row alone has any): the call returns BDF_OK, the next sync raises NotPositiveDefinite once and the one after is clean,
    no split row is left unfinished, the 16 guard rows behind `out` stay NaN, and the same route then samples the `plain` case with a
    good Lambda inside both bounds.  The library's own status path: nothing faults."""
    case = T.case_of(route, "plain", D, nobs, False)
    if bad == "negative":
        bad_case, Lam = case, -1e6 * np.eye(D)
    else:
        t = case.terms[0]
        last = t.ids[:, 0] == case.N
        assert last.any()
        bad_case = T.Case(("late",) + case.key, "plain", D, case.N, case.Lam, case.mu, case.mu_rows,
                          [T.TermData(t.ids[last], t.vals[last], t.V, t.alpha, t.mean)])
        assert np.all(bad_case.counts[:-1] == 0)
        Lam = _late_bad_lambda(D)
        # late in the kernels' order (the index-reversed matrix) and in k_lr_prep's (Lambda itself): one of the last two pivots
        assert _first_bad_pivot(Lam[::-1, ::-1]) >= D - 2 and _first_bad_pivot(Lam) >= D - 2
    dev = Dev(B, rctx, bad_case, Lam=Lam)
    try:
        _route(rctx, route)
        for per_row in (False, True):
            tag = next(_tags)
            rc, out_t = dev.sample(per_row, tag)
            assert rc == 0                              # BDF_OK: the flag is raised on the device
            with pytest.raises(B.NotPositiveDefinite):
                rctx.sync()
            rctx.sync()                                 # reported once
            _dispatched(route, bad_case, rctx.rows_dispatch(tag))
            assert rctx.rows_unfinished() == 0
            _guard_untouched(out_t.cpu().numpy())
    finally:
        _restore(rctx)
        dev.close()
    _run_case(B, O, rctx, route, case, f"after the flag: {route} plain D={D}")
