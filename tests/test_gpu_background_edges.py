"""Background cells (setBackground) past one tile, one workgroup and one term: what csrc/k_background.hip does
beyond N = 37, M = 29 and one relation, where tests/test_gpu_background.py stays.

(a) k_bg_mu_rows (bdf_background_prior with a per-row prior mean).  One iteration of a workgroup covers R(D) = 64, 32, 16 rows for
    D <= 16, <= 32, <= 64 and the grid is min(iterations, 4096): the row edges N in {1, 15, 16, 17, R - 1, R, R + 1} and N = 0, then
    N = 4096 R + R + 1, the smallest N at which workgroup 0 runs a full second tile and workgroup 1 a second tile of one row.
(b) k_bg_fold with two to four terms, alpha by argument and from alpha_dev in turn, and the same terms in reversed order.
(c) bdf_background_sse at n in {0, 1, 7, 8, 9, 257} listed cells for its three instantiations, and over 257 workgroups' sums.
(d) one entity in two background relations with a plain relation between them, end to end on both iteration paths.
(e) a fold at kappa_2 ~ 1e9, where the refinement step of fold_solve decides the residual, and a fold that is not positive definite.

References are numpy in float64 (math.fsum for the sums); the bounds are those of tests/test_gpu_background.py."""
import ctypes as C
import functools
import math
import os
import textwrap

import numpy as np
import pytest

from both_paths import child
import background_restatement as BR
from test_gpu_background import _distance, _fold, _prior, _take
from test_gpu_pair_edges import _dev, _facs, _nan, _p, _untouched

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U52 = 2.0 ** -52
GRID = 4096                       # k_bg_mu_rows: the cap on its workgroups
MAX_TERMS = 4                     # BDF_MAX_TERMS
# (d): how far the dense explicit run of the three relations moves from itself when the rows of its listings are permuted (max
# |difference| / max(1, max |value|) over the three entities' samples, the test predictions and both alpha traces after 3 + 3
# iterations), measured on an MI355X as FLOOR of tests/test_gpu_background.py was, per D.  Each D is held to
# ten times its own floor, and to 1e-6 at most.  (The background runs measured 1.5e-15 and 1.1e-14 from the dense run.)
FLOOR_TWO = {5: 1.75e-15, 40: 8.0e-15}
CHAIN_TOL_TWO = {D: min(10.0 * f, 1e-6) for D, f in FLOOR_TWO.items()}


def _rows_per_iteration(D):
    return 64 if D <= 16 else (32 if D <= 32 else 16)


def _sums(ctx, D, V_t):
    from bdf_amd._lib import check, lib
    s_t, G_t = ctx.zeros(D), ctx.zeros(D, D)
    check(lib().bdf_hyper_sums(ctx.handle, D, V_t.shape[0], _p(V_t), None, _p(s_t), _p(G_t)))
    return s_t, G_t


def _prior_call(ctx, D, N, terms, mu_t, is_matrix, Lam_t, pack=True):
    """bdf_background_prior on terms = [(s_t, G_t, alpha, alpha_dev tensor | None, c0, rb)] -> (rc, Lambda_eff, mu_eff, pack | None,
    alpha_rows) tensors.  mu_eff of a per-row prior mean has 16 rows of NaN behind its N, the pack 16 NaN behind its end, alpha_rows
    is BDF_MAX_TERMS NaN"""
    from bdf_amd._lib import BackgroundTerm, lib
    bg = (BackgroundTerm * len(terms))()
    for k, (s_t, G_t, alpha, a_dev, c0, rb) in enumerate(terms):
        bg[k].sum, bg[k].gram, bg[k].alpha, bg[k].weight, bg[k].resid = s_t.data_ptr(), G_t.data_ptr(), alpha, c0, rb
        bg[k].alpha_dev = a_dev.data_ptr() if a_dev is not None else None
    Le_t = _nan(ctx, D + 16, D)
    me_t = _nan(ctx, N + 16, D) if is_matrix else _nan(ctx, D + 16)
    pk_t = _nan(ctx, lib().bdf_prior_pack_doubles(D) + 16) if (pack and not is_matrix) else None
    ar_t = ctx.tensor(np.full(MAX_TERMS, np.nan))
    rc = lib().bdf_background_prior(ctx.handle, D, N, len(terms), bg, _p(mu_t), int(is_matrix), _p(Lam_t), _p(Le_t), _p(me_t), _p(pk_t), _p(ar_t))
    return rc, Le_t, me_t, pk_t, ar_t


def _check_mu(what, D, Le, ref, want, rhs, m_dev, kappa=None, hold=True):
    """the two bounds of test_fold_alone_against_numpy: forward error 8 D kappa_2 2^-52 of max |want|, residual Lambda_eff mu_eff - rhs
    within D 2^-50 of |Lambda_eff|_inf max |want|; Le the device's Lambda_eff, ref the reference's -> (forward error, residual).
    hold=False: print the two figures and return them"""
    kappa = np.linalg.cond(ref) if kappa is None else kappa
    err = np.abs(m_dev - want).max() / np.abs(want).max()
    res = np.abs(m_dev @ Le.T - rhs).max() / (np.abs(Le).sum(axis=1).max() * np.abs(want).max())
    print(f"{what}: kappa {kappa:.3g}, forward error {err:.2e} (bound {8 * D * kappa * U52:.2e}), residual {res:.2e} (bound {D * 4 * U52:.2e})")
    if hold:
        assert np.all(np.isfinite(m_dev)), what
        assert err <= 8 * D * kappa * U52 and res <= D * 2.0 ** -50, (what, err, res)
    return err, res


def _check_pack(pk, Le, me, D):
    """the pack: Lambda_eff mu_eff, then the accumulator-layout image of the index-reversed Lambda_eff (identity on the padding)"""
    assert np.allclose(pk[:D], Le @ me, rtol=1e-13, atol=1e-13 * np.abs(Le @ me).max())
    DP = 16 if D <= 16 else (32 if D <= 32 else 64)
    full = np.eye(DP)
    full[:D, :D] = Le[::-1, ::-1]
    img, e = pk[D:].reshape(-1, 64), 0
    for I in range(DP // 16):
        for J in range(I + 1):
            for r in range(4):
                lane = np.arange(64)
                assert np.array_equal(img[e], full[16 * I + (lane >> 4) + 4 * r, 16 * J + (lane & 15)]), (I, J, r)
                e += 1
    assert e == len(img)


# ---- (a) per-row prior means ------------------------------------------------------------------------------------------------------
class _RowsCase:
    """one fold (M = 29, one term) per D for the tests of k_bg_mu_rows: the device's s and G, numpy's Lambda_eff on them"""

    def __init__(self, ctx, D, seed):
        rng = np.random.default_rng(seed)
        self.ctx, self.D, self.rng = ctx, D, rng
        self.alpha, self.c0, self.rb = 2.5, 0.2, -0.7
        V, self.Lam = rng.standard_normal((29, D)), _prior(rng, D)
        self.Lam_t = ctx.tensor(self.Lam)
        self.s_t, self.G_t = _sums(ctx, D, ctx.tensor(V))
        ctx.sync()
        s, G = self.s_t.cpu().numpy(), self.G_t.cpu().numpy()
        assert np.allclose(G, V.T @ V, rtol=1e-12, atol=1e-12) and np.allclose(s, V.sum(axis=0), rtol=1e-12, atol=1e-12)
        self.ref = self.Lam + (self.alpha * self.c0) * G
        self.t = (self.alpha * self.c0 * self.rb) * s
        self.kappa = np.linalg.cond(self.ref)

    def run(self, mus):
        """mu_eff of the rows `mus`, its guard rows checked, and the device's Lambda_eff"""
        N = len(mus)
        rc, Le_t, me_t, _, _ = _prior_call(self.ctx, self.D, N, [(self.s_t, self.G_t, self.alpha, None, self.c0, self.rb)], self.ctx.tensor(mus), True, self.Lam_t)
        assert rc == 0
        self.ctx.sync()
        assert _untouched(me_t, N) and _untouched(Le_t, self.D)
        Le = Le_t.cpu().numpy()[:self.D]
        assert np.abs(Le - self.ref).max() <= 4 * U52 * np.abs(self.ref).max()
        return me_t.cpu().numpy()[:N], Le

    def check(self, what, mus, out, Le):
        rhs = mus @ self.Lam.T + self.t
        want = np.linalg.solve(self.ref, rhs.T).T
        return _check_mu(what, self.D, Le, self.ref, want, rhs, out, self.kappa)


@pytest.mark.parametrize("D", [3, 16, 17, 32, 33, 64])
def test_per_row_prior_means_at_the_row_edges(B, ctx, D):
    """mu_eff,i = Lambda_eff^-1 (Lambda mu_i + t) for N in {1, 15, 16, 17, R - 1, R, R + 1} rows against numpy's solve at the two
    bounds of test_fold_alone_against_numpy (forward 8 D kappa_2 2^-52, residual D 2^-50); the 16 rows of NaN behind the N stay NaN
    (tile_row() < 0 on the partly filled last iteration).  N = 0: BDF_OK, no row launch, mu_out untouched"""
    R = _rows_per_iteration(D)
    c = _RowsCase(ctx, D, 700 + D)
    for N in sorted({1, 15, 16, 17, R - 1, R, R + 1}):
        mus = c.rng.standard_normal((N, D))
        out, Le = c.run(mus)
        c.check(f"per-row prior means D={D} N={N}", mus, out, Le)
    rc, Le_t, me_t, _, ar_t = _prior_call(ctx, D, 0, [(c.s_t, c.G_t, c.alpha, None, c.c0, c.rb)], ctx.zeros(8, D), True, c.Lam_t)
    assert rc == 0
    ctx.sync()
    assert _untouched(me_t, 0) and float(ar_t.cpu().numpy()[0]) == c.alpha * (1.0 - c.c0)
    assert np.abs(Le_t.cpu().numpy()[:D] - c.ref).max() <= 4 * U52 * np.abs(c.ref).max()


@pytest.mark.parametrize("D", [3, 16, 17, 33])
def test_per_row_prior_means_on_the_second_trip(B, ctx, D):
    """N = 4096 R + R + 1 (D = 16: 4096 * 64 + 65, DB = 1 and no padded column): workgroup 0 takes a full second tile and workgroup 1
    a second tile of one row; every other workgroup leaves after its first.  Two inputs, each held to the two bounds over all rows.

    twins: row r + 4096 R repeats row r.  The second-trip rows sit in the lanes of the same wave of the same workgroup as their
    twins and go through the same operations in the same order: their outputs are the twins' bits.  (A wrong stride or a wrong row
    index fails this and the bounds.  A stale prefetch or a tile overwritten too early would not: the tile the twins came from holds
    the same numbers.)
    distinct: every row its own.  The second-trip rows against a launch of those R + 1 rows alone, which puts them in the same
    lanes of the same waves of workgroups 0 and 1 on their FIRST trip: the same bits -- with a stale or a half-overwritten tile
    the second trip would have read rows 0 .. 2 R of the input instead."""
    R = _rows_per_iteration(D)
    first, N = GRID * R, GRID * R + R + 1
    c = _RowsCase(ctx, D, 800 + D)
    distinct = c.rng.standard_normal((N, D))
    twins = distinct.copy()
    twins[first:] = twins[:R + 1]
    out, Le = c.run(twins)
    c.check(f"second trip D={D} N={N} twins", twins, out, Le)
    assert np.array_equal(out[first:], out[:R + 1])
    out, Le = c.run(distinct)
    c.check(f"second trip D={D} N={N} distinct", distinct, out, Le)
    c.check(f"second trip D={D} N={N} distinct, the second-trip rows", distinct[first:], out[first:], Le)
    alone, _ = c.run(distinct[first:])
    assert np.array_equal(out[first:], alone)
    assert not np.array_equal(out[first:], out[:R + 1])


# ---- (b) two to four terms --------------------------------------------------------------------------------------------------------
def _fold_terms(ctx, D, N, Vs, alphas, c0s, rbs, order, mu, mus, Lam):
    """the terms `order` of (Vs, alphas, c0s, rbs) in one bdf_background_prior, with a shared prior mean (and the pack) and with a
    per-row one, held against BR.fold of the same list.  alpha of the k-th term of the call: k even as the argument, k odd from
    alpha_dev with a decoy as the argument.  -> the worst (forward error, residual)"""
    n_bg = len(order)
    terms, listed = [], []
    for k, q in enumerate(order):
        s_t, G_t = _sums(ctx, D, ctx.tensor(Vs[q]))
        terms.append((s_t, G_t, alphas[q], None, c0s[q], rbs[q]) if k % 2 == 0 else (s_t, G_t, 123.0, ctx.tensor([alphas[q]]), c0s[q], rbs[q]))
        listed.append((alphas[q], c0s[q], rbs[q], Vs[q]))
    Lam_t = ctx.tensor(Lam)
    rc1, Le_t, me_t, pk_t, ar_t = _prior_call(ctx, D, N, terms, ctx.tensor(mu), False, Lam_t)
    rc2, Lm_t, mm_t, _, am_t = _prior_call(ctx, D, N, terms, ctx.tensor(mus), True, Lam_t)
    assert rc1 == 0 and rc2 == 0
    ctx.sync()
    from bdf_amd._lib import lib
    npk = lib().bdf_prior_pack_doubles(D)
    assert _untouched(Le_t, D) and _untouched(Lm_t, D) and _untouched(me_t, D) and _untouched(mm_t, N) and _untouched(pk_t, npk)
    for t, q in zip(terms, order):                     # the sums are exact on these V: BR.fold sees what the device saw
        assert np.array_equal(t[1].cpu().numpy(), Vs[q].T @ Vs[q]) and np.array_equal(t[0].cpu().numpy(), Vs[q].sum(axis=0))
    Le, me, pk, ar = Le_t.cpu().numpy()[:D], me_t.cpu().numpy()[:D], pk_t.cpu().numpy()[:npk], ar_t.cpu().numpy()
    Lm, mm, am = Lm_t.cpu().numpy()[:D], mm_t.cpu().numpy()[:N], am_t.cpu().numpy()
    ref, want, ar_ref = BR.fold(Lam, mu, listed)
    _, wants, _ = BR.fold(Lam, mus, listed)
    eL = np.abs(Le - ref).max() / np.abs(ref).max()
    print(f"fold of {n_bg} terms {list(order)} D={D}: |dLambda_eff| {eL / U52:.2f} ulp of max |Lambda_eff| (bound {4 * n_bg})")
    assert eL <= 4 * n_bg * U52 and np.array_equal(Le, Lm)
    assert np.array_equal(ar[:n_bg], ar_ref) and np.all(np.isnan(ar[n_bg:])) and np.array_equal(ar, am, equal_nan=True), (ar, ar_ref)
    t = np.zeros(D)
    for a, c0, rb, V in listed:
        t = t + (a * c0 * rb) * V.sum(axis=0)
    e1 = _check_mu(f"fold of {n_bg} terms {list(order)} D={D} rows=1", D, Le, ref, want, mu @ Lam.T + t, me)
    e2 = _check_mu(f"fold of {n_bg} terms {list(order)} D={D} rows={N}", D, Le, ref, wants, mus @ Lam.T + t, mm)
    _check_pack(pk, Le, me, D)
    return max(e1[0], e2[0]), max(e1[1], e2[1])


@pytest.mark.parametrize("n_bg", [2, 3, 4])
@pytest.mark.parametrize("D", [3, 17, 64])
def test_fold_of_two_to_four_terms(B, ctx, D, n_bg):
    """Lambda_eff = Lambda + sum_k alpha_k c0_k G_k, M_k = 29, 5, 41, 1 rows (G_k rank-deficient wherever M_k < D), every term its
    own alpha, c0 and rb, against BR.fold: Lambda_eff within 4 n_bg 2^-52 max |Lambda_eff| (every partial sum is positive
    semidefinite and no larger than the total, a term adds one rounding of its product and one of the sum: 2 n_bg u, and a factor
    2), alpha_rows_out[k] = alpha_k (1 - c0_k) exactly and NaN behind n_bg, mu_eff for a shared and a per-row prior mean at the two
    bounds, the pack's image; then the same terms in reversed order against BR.fold of the reversed list.  The entries of V_k are
    multiples of 1/8 in [-1, 1], so s_k and G_k are exact on the device and in numpy: both folds start from the same numbers."""
    rng = np.random.default_rng(500 + 10 * D + n_bg)
    N = 37
    Vs = [rng.integers(-8, 9, (M, D)) / 8.0 for M in (29, 5, 41, 1)[:n_bg]]
    alphas, c0s, rbs = [2.5, 0.7, 11.0, 1.3][:n_bg], [0.2, 0.05, 0.5, 1.0][:n_bg], [-0.7, 0.4, 0.0, 1.9][:n_bg]
    Lam, mu, mus = _prior(rng, D), rng.standard_normal(D), rng.standard_normal((N, D))
    for order in (tuple(range(n_bg)), tuple(reversed(range(n_bg)))):
        _fold_terms(ctx, D, N, Vs, alphas, c0s, rbs, order, mu, mus, Lam)


# ---- (c) alpha's sum of squares ---------------------------------------------------------------------------------------------------
def _fsum(a):
    return math.fsum(np.asarray(a, dtype=np.float64).ravel().tolist())


@functools.lru_cache(maxsize=None)
def _sse_case(N, M, D, n, weights):
    """n distinct listed cells of an N x M relation in a random order, a background of weight 0.3 min omega at -0.5, and the folded
    sum restated: the listed cells' terms omega e^2 - c0 (rb - psi)^2, the three pieces of the closed form, math.fsum of all of them,
    and `scale` = sum |terms| + sum |pieces|, what a relative bound on the sum is taken against (a listed term can be negative).
    Shared by the tests and left unchanged"""
    rng = np.random.default_rng(6000 + 100 * D + n + int(weights))
    cells = rng.choice(N * M, size=n, replace=False)
    assert len(np.unique(cells)) == n
    ids = np.stack([cells // M + 1, cells % M + 1], axis=1).astype(np.int64).reshape(n, 2)
    y = np.round(rng.normal(1.0, 1.0, n), 1)
    w = np.exp(rng.uniform(-0.5, 1.5, n)) if weights else np.ones(n)
    c0, value = 0.3 * float(w.min()) if n else 0.3, -0.5
    assert n == 0 or w.min() > c0
    U, V = 0.5 * rng.standard_normal((N, D)), 0.5 * rng.standard_normal((M, D))
    mean = BR.all_cells_mean(N, M, y, value)
    rb = value - mean
    psi = np.sum(U[ids[:, 0] - 1] * V[ids[:, 1] - 1], axis=1)
    e, d = (y - mean) - psi, rb - psi
    terms = w * (e * e) - c0 * (d * d)
    pieces = [c0 * (N * M) * (rb * rb), -2.0 * c0 * rb * _fsum(U.sum(axis=0) * V.sum(axis=0)), c0 * _fsum((U.T @ U) * (V.T @ V))]
    total, scale = _fsum(terms.tolist() + pieces), _fsum(np.abs(terms).tolist() + np.abs(pieces).tolist())
    assert total >= 0.1 * scale, (total, scale)        # the relative bound below bounds the kernel, not the cancellation
    c = dict(ids=ids, y=y, w=w, c0=c0, value=value, mean=mean, rb=rb, U=U, V=V, terms=terms, total=total, scale=scale,
             dense=BR.sse_dense(ids, y, w, mean, c0, value, U, V))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def _sse_run(B, ctx, N, M, D, c, weights, sort):
    """bdf_background_sse twice on the listed cells, bdf_pairs_weighted_sse on the dense listing -> (folded, folded again, dense, the
    two entities' sums and Gram matrices as the device made them)"""
    from bdf_amd._lib import check, lib
    ida, ya, wa = BR.dense_listing(N, M, c["ids"], c["y"], c["w"], c["c0"], c["value"])
    ft = [ctx.tensor(c["U"]), ctx.tensor(c["V"])]
    pl, pd = B.DevicePairs(ctx, c["ids"], c["y"]), B.DevicePairs(ctx, ida, ya)
    if sort:
        pl.sort(1)
        pd.sort(1)
    sums = [ctx.zeros(D), ctx.zeros(D, D), ctx.zeros(D), ctx.zeros(D, D)]
    for k in (0, 1):
        check(lib().bdf_hyper_sums(ctx.handle, D, ft[k].shape[0], _p(ft[k]), None, _p(sums[2 * k]), _p(sums[2 * k + 1])))
    out = ctx.tensor(np.full(8, np.nan))
    w_t = _dev(ctx, c["w"]) if weights else None
    for k in (0, 1):
        check(lib().bdf_background_sse(ctx.handle, pl.handle, D, _facs(ft), c["mean"], _p(w_t), c["value"], c["c0"], *[_p(t) for t in sums], N, M,
                                       C.c_void_p(out.data_ptr() + 8 * k)))
    check(lib().bdf_pairs_weighted_sse(ctx.handle, pd.handle, D, _facs(ft), c["mean"], _p(ctx.tensor(wa)), C.c_void_p(out.data_ptr() + 16)))
    ctx.sync()
    s = out.cpu().numpy()
    assert np.all(np.isnan(s[3:]))
    pl.close()
    pd.close()
    return s[0], s[1], s[2], [t.cpu().numpy() for t in sums]


@pytest.mark.parametrize("sort", [False, True])
@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("D", [7, 32, 64])
def test_folded_sum_of_squares_at_the_group_edges(B, ctx, D, weights, sort):
    """bdf_background_sse at n in {0, 1, 7, 8, 9, 257} distinct listed cells of a 37 x 29 relation: an empty listing (no gather is
    launched: the closed form alone), a lone lane, one short of a group of eight lanes, one group, one over, and one cell alone in a
    second workgroup; D = 7, 32, 64 are k_bg_sse<1, 1>, <4, 1> and <4, 2>.  Against math.fsum of the restated terms, BR.sse_dense
    and bdf_pairs_weighted_sse over the dense listing at 1e-12 of sum |terms| + sum |pieces of the closed form| (the kernel's
    own error is of order (log2 n + 2 D) u, 3e-14 at the widest); two calls: the same bits"""
    N, M = 37, 29
    for n in (0, 1, 7, 8, 9, 257):
        c = _sse_case(N, M, D, n, weights)
        s0, s1, sd, sums = _sse_run(B, ctx, N, M, D, c, weights, sort)
        tol = 1e-12 * c["scale"]
        print(f"background sse edges D={D} weights={weights} sort={sort} n={n}: folded {s0:.15g} dense {sd:.15g}; of the scale "
              f"{c['scale']:.6g}: against fsum {abs(s0 - c['total']) / c['scale']:.2e}, BR.sse_dense {abs(s0 - c['dense']) / c['scale']:.2e}, "
              f"the dense call {abs(s0 - sd) / c['scale']:.2e}")
        assert np.isfinite(s0) and s0.tobytes() == s1.tobytes()
        assert abs(s0 - c["total"]) <= tol and abs(s0 - c["dense"]) <= tol and abs(s0 - sd) <= tol, (n, s0, sd, c["total"], c["dense"])
        if n == 0:
            closed = c["c0"] * (((N * M) * (c["rb"] * c["rb"]) - 2.0 * c["rb"] * float(sums[0] @ sums[2])) + float(np.sum(sums[1] * sums[3])))
            assert abs(s0 - closed) <= tol, (s0, closed)


@pytest.mark.parametrize("weights", [False, True])
def test_folded_sum_of_squares_over_257_workgroups(B, ctx, weights):
    """65,537 distinct listed cells of a 300 x 250 relation, D = 8: nblocks = 257, so thread 0 of k_bg_sse_final adds partial 0 and
    partial 256, the sum of the one cell that is alone in the last workgroup.  Against math.fsum of the per-pair bdf_bg_term values
    plus the closed form, BR.sse_dense over the 75,000 cells and the dense device call, at 1e-12 of sum |terms| + sum |pieces|;
    the last cell's term is far outside that bound"""
    N, M, D, n = 300, 250, 8, 256 * 256 + 1
    c = _sse_case(N, M, D, n, weights)
    s0, s1, sd, _ = _sse_run(B, ctx, N, M, D, c, weights, False)
    tol = 1e-12 * c["scale"]
    print(f"background sse 257 workgroups weights={weights}: folded {s0:.15g} dense {sd:.15g}; of the scale {c['scale']:.6g}: against fsum "
          f"{abs(s0 - c['total']) / c['scale']:.2e}, BR.sse_dense {abs(s0 - c['dense']) / c['scale']:.2e}, the dense call {abs(s0 - sd) / c['scale']:.2e}; "
          f"the last cell's term, alone in workgroup 257, {c['terms'][-1]:.3e}")
    assert abs(c["terms"][-1]) > 100 * tol
    assert np.isfinite(s0) and s0.tobytes() == s1.tobytes()
    assert abs(s0 - c["total"]) <= tol and abs(s0 - c["dense"]) <= tol and abs(s0 - sd) <= tol, (s0, sd, c["total"], c["dense"])


# ---- (d) one entity in two background relations -------------------------------------------------------------------------------------
TWO_DS = (5, 40)

CHILD = textwrap.dedent('''
    import os, sys
    import numpy as np
    sys.path.insert(0, %r); sys.path.insert(0, %r)
    import bdf_amd as B
    import background_restatement as BR
    out, d = sys.argv[1], {}
    NU, NV, NW = 37, 29, 23
    p_ids, p_y, p_w = BR.listing(NU, NV, weights=True)                  # plays (u, v): weights, a background
    p_bg = (0.3 * float(p_w.min()), -0.5)
    r_ids, r_y, _ = BR.listing(NU, NW, seed=1)                          # rated (u, w): no background
    t_ids, t_y, t_w = BR.listing(NW, NU, seed=2)                        # tagged (w, u): unit weights, a background
    t_bg = (0.25, 0.5)
    rng = np.random.default_rng(11)
    cells = rng.choice(NU * NV, size=40, replace=False)
    test, test_y = np.stack([cells // NV + 1, cells %% NV + 1], axis=1).astype(np.int64), rng.standard_normal(40)

    def relation(name, ents, ids, y, weights, background, dims, sample):
        a, b = ents
        r = B.Relation({a.name: ids[:, 0], b.name: ids[:, 1], "y": y}, name, [a, b], alpha=2.0, dims=list(dims))
        r.model.alpha_sample = sample
        if name == "plays":
            B.setTest(r, {"u": test[:, 0], "v": test[:, 1], "y": test_y})
        if weights is not None:
            B.setWeights(r, weights)
        if background is not None:
            B.setBackground(r, *background)
        return r

    def run(key, D, plays, rated, tagged):
        """plays, tagged: (ids, y, weights | None, background | None); rated: (ids, y)"""
        u, v, w = B.Entity("u"), B.Entity("v"), B.Entity("w")
        rels = [relation("plays", (u, v), *plays, (NU, NV), True), relation("rated", (u, w), *rated, None, None, (NU, NW), False),
                relation("tagged", (w, u), *tagged, (NW, NU), True)]
        rd = B.RelationData()
        for r in rels:
            B.addRelation(rd, r)
        names = [en.name for en in rd.entities]
        # u's terms: plays (background slot 0), rated (none), tagged (term 2, background slot 1, u its second mode)
        res = B.macau(rd, num_latent=D, burnin=3, psamples=3, verbose=False, seed=91,
                      f=lambda data: [float(data.relations[k]._dev.alpha_dev.item()) for k in (0, 2)])
        eu = rd.entities[names.index("u")]
        d[key + "u_terms"], d[key + "u_modes"] = np.array([r.name for r in eu.relations]), np.array(list(eu.modes))
        d[key + "native"] = np.array(int(rd._engine.native))
        d[key + "pred"], d[key + "trace"] = res["predictions"]["pred"].to_numpy(), np.array(res["f_output"])
        d[key + "mean"], d[key + "alpha"] = np.array([rels[0].model.mean_value, rels[2].model.mean_value]), np.array([rels[0].model.alpha, rels[2].model.alpha])
        for k, name in enumerate("uvw"):
            d[key + "S%%d" %% k] = rd.entities[names.index(name)].model.sample.T
        bg = res.get("background", {})
        d[key + "bg_names"], d[key + "bg_cells"] = np.array(sorted(bg)), np.array([bg[k]["cells"] for k in sorted(bg)], dtype=np.int64)
        rd._engine.close()

    p_dense = BR.dense_listing(NU, NV, p_ids, p_y, p_w, *p_bg)
    t_dense = BR.dense_listing(NW, NU, t_ids, t_y, t_w, *t_bg)
    for D in %r:
        key = "%%d_" %% D
        run(key + "bg_", D, (p_ids, p_y, p_w, p_bg), (r_ids, r_y), (t_ids, t_y, None, t_bg))
        run(key + "dense_", D, (*p_dense, None), (r_ids, r_y), (*t_dense, None))
        if not os.environ.get("BDF_NO_NATIVE"):
            pp, pr, pt = (np.random.default_rng(3 + k).permutation(n) for k, n in enumerate((NU * NV, len(r_y), NW * NU)))
            run(key + "perm_", D, (*[x[pp] for x in p_dense], None), (r_ids[pr], r_y[pr]), (*[x[pt] for x in t_dense], None))
    np.savez(out, **d)
''') % (ROOT, os.path.join(ROOT, "tests"), TWO_DS)


@pytest.fixture(scope="module")
def chains():
    """3 + 3 iterations of every run on the native and on the step-by-step path: one child process per path"""
    return child(CHILD, no_native=False), child(CHILD, no_native=True)


def _distance3(a, b):
    """_distance of tests/test_gpu_background.py (two entities' samples, the predictions, the alpha traces) and the third entity's samples"""
    return max(_distance(a, b), np.abs(a["S2"] - b["S2"]).max() / max(1.0, np.abs(b["S2"]).max()))


@pytest.mark.parametrize("D", TWO_DS)
def test_one_entity_in_two_background_relations_equals_the_dense_explicit_run(chains, D):
    """Entities u (37), v (29), w (23); u's relations in this order: plays (u, v) with a background, weights and a sampled alpha;
    rated (u, w) without a background; tagged (w, u) with a background, unit weights and a sampled alpha -- for u the unit-weight
    background term is term 2 but background slot 1, and u is its second mode.  macau(burnin=3, psamples=3) on the native and on
    the step-by-step path: the same bits; against the dense explicit run (BR.dense_listing of both background relations, with
    setWeights) the three entities' samples, the test predictions and both alpha traces within CHAIN_TOL_TWO[D], ten times the
    floor that the dense run permuted against itself measured at this D (FLOOR_TWO)"""
    nat, step = _take(chains[0], "%d_" % D), _take(chains[1], "%d_" % D)
    for k in nat:
        if not k.endswith("native") and not k.startswith("perm_"):
            assert np.array_equal(nat[k], step[k]), k
    bg, dense, perm = _take(nat, "bg_"), _take(nat, "dense_"), _take(nat, "perm_")
    assert bg["native"] == 1 and _take(step, "bg_")["native"] == 0
    assert list(bg["u_terms"]) == ["plays", "rated", "tagged"] and list(bg["u_modes"]) == [1, 1, 2]
    n_plays, n_tagged = len(BR.listing(37, 29, weights=True)[1]), len(BR.listing(23, 37, seed=2)[1])
    assert list(bg["bg_names"]) == ["plays", "tagged"] and list(bg["bg_cells"]) == [37 * 29 - n_plays, 23 * 37 - n_tagged]
    assert len(dense["bg_names"]) == 0
    assert np.abs(bg["mean"] - dense["mean"]).max() <= 1e-14
    assert bg["trace"].shape == (3, 2) and np.all(bg["trace"] > 0) and len(set(bg["trace"][:, 0])) == 3 and len(set(bg["trace"][:, 1])) == 3
    floor, dist = _distance3(perm, dense), _distance3(bg, dense)
    print(f"two background relations on one entity D={D}: permuted dense run {floor:.2e}, background run {dist:.2e}")
    assert dist <= CHAIN_TOL_TWO[D], (dist, floor)
    assert min(np.abs(bg[k]).max() for k in ("S0", "S1", "S2")) > 0.1          # (chains, not zeros)


# ---- (e) ill-conditioned and indefinite folds ---------------------------------------------------------------------------------------
def _refined(A, b, steps=2):
    """np.linalg.solve, then `steps` of refinement with the residual taken in np.longdouble: well below kappa u"""
    x = np.linalg.solve(A, b)
    Al, bl = A.astype(np.longdouble), b.astype(np.longdouble)
    for _ in range(steps):
        x = x + np.linalg.solve(A, (bl - Al @ x.astype(np.longdouble)).astype(np.float64))
    return x


def _cholesky_refined(A, b):
    """what a float64 Cholesky solve with one refinement step in float64 reaches: the yardstick for the device's fold_solve"""
    L = np.linalg.cholesky(A)

    def solve(r):
        return np.linalg.solve(L.T, np.linalg.solve(L, r))

    x = solve(b)
    return x + solve(b - A @ x)


@pytest.mark.parametrize("D", [16, 33])
def test_ill_conditioned_fold_keeps_its_residual(B, ctx, D):
    """Lambda with eigenvalues log-spaced over 1e-6 .. 1, V of M = 5 rows of length about 2 with alpha c0 = 1e3:
    kappa_2(Lambda_eff) of order 1e9 (asserted in 1e7 .. 1e10).  mu_eff of a shared prior mean against np.linalg.solve refined twice
    with a long-double residual, at the same two bounds as the well-conditioned folds: forward 8 D kappa_2 2^-52, residual D 2^-50 of
    |Lambda_eff|_inf max |mu_eff| -- which an unrefined solve with pivots' reciprocals good to 1.5e-15 does not promise.  A float64
    numpy Cholesky solve with one refinement step goes through the same check beside it, as the yardstick."""
    rng = np.random.default_rng(1600 + D)
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    Lam = (Q * np.logspace(-6.0, 0.0, D)) @ Q.T
    Lam = 0.5 * (Lam + Lam.T)
    V, mu = 2.0 * rng.standard_normal((5, D)) / math.sqrt(D), rng.standard_normal(D)
    alpha, c0, rb, N = 1e4, 0.1, -0.7, 37
    V_t, Lam_t = ctx.tensor(V), ctx.tensor(Lam)
    s_t, G_t, Le_t, me_t, _, ar_t = _fold(ctx, D, N, V_t, alpha, c0, rb, ctx.tensor(mu), False, Lam_t)
    ctx.sync()
    s, G, Le, me = (t.cpu().numpy() for t in (s_t, G_t, Le_t, me_t))
    ref = Lam + (alpha * c0) * G
    kappa = np.linalg.cond(ref)
    assert 1e7 <= kappa <= 1e10, kappa
    assert np.abs(Le - ref).max() <= 4 * U52 * np.abs(ref).max() and float(ar_t.item()) == alpha * (1.0 - c0)
    rhs = Lam @ mu + (alpha * c0 * rb) * s
    want = _refined(ref, rhs)
    _check_mu(f"ill-conditioned fold D={D}, numpy Cholesky with one refinement step", D, ref, ref, want, rhs, _cholesky_refined(ref, rhs), kappa, hold=False)
    _check_mu(f"ill-conditioned fold D={D}, the device", D, Le, ref, want, rhs, me, kappa)


@pytest.mark.parametrize("D", [3, 33])
def test_indefinite_fold_is_reported(B, ctx, D):
    """Lambda = -1e6 I with a small Gram term: the calls return BDF_OK, the fold raises the context's not-positive-definite flag
    (the library's own status: ctx.sync() raises NotPositiveDefinite once, a second sync is clean) and nothing is written outside
    the outputs, with a shared and with a per-row prior mean"""
    rng = np.random.default_rng(1700 + D)
    N = 37
    s_t, G_t = _sums(ctx, D, ctx.tensor(rng.standard_normal((5, D))))
    Lam_t = ctx.tensor(-1e6 * np.eye(D))
    ctx.sync()
    from bdf_amd._lib import lib
    for is_matrix in (False, True):
        mu_t = ctx.tensor(rng.standard_normal((N, D)) if is_matrix else rng.standard_normal(D))
        rc, Le_t, me_t, pk_t, ar_t = _prior_call(ctx, D, N, [(s_t, G_t, 2.0, None, 0.25, -0.7)], mu_t, is_matrix, Lam_t)
        assert rc == 0
        with pytest.raises(B.NotPositiveDefinite):
            ctx.sync()
        ctx.sync()                                     # the flag is cleared
        assert _untouched(Le_t, D) and _untouched(me_t, N if is_matrix else D)
        assert pk_t is None or _untouched(pk_t, lib().bdf_prior_pack_doubles(D))
        ar = ar_t.cpu().numpy()
        assert ar[0] == 2.0 * 0.75 and np.all(np.isnan(ar[1:]))
        assert np.array_equal(Le_t.cpu().numpy()[:D], -1e6 * np.eye(D) + 0.5 * G_t.cpu().numpy())
    # the context is good for the next fold
    rc, Le_t, me_t, _, _ = _prior_call(ctx, D, N, [(s_t, G_t, 2.0, None, 0.25, -0.7)], ctx.tensor(rng.standard_normal(D)), False, ctx.tensor(np.eye(D)))
    assert rc == 0
    ctx.sync()
    assert np.all(np.isfinite(me_t.cpu().numpy()[:D]))
