"""Dense relations (setDense) on the GPU.  The oracle is the existing code on the explicit listing: the same
matrix listed cell by cell has, with the same seed, the same row normals and the same alpha stream, so the same chain up to rounding.
The two products against math.fsum, the prior and the row systems against the explicit call, alpha's closed-form sum of squares
against math.fsum over all cells (also past 256 partial sums), the row means past one wave and one workgroup, whole chains on both iteration paths, and the C ABI's refusals."""
import ctypes as C
import math
import os
import textwrap

import numpy as np
import pytest

from both_paths import child
import background_restatement as BR
import dense_restatement as DR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1234
DS = [3, 16, 17, 32, 33, 64]
# A product workgroup owns 16 rows of the result and its 8 waves take 16 contraction indices each per trip: (17, .) is the smallest
# shape with a second workgroup, 129 the smallest contraction length at which a wave takes a second trip -- (130, 129) has both for
# either orientation.
SHAPES = [(1, 1), (15, 3), (16, 4), (17, 5), (37, 29), (64, 64), (65, 67), (130, 129)]


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _prior(rng, D):
    A = rng.standard_normal((D, D))
    return A @ A.T / D + np.eye(D)


def _product(B, c2, R_t, N, M, D, F_t, transpose, guard=0):
    from bdf_amd._lib import check, lib
    T = M if transpose else N
    out = c2.tensor(np.full((T + guard, D), np.nan))
    check(lib().bdf_dense_product(c2.handle, _p(R_t), N, M, D, _p(F_t), int(transpose), _p(out)))
    return out


# ---- (a) the two products ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("D", DS)
def test_products_against_fsum(B, D, transpose):
    """C = R V and C' = R' U at every shape: each element to 1e-13 of sum |r| |v| (at most 130 terms in float64, each product and each
    partial sum rounded once: 131 x 2^-53 = 1.5e-14 in the worst case), 16 guard rows of NaN behind the result untouched, two runs the same bits"""
    c2 = B.Context(seed=SEED)
    for N, M in SHAPES:
        rng = np.random.default_rng(1000 * D + 10 * N + M + int(transpose))
        R = rng.standard_normal((N, M))
        F = rng.standard_normal(((N if transpose else M), D))
        R_t, F_t = c2.tensor(R), c2.tensor(F)
        o1 = _product(B, c2, R_t, N, M, D, F_t, transpose, guard=16)
        o2 = _product(B, c2, R_t, N, M, D, F_t, transpose, guard=16)
        c2.sync()
        g1, g2 = o1.cpu().numpy(), o2.cpu().numpy()
        T = M if transpose else N
        assert np.all(np.isnan(g1[T:])) and np.array_equal(g1[:T], g2[:T])
        ref, mag = DR.product_reference(R, F, transpose)
        err = (np.abs(g1[:T] - ref) / mag).max()
        print(f"dense product D={D} transpose={transpose} N={N} M={M}: max error {err:.2e} of sum |r v|")
        assert np.all(np.isfinite(g1[:T])) and err <= 1e-13, (N, M, err)
    c2.close()


def test_product_layout_with_an_asymmetric_operand(B):
    """R = I (and a shifted identity) against an asymmetric F: the result is F's rows where they belong, exactly"""
    c2 = B.Context(seed=SEED)
    N, D = 48, 32
    F = np.arange(N * D, dtype=np.float64).reshape(N, D) + 1.0
    for shift in (0, 5):
        R = np.roll(np.eye(N), shift, axis=1)
        R_t, F_t = c2.tensor(R), c2.tensor(F)
        a, b = _product(B, c2, R_t, N, N, D, F_t, False), _product(B, c2, R_t, N, N, D, F_t, True)
        c2.sync()
        assert np.array_equal(a.cpu().numpy(), R @ F) and np.array_equal(b.cpu().numpy(), R.T @ F)
    c2.close()


# ---- (b) the prior and the row systems ---------------------------------------------------------------------------------------------------
def _terms(specs):
    from bdf_amd._lib import Term
    terms = (Term * len(specs))()
    for t, s in zip(terms, specs):
        t.rel, t.mode, t.alpha, t.mean_value = s["rel"].handle, s["mode"], s["alpha"], s["mean"]
        t.obs_precision = s["weights"].data_ptr() if s.get("weights") is not None else None
        t.alpha_dev = s["alpha_dev"] if s.get("alpha_dev") is not None else None
        t.factors[1 - s["mode"]] = s["other"].data_ptr()
    return terms


@pytest.mark.parametrize("terms", ["dense", "dense+dense", "dense+sparse", "sparse+dense", "dense+background"])
@pytest.mark.parametrize("D", DS)
def test_row_systems_of_a_dense_entity_equal_the_explicit_call(B, D, terms):
    """bdf_row_system with (Lambda_eff, mu_eff) of bdf_dense_prior and the entity's other terms -- the dense relations themselves are
    empty relations there -- against the existing code on the explicit listing, for the rows of both modes at N = 37, M = 29, a shared
    and a per-row prior mean: to 1e-12 max |P|"""
    from bdf_amd._lib import DenseTerm, check, lib
    rng = np.random.default_rng(700 + D)
    N, M = 37, 29
    c2 = B.Context(seed=SEED)
    Lam = _prior(rng, D)
    Lam_t = c2.tensor(Lam)
    worst = 0.0
    for mode0 in (0, 1):
        n = (N, M)[mode0]
        kinds = terms.split("+")
        folded, explicit, dts, keep = [], [], [], []
        for k, kind in enumerate(kinds):
            dims = [N, M]
            if k > 0:
                dims[1 - mode0] = 23                       # the second relation has another entity on its other side
            m = dims[1 - mode0]
            other = 0.5 * rng.standard_normal((m, D))
            other_t = c2.tensor(other)
            alpha = 1.7 - 0.6 * k
            keep.append(other_t)
            if kind == "dense":
                Y = DR.table(dims[0], dims[1], seed=D + k)
                mean = float(Y.mean())
                ids, y = DR.listing(Y)
                R_t = c2.tensor(Y - mean)
                C_t = _product(B, c2, R_t, dims[0], dims[1], D, other_t, bool(mode0))
                G_t, s_t = c2.zeros(D, D), c2.zeros(D)
                check(lib().bdf_hyper_sums(c2.handle, D, m, _p(other_t), None, _p(s_t), _p(G_t)))
                dts.append(dict(gram=G_t, C=C_t, sum=None, alpha=alpha, weight=1.0, resid=0.0))
                empty = B.DeviceRelation(c2, B.IndexedDF((ids[:0], y[:0]), dims))
                folded.append(dict(rel=empty, mode=mode0, alpha=alpha, mean=mean, other=other_t))
                explicit.append(dict(rel=B.DeviceRelation(c2, B.IndexedDF((ids, y), dims)), mode=mode0, alpha=alpha, mean=mean, other=other_t))
                keep += [R_t, C_t, G_t, s_t]
            elif kind == "sparse":
                ids, y, _ = BR.listing(dims[0], dims[1])
                rel = B.DeviceRelation(c2, B.IndexedDF((ids, y), dims))
                spec = dict(rel=rel, mode=mode0, alpha=alpha, mean=float(y.mean()), other=other_t)
                folded.append(spec)
                explicit.append(spec)
            else:
                ids, y, w = BR.listing(dims[0], dims[1])
                c0, value = 0.3, -0.5
                mean = BR.all_cells_mean(dims[0], dims[1], y, value)
                rb = value - mean
                ida, ya, wa = BR.dense_listing(dims[0], dims[1], ids, y, w, c0, value)
                G_t, s_t, wa_t = c2.zeros(D, D), c2.zeros(D), c2.tensor(wa)
                check(lib().bdf_hyper_sums(c2.handle, D, m, _p(other_t), None, _p(s_t), _p(G_t)))
                dts.append(dict(gram=G_t, C=None, sum=s_t, alpha=alpha, weight=c0, resid=rb))
                listed = B.DeviceRelation(c2, B.IndexedDF((ids, BR.unit_values(y, mean, c0, rb)), dims))
                folded.append(dict(rel=listed, mode=mode0, alpha=alpha, mean=mean, other=other_t, alpha_rows=len(dts) - 1))
                explicit.append(dict(rel=B.DeviceRelation(c2, B.IndexedDF((ida, ya), dims)), mode=mode0, alpha=alpha, mean=mean, other=other_t,
                                     weights=wa_t))
                keep += [G_t, s_t, wa_t]
        arr = (DenseTerm * len(dts))()
        for a, d in zip(arr, dts):
            a.gram, a.C, a.sum = d["gram"].data_ptr(), (d["C"].data_ptr() if d["C"] is not None else None), (d["sum"].data_ptr() if d["sum"] is not None else None)
            a.alpha, a.weight, a.resid = d["alpha"], d["weight"], d["resid"]
        for is_matrix in (False, True):
            mu = rng.standard_normal((n, D)) if is_matrix else rng.standard_normal(D)
            mu_t = c2.tensor(mu)
            Le_t, me_t, ar_t = c2.zeros(D, D), c2.tensor(np.full((n + 16, D), np.nan)), c2.tensor(np.full(4, np.nan))
            check(lib().bdf_dense_prior(c2.handle, D, n, len(dts), arr, _p(mu_t), int(is_matrix), _p(Lam_t), _p(Le_t), _p(me_t), _p(ar_t)))
            for s in folded:
                if "alpha_rows" in s:
                    s["alpha_dev"] = ar_t.data_ptr() + 8 * s["alpha_rows"]
            P_t, b_t, Pd_t, bd_t = c2.zeros(n, D, D), c2.zeros(n, D), c2.zeros(n, D, D), c2.zeros(n, D)
            check(lib().bdf_row_system(c2.handle, D, n, len(folded), _terms(folded), _p(me_t), 1, _p(Le_t), _p(P_t), _p(b_t)))
            check(lib().bdf_row_system(c2.handle, D, n, len(explicit), _terms(explicit), _p(mu_t), int(is_matrix), _p(Lam_t), _p(Pd_t), _p(bd_t)))
            c2.sync()
            P, b, Pd, bd, me = (t.cpu().numpy() for t in (P_t, b_t, Pd_t, bd_t, me_t))
            assert np.all(np.isnan(me[n:])) and np.all(np.isfinite(me[:n]))           # 16 guard rows behind mu_eff
            scale = np.abs(Pd).max()
            eP, eb = np.abs(P - Pd).max() / scale, np.abs(b - bd).max() / scale
            worst = max(worst, eP, eb)
            print(f"dense row systems D={D} terms={terms} mode={mode0} matrix mean={is_matrix}: |dP| {eP:.2e} |db| {eb:.2e} of max |P| = {scale:.1f}")
            assert eP <= 1e-12 and eb <= 1e-12, (mode0, is_matrix, eP, eb)
        for s in folded + explicit:
            s["rel"].close()
    c2.close()


def test_prior_alone_against_numpy(B):
    """Lambda_eff and mu_eff of one dense term against the restatement (dense_restatement.systems_dense) solved in numpy, alpha as an
    argument and read from alpha_dev: the same bits either way; a prior precision that is not positive definite sets the flag"""
    from bdf_amd._lib import DenseTerm, check, lib
    c2 = B.Context(seed=SEED)
    for D in (7, 32, 64):
        rng = np.random.default_rng(D)
        N, M, alpha = 37, 29, 2.5
        Y = DR.table(N, M)
        R, V, Lam, mus = Y - Y.mean(), rng.standard_normal((M, D)), _prior(rng, D), rng.standard_normal((N, D))
        R_t, V_t, Lam_t, mus_t = c2.tensor(R), c2.tensor(V), c2.tensor(Lam), c2.tensor(mus)
        C_t = _product(B, c2, R_t, N, M, D, V_t, False)
        G_t, s_t = c2.zeros(D, D), c2.zeros(D)
        check(lib().bdf_hyper_sums(c2.handle, D, M, _p(V_t), None, _p(s_t), _p(G_t)))
        got = []
        for a_arg, a_dev in ((alpha, None), (123.0, c2.tensor([alpha]))):
            arr = (DenseTerm * 1)()
            arr[0].gram, arr[0].C, arr[0].alpha, arr[0].weight = G_t.data_ptr(), C_t.data_ptr(), a_arg, 1.0
            arr[0].alpha_dev = a_dev.data_ptr() if a_dev is not None else None
            Le_t, me_t, ar_t = c2.zeros(D, D), c2.zeros(N, D), c2.zeros(1)
            check(lib().bdf_dense_prior(c2.handle, D, N, 1, arr, _p(mus_t), 1, _p(Lam_t), _p(Le_t), _p(me_t), _p(ar_t)))
            c2.sync()
            got.append((Le_t.cpu().numpy(), me_t.cpu().numpy(), ar_t.cpu().numpy()))
        P, b = DR.systems_dense([R], [V], [alpha], Lam, mus)
        Le, me, ar = got[0]
        want = np.linalg.solve(P, b.T).T
        kappa = np.linalg.cond(P)
        err = np.abs(me - want).max() / np.abs(want).max()
        print(f"dense prior D={D}: kappa {kappa:.1f}, forward error of mu_eff {err:.2e}")
        assert np.abs(Le - P).max() <= 1e-13 * np.abs(P).max() and ar[0] == alpha
        assert err <= 8 * D * kappa * 2.0 ** -52                                  # the bound test_gpu_background.py holds its fold to
        for x, y in zip(got[0], got[1]):
            assert np.array_equal(x, y)
    # not positive definite: Lambda = -100 I beside a small Gram term
    arr[0].alpha_dev = None
    arr[0].alpha = 1e-3
    bad = c2.tensor(-100.0 * np.eye(D))
    check(lib().bdf_dense_prior(c2.handle, D, N, 1, arr, _p(mus_t), 1, _p(bad), _p(Le_t), _p(me_t), _p(ar_t)))
    with pytest.raises(B.NotPositiveDefinite):
        c2.sync()
    c2.sync()                                                  # (raised once)
    c2.close()


# ---- (c) alpha's sum of squares ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(37, 29), (130, 129)])
@pytest.mark.parametrize("D", DS)
def test_closed_form_sum_of_squares_and_the_alpha_drawn_from_it(B, D, shape):
    """bdf_dense_sse from C = R V and the two Gram matrices against math.fsum over all cells: to 1e-12 of the sum of the closed form's
    pieces (sum r^2 + 2 |sum u.C| + <U'U, V'V>); twice: the same bits.  alpha drawn from it against alpha drawn from the fsum: alpha
    is a gamma variate over (lambda0 nu0 + sum) -- the same relative bound, taken of the pieces over the sum"""
    from bdf_amd._lib import check, lib
    N, M = shape
    rng = np.random.default_rng(50 + D)
    Y = DR.table(N, M, seed=D)
    R, U, V = Y - Y.mean(), 0.5 * rng.standard_normal((N, D)), 0.5 * rng.standard_normal((M, D))
    c2 = B.Context(seed=SEED)
    R_t, U_t, V_t = c2.tensor(R), c2.tensor(U), c2.tensor(V)
    C_t = _product(B, c2, R_t, N, M, D, V_t, False)
    g = [c2.zeros(D, D), c2.zeros(D, D)]
    s_t = c2.zeros(D)
    for t, f in zip(g, (U_t, V_t)):
        check(lib().bdf_hyper_sums(c2.handle, D, f.shape[0], _p(f), None, _p(s_t), _p(t)))
    r2 = math.fsum((R * R).ravel().tolist())
    ref = DR.sse_explicit(R, U, V)
    out = c2.tensor([np.nan, np.nan, ref])
    for k in (0, 1):
        check(lib().bdf_dense_sse(c2.handle, D, N, _p(U_t), _p(C_t), _p(g[0]), _p(g[1]), r2, None, C.c_void_p(out.data_ptr() + 8 * k)))
    c2.set_sweep(2)
    al = c2.tensor([np.nan, np.nan])
    check(lib().bdf_sample_alpha(c2.handle, 1.0, 2.0, N * M, C.c_void_p(out.data_ptr()), 1, C.c_void_p(al.data_ptr())))
    check(lib().bdf_sample_alpha(c2.handle, 1.0, 2.0, N * M, C.c_void_p(out.data_ptr() + 16), 1, C.c_void_p(al.data_ptr() + 8)))
    c2.sync()
    s, a = out.cpu().numpy(), al.cpu().numpy()
    p = DR.sse_pieces(R, U, V)
    pieces = p[0] + 2.0 * abs(p[1]) + p[2]
    print(f"dense sse D={D} N={N} M={M}: closed form {s[0]:.15g} fsum {ref:.15g}, error {abs(s[0] - ref) / pieces:.2e} of the pieces; alpha {a[0]:.15g} {a[1]:.15g}")
    assert s[0] == s[1] and abs(s[0] - ref) <= 1e-12 * pieces
    assert a[0] > 0 and abs(a[0] - a[1]) <= 1e-12 * (pieces / ref) * a[1]
    c2.close()


DOT_SLAB = 4096                                              # elements of U and C a workgroup of k_dmat_dot takes (csrc/k_dense.hip)
FINAL = 256                                                  # threads of k_dmat_sse_final: the partial sums it adds in one pass


@pytest.mark.parametrize("D,N", [(64, 16385), (33, -(-(FINAL * DOT_SLAB + 1) // 33))])
def test_closed_form_sum_of_squares_past_256_partial_sums(B, D, N):
    """bdf_dense_sse over N x D elements of U that leave 257 partial sums of u.C, one more than k_dmat_sse_final's 256 threads take in
    one pass: D = 64 with 16385 rows (the last workgroup of k_dmat_dot holds 64 elements) and D = 33 with 31776 (a ragged tail of
    32); M = 3.  Against math.fsum over all cells to 1e-12 of the closed form's pieces, as at the small shapes; twice: the same bits.
    On the CPU first: the kernels' own rounding of sum u.C -- 40 roundings deep: 16 serial fmas, the wave's and the workgroup's
    reductions, then thread 0's two-term serial sum and the final reduction -- stays inside that bound, and the partial sums from
    the 257th on move the reference by more than the bound."""
    from bdf_amd._lib import check, lib
    M = 3
    assert -(-(N * D) // DOT_SLAB) == FINAL + 1 and 0 < N * D - FINAL * DOT_SLAB < DOT_SLAB
    rng = np.random.default_rng(60 + D)
    Y = DR.table(N, M, seed=D)
    R, U, V = Y - Y.mean(), 0.5 * rng.standard_normal((N, D)), 0.5 * rng.standard_normal((M, D))
    p = DR.sse_pieces(R, U, V)
    pieces = p[0] + 2.0 * abs(p[1]) + p[2]
    uc = (U * (R @ V)).ravel()
    assert 40 * 2.0 ** -53 * math.fsum(np.abs(uc).tolist()) <= 1e-12 * pieces
    tail = 2.0 * abs(math.fsum(uc[FINAL * DOT_SLAB:].tolist()))
    assert tail > 1e-12 * pieces, (tail, pieces)
    c2 = B.Context(seed=SEED)
    R_t, U_t, V_t = c2.tensor(R), c2.tensor(U), c2.tensor(V)
    C_t = _product(B, c2, R_t, N, M, D, V_t, False)
    g = [c2.zeros(D, D), c2.zeros(D, D)]
    s_t = c2.zeros(D)
    for t, f in zip(g, (U_t, V_t)):
        check(lib().bdf_hyper_sums(c2.handle, D, f.shape[0], _p(f), None, _p(s_t), _p(t)))
    r2 = math.fsum((R * R).ravel().tolist())
    ref = DR.sse_explicit(R, U, V)
    out = c2.tensor([np.nan, np.nan])
    for k in (0, 1):
        check(lib().bdf_dense_sse(c2.handle, D, N, _p(U_t), _p(C_t), _p(g[0]), _p(g[1]), r2, None, C.c_void_p(out.data_ptr() + 8 * k)))
    c2.sync()
    s = out.cpu().numpy()
    print(f"dense sse D={D} N={N} M={M}: closed form {s[0]:.15g} fsum {ref:.15g}, error {abs(s[0] - ref) / pieces:.2e} of the pieces "
          f"(the last partial sums weigh {tail / pieces:.2e})")
    assert s[0] == s[1] and abs(s[0] - ref) <= 1e-12 * pieces
    c2.close()


@pytest.mark.parametrize("D", [7, 32, 33, 64])
def test_prior_rows_past_one_wave_and_one_workgroup(B, D):
    """k_dmat_mu_rows takes one wave per 16 rows and four waves per workgroup: N = 1, 15, 16, 17 (one wave, its tile short, full, a
    second wave with one row), 48, 49 (the fourth wave idle, with one row), 63, 64, 65 and 130 (a second and a third workgroup), at
    M = 29 with one dense term, the shared and the per-row prior mean.  Lambda_eff to 1e-13 max |P| and mu_eff to the forward bound
    8 D kappa 2^-52 against numpy, as test_prior_alone_against_numpy holds them; 16 guard rows of NaN behind mu_out untouched; a
    rerun gives the same bits.  R's first column and the per-row means' first coordinate carry the row's index, so that C and mu
    differ strongly from row to row: the reference with two neighbouring rows swapped is outside the bound (asserted), and so is
    a tile row stored to another output row."""
    from bdf_amd._lib import DenseTerm, check, lib
    c2 = B.Context(seed=SEED)
    M, alpha = 29, 2.5
    for N in (1, 15, 16, 17, 48, 49, 63, 64, 65, 130):
        rng = np.random.default_rng(1000 * D + N)
        Y = DR.table(N, M, seed=D + N)
        R = Y - Y.mean()
        R[:, 0] += np.arange(N)
        V, Lam = rng.standard_normal((M, D)), _prior(rng, D)
        mus = rng.standard_normal((N, D))
        mus[:, 0] += np.arange(N)
        R_t, V_t, Lam_t = c2.tensor(R), c2.tensor(V), c2.tensor(Lam)
        C_t = _product(B, c2, R_t, N, M, D, V_t, False)
        G_t, s_t = c2.zeros(D, D), c2.zeros(D)
        check(lib().bdf_hyper_sums(c2.handle, D, M, _p(V_t), None, _p(s_t), _p(G_t)))
        arr = (DenseTerm * 1)()
        arr[0].gram, arr[0].C, arr[0].alpha, arr[0].weight = G_t.data_ptr(), C_t.data_ptr(), alpha, 1.0
        for is_matrix in (False, True):
            mu = mus if is_matrix else mus[0]
            mu_t = c2.tensor(mu)
            got = []
            for _ in (0, 1):
                Le_t, me_t, ar_t = c2.zeros(D, D), c2.tensor(np.full((N + 16, D), np.nan)), c2.zeros(1)
                check(lib().bdf_dense_prior(c2.handle, D, N, 1, arr, _p(mu_t), int(is_matrix), _p(Lam_t), _p(Le_t), _p(me_t), _p(ar_t)))
                c2.sync()
                got.append((Le_t.cpu().numpy(), me_t.cpu().numpy(), ar_t.cpu().numpy()))
            Le, me, ar = got[0]
            assert np.all(np.isnan(me[N:])) and np.all(np.isfinite(me[:N])), (N, is_matrix)
            for x, y in zip(got[0], got[1]):
                assert np.array_equal(x, y, equal_nan=True)
            P, b = DR.systems_dense([R], [V], [alpha], Lam, mu)
            want = np.linalg.solve(P, b.T).T
            kappa = np.linalg.cond(P)
            bound = 8 * D * kappa * 2.0 ** -52
            if N > 1:
                swapped = want.copy()
                swapped[[N - 2, N - 1]] = want[[N - 1, N - 2]]
                assert np.abs(swapped - want).max() / np.abs(want).max() > bound
            err = np.abs(me[:N] - want).max() / np.abs(want).max()
            print(f"dense prior rows D={D} N={N} matrix mean={is_matrix}: kappa {kappa:.1f}, forward error of mu_eff {err:.2e} (bound {bound:.2e})")
            assert np.abs(Le - P).max() <= 1e-13 * np.abs(P).max() and ar[0] == alpha
            assert err <= bound, (N, is_matrix, err, bound)
    c2.close()


# ---- (d) errors through the C ABI ---------------------------------------------------------------------------------------------------------
def test_dense_c_abi_errors(B, ctx):
    from bdf_amd._lib import DenseTerm, lib
    D = 4
    z, Z, O2 = ctx.zeros(D), ctx.tensor(np.eye(D)), ctx.zeros(D, D)
    R, F, out, mo, ar = ctx.zeros(3, 5), ctx.zeros(5, D), ctx.zeros(3, D), ctx.zeros(3, D), ctx.zeros(2)
    L = lib()
    assert L.bdf_dense_product(ctx.handle, _p(R), 3, 5, D, _p(F), 0, _p(out)) == 0
    assert L.bdf_dense_product(ctx.handle, _p(R), 3, 5, 0, _p(F), 0, _p(out)) == -1
    assert L.bdf_dense_product(ctx.handle, _p(R), 3, 5, 65, _p(F), 0, _p(out)) == -1
    assert L.bdf_dense_product(ctx.handle, _p(R), 0, 5, D, _p(F), 0, _p(out)) == -1
    assert L.bdf_dense_product(ctx.handle, None, 3, 5, D, _p(F), 0, _p(out)) == -1
    t = (DenseTerm * 2)()
    t[0].gram, t[0].C, t[0].alpha, t[0].weight = Z.data_ptr(), out.data_ptr(), 1.0, 1.0

    def prior(D=D, n=1, mu=z, matrix=0, Lam=Z, Lo=O2, mo=mo):
        return L.bdf_dense_prior(ctx.handle, D, 3, n, t, _p(mu), matrix, _p(Lam), _p(Lo), _p(mo), _p(ar))

    assert prior() == 0
    assert prior(D=0) == -1 and prior(D=65) == -1 and prior(n=0) == -1 and prior(n=5) == -1 and prior(Lo=Z) == -1 and prior(mu=None) == -1
    assert prior(n=2) == -1                                    # the second term has neither C nor sum
    for field, bad in (("weight", 0.5), ("weight", 0.0), ("alpha", 0.0), ("resid", float("nan")), ("gram", None)):
        keep = getattr(t[0], field)
        setattr(t[0], field, bad)
        assert prior() == -1, field
        setattr(t[0], field, keep)
    t[0].C, t[0].sum, t[0].weight = None, z.data_ptr(), 0.5     # a background term alone is bdf_background_prior's
    assert prior() == -1 and b"no dense term" in L.bdf_last_error()
    assert L.bdf_dense_sse(ctx.handle, D, 3, _p(out), _p(out), _p(Z), _p(Z), -1.0, None, _p(ar)) == -1
    assert L.bdf_dense_sse(ctx.handle, D, 3, _p(out), _p(out), _p(Z), _p(Z), 2.0, None, _p(ar)) == 0
    h = ctx.tensor([0.5, 0.0, 0.0, 0.0])
    assert L.bdf_dense_sse(ctx.handle, D, 3, _p(out), _p(out), _p(Z), _p(Z), 2.0, _p(h), C.c_void_p(ar.data_ptr() + 8)) == 0
    ctx.sync()
    assert float(ar[0].item()) == 2.0 + D and float(ar[1].item()) == 2.5 + D      # U = C = 0: sum r^2 (+ the holes') + <I, I>
    p3 = B.DevicePairs(ctx, np.array([[1, 1, 1]], dtype=np.int64), np.zeros(1))
    f3 = (C.c_void_p * 3)(*[F.data_ptr()] * 3)
    assert L.bdf_dense_impute(ctx.handle, p3.handle, D, f3, 1.0, None, 1, _p(R), 3, 5, _p(h)) == -1 and b"two modes" in L.bdf_last_error()
    p2 = B.DevicePairs(ctx, np.array([[2, 3]], dtype=np.int64), np.zeros(1))
    U0 = ctx.zeros(3, D)
    f2 = (C.c_void_p * 2)(U0.data_ptr(), F.data_ptr())
    assert L.bdf_dense_impute(ctx.handle, p2.handle, D, f2, 0.0, None, 1, _p(R), 3, 5, _p(h)) == -1      # alpha must be positive
    assert L.bdf_dense_impute(ctx.handle, p2.handle, D, f2, 4.0, None, 1, _p(R), 3, 5, _p(h)) == 0
    ctx.sync()
    got, st = R.cpu().numpy(), h.cpu().numpy()
    assert got[1, 2] != 0.0 and np.count_nonzero(got) == 1 and st[0] == got[1, 2] ** 2        # u = v = 0: z / 2 and nothing else
    p3.close()
    p2.close()


# ---- (e) the holes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_holes", [0, 1, 7, 8, 9, 257])
@pytest.mark.parametrize("D", [7, 32, 64])
def test_imputation_against_the_restatement(B, O, D, n_holes):
    """bdf_dense_impute at N = 37, M = 29: R after the launch against the imputing map of the restatement on the library's own
    normals (bdf_normals) to 1e-12, the listed cells untouched bit for bit, the returned sum of r^2 against math.fsum to 1e-12;
    the normals themselves against the oracle's stream; alpha as an argument and from alpha_dev, the pairs sorted or not: the same bits"""
    from bdf_amd._lib import P_DENSE, check, lib
    N, M, alpha, tag, sweep = 37, 29, 1.7, 3, 4
    rng = np.random.default_rng(100 * D + n_holes)
    R = rng.standard_normal((N, M))
    U, V = 0.5 * rng.standard_normal((N, D)), 0.5 * rng.standard_normal((M, D))
    cells = rng.choice(N * M, size=n_holes, replace=False)              # (in a shuffled order: the stream is keyed by the caller's index)
    holes = np.stack([cells // M, cells % M], axis=1).astype(np.int64).reshape(n_holes, 2)
    c2 = B.Context(seed=SEED)
    c2.set_sweep(sweep)
    ft = [c2.tensor(U), c2.tensor(V)]
    facs = (C.c_void_p * 2)(*[t.data_ptr() for t in ft])
    z_t = c2.zeros(max(n_holes, 1))
    if n_holes:
        check(lib().bdf_normals(c2.handle, P_DENSE, 0x800000 | tag, 0, n_holes, 1, _p(z_t)))
    got = []
    for a_arg, a_dev, sort in ((alpha, None, False), (99.0, c2.tensor([alpha]), True)):
        R_t = c2.tensor(np.concatenate([R.ravel(), np.full(16, np.nan)]))          # 16 guard doubles behind R
        pairs = B.DevicePairs(c2, holes + 1, np.zeros(n_holes))
        if sort and n_holes:
            pairs.sort(1)
        st = c2.tensor(np.full(4, np.nan))
        check(lib().bdf_dense_impute(c2.handle, pairs.handle, D, facs, a_arg, _p(a_dev), tag, _p(R_t), N, M, _p(st)))
        c2.sync()
        got.append((R_t.cpu().numpy(), st.cpu().numpy()))
        pairs.close()
    z = z_t.cpu().numpy()[:n_holes]
    if n_holes:
        assert np.allclose(z, DR.hole_normals(SEED, sweep, tag, n_holes), rtol=1e-12, atol=1e-14)
    want = DR.impute(R, holes, U, V, alpha, z)
    Rg, st = got[0]
    assert np.all(np.isnan(Rg[N * M:]))
    Rg = Rg[:N * M].reshape(N, M)
    mask = np.zeros((N, M), dtype=bool)
    mask[holes[:, 0], holes[:, 1]] = True
    assert np.array_equal(Rg[~mask], R[~mask])
    err = np.abs(Rg - want).max() / max(1.0, np.abs(want).max())
    r2 = math.fsum((want[mask] ** 2).tolist())
    print(f"dense imputation D={D} holes={n_holes}: max error {err:.2e}; sum r^2 {st[0]:.15g} against {r2:.15g}")
    assert err <= 1e-12 and abs(st[0] - r2) <= 1e-12 * max(r2, 1.0) and np.array_equal(st[1:], np.zeros(3))
    assert np.array_equal(got[0][0][:N * M], got[1][0][:N * M]) and abs(got[0][1][0] - got[1][1][0]) <= 1e-12 * max(r2, 1.0)
    c2.close()


# ---- (f) chains --------------------------------------------------------------------------------------------------------------------------
# (D, alpha sampled, what): "plain" N = 37, M = 29; "wide" N = 130, M = 45 (a second trip of the transposed product); "feat" a dense
# 37 x 4 feature matrix on the first entity; "shared" the first entity also in a sparse relation with a third entity
# "three" the first entity in the dense panel, as the SECOND mode of another dense relation and in a relation with a background
CASES = ([(D, a, "plain") for D in (5, 32, 40) for a in (0, 1)] + [(32, 1, "wide"), (5, 1, "feat"), (5, 0, "shared"), (32, 1, "shared")] +
         [(5, 1, "three"), (32, 0, "three")])
# How far the explicit run moves from itself when its rows are listed in a permuted order, over the chain cases (max |difference| /
# max(1, max |value|) over samples, predictions and the alpha trace after 3 + 3 iterations): the reference's own rounding floor,
# measured on an MI355X.  The dense runs are held to ten times that, and to 1e-6 at most.
FLOOR = 2.0e-14            # (the 12 cases: 1.8e-15 .. 2.0e-14, the largest at N = 130, D = 32 with a sampled alpha; the dense runs: 1.6e-15 .. 1.0e-13)
CHAIN_TOL = min(10.0 * FLOOR, 1e-6)

CHILD = textwrap.dedent('''
    import os, sys
    import numpy as np
    sys.path.insert(0, %r); sys.path.insert(0, %r)
    import bdf_amd as B
    import background_restatement as BR
    import dense_restatement as DR
    out, d = sys.argv[1], {}
    cases = %r

    def run(key, D, alpha_sample, what, how):
        N, M = (130, 45) if what == "wide" else (37, 29)
        Y = DR.table(N, M, seed=7)
        rng = np.random.default_rng(11)
        cells = rng.choice(N * M, size=40, replace=False)
        test, test_y = np.stack([cells // M + 1, cells %% M + 1], axis=1), rng.standard_normal(40)
        F = rng.standard_normal((N, 4)) if what == "feat" else None
        ents = [B.Entity("u", F=F), B.Entity("v")]
        ids, y = DR.listing(Y)
        if how == "dense":
            rel = B.denseRelation(Y, "panel", ents, alpha=2.0)
        else:
            p = np.random.default_rng(3).permutation(N * M) if how == "perm" else np.arange(N * M)
            rel = B.Relation({"u": ids[p, 0], "v": ids[p, 1], "y": y[p]}, "panel", ents, alpha=2.0, dims=[N, M])
        rel.model.alpha_sample = bool(alpha_sample)
        B.setTest(rel, {"u": test[:, 0], "v": test[:, 1], "y": test_y})
        rd = B.RelationData(rel)
        if what == "shared":
            i2, y2, _ = BR.listing(N, 23)
            r2 = B.Relation({"u": i2[:, 0], "w": i2[:, 1], "y": y2}, "side", [ents[0], B.Entity("w")], alpha=1.5, dims=[N, 23])
            r2.model.alpha_sample = bool(alpha_sample)
            B.addRelation(rd, r2)
        if what == "three":
            Y2 = DR.table(23, N, seed=8)
            w = B.Entity("w")
            if how == "dense":
                r2 = B.denseRelation(Y2, "plate", [w, ents[0]], alpha=1.5)
            else:
                i2, y2 = DR.listing(Y2)
                p2 = np.random.default_rng(4).permutation(len(y2)) if how == "perm" else np.arange(len(y2))
                r2 = B.Relation({"w": i2[p2, 0], "u": i2[p2, 1], "y": y2[p2]}, "plate", [w, ents[0]], alpha=1.5, dims=[23, N])
            i3, y3, _ = BR.listing(N, 31)
            r3 = B.Relation({"u": i3[:, 0], "x": i3[:, 1], "y": y3}, "plays", [ents[0], B.Entity("x")], alpha=1.2, dims=[N, 31])
            B.setBackground(r3, 0.3, -0.5)
            for r in (r2, r3):
                r.model.alpha_sample = bool(alpha_sample)
                B.addRelation(rd, r)
        res = B.macau(rd, num_latent=D, burnin=3, psamples=3, verbose=False, seed=91,
                      f=lambda data: float(data.relations[0]._dev.alpha_dev.item()))
        d[key + "native"] = np.array(int(rd._engine.native))
        d[key + "pred"], d[key + "trace"] = res["predictions"]["pred"].to_numpy(), np.array(res["f_output"])
        d[key + "mean"], d[key + "alpha"] = np.array(rel.model.mean_value), np.array(rel.model.alpha)
        for k, en in enumerate(rd.entities):
            d[key + "S%%d" %% k] = en.model.sample.T
        d[key + "cells"] = np.array(res["dense"]["panel"]["cells"] if "dense" in res else -1)
        rd._engine.close()

    for D, alpha_sample, what in cases:
        key = "%%d%%d%%s_" %% (D, alpha_sample, what)
        run(key + "dense_", D, alpha_sample, what, "dense")
        run(key + "explicit_", D, alpha_sample, what, "explicit")
        if not os.environ.get("BDF_NO_NATIVE"):
            run(key + "perm_", D, alpha_sample, what, "perm")
    np.savez(out, **d)
''') % (ROOT, os.path.join(ROOT, "tests"), CASES)


@pytest.fixture(scope="module")
def chains():
    """3 + 3 iterations of every case on the native and on the step-by-step path: one child process per path"""
    return child(CHILD, no_native=False), child(CHILD, no_native=True)


def _take(ch, key):
    return {k[len(key):]: v for k, v in ch.items() if k.startswith(key)}


def _distance(a, b):
    """max |difference| / max(1, max |value|) over the samples, the test predictions and the alpha trace of two runs"""
    keys = [k for k in a if k[0] == "S"] + ["pred", "trace", "alpha"]
    return max(np.abs(a[k] - b[k]).max() / max(1.0, np.abs(b[k]).max()) for k in keys)


@pytest.mark.parametrize("D,alpha_sample,what", CASES)
def test_chains_equal_the_explicit_listing_on_both_paths(chains, D, alpha_sample, what):
    """samples, test predictions and the alpha trace of the dense run against the existing code on the explicit listing, 3 + 3
    iterations, on both iteration paths -- which enqueue the same launches: the same bits"""
    key = "%d%d%s_" % (D, alpha_sample, what)
    nat, step = _take(chains[0], key), _take(chains[1], key)
    for k in nat:
        if not k.endswith("native") and not k.startswith("perm_"):
            assert np.array_equal(nat[k], step[k]), k
    dense, explicit, perm = _take(nat, "dense_"), _take(nat, "explicit_"), _take(nat, "perm_")
    assert dense["native"] == 1 and _take(step, "dense_")["native"] == 0
    assert dense["cells"] == ((130 * 45) if what == "wide" else (37 * 29)) and explicit["cells"] == -1
    assert dense["mean"] == explicit["mean"]
    assert (len(set(dense["trace"])) == 3) == bool(alpha_sample) and np.all(dense["trace"] > 0)
    floor, dist = _distance(perm, explicit), _distance(dense, explicit)
    print(f"dense chain D={D} alpha_sample={alpha_sample} {what}: permuted explicit run {floor:.2e}, dense run {dist:.2e}")
    assert dist <= CHAIN_TOL, (dist, floor)
    assert np.abs(dense["S0"]).max() > 0.1                     # (a chain, not zeros)


HOLES_CHILD = textwrap.dedent('''
    import sys
    import numpy as np
    sys.path.insert(0, %r); sys.path.insert(0, %r)
    import bdf_amd as B
    import dense_restatement as DR
    out, d = sys.argv[1], {}
    for D, alpha_sample in ((5, 0), (32, 1)):
        Y = DR.table(37, 29, seed=7)
        held = np.sort(np.random.default_rng(2).choice(37 * 29, size=215, replace=False)) + 1
        rel = B.denseRelation(Y, "panel", [B.Entity("u"), B.Entity("v")], alpha=2.0)
        rel.model.alpha_sample = bool(alpha_sample)
        B.assignToTest(rel, held)
        rd = B.RelationData(rel)
        res = B.macau(rd, num_latent=D, burnin=3, psamples=3, verbose=False, seed=91, lpd=True, rmse_train=True,
                      f=lambda data: float(data.relations[0]._dev.alpha_dev.item()))
        key = "%%d%%d_" %% (D, alpha_sample)
        d[key + "pred"], d[key + "trace"] = res["predictions"]["pred"].to_numpy(), np.array(res["f_output"])
        d[key + "holes"], d[key + "lpd"], d[key + "rmse_train"] = np.array(res["dense"]["panel"]["holes"]), np.array(res["LPD"]), np.array(res["RMSE_train"])
        for k, en in enumerate(rd.entities):
            d[key + "S%%d" %% k] = en.model.sample.T
        d[key + "R"] = rel._dev.dense["R"].cpu().numpy()
        rd._engine.close()
    np.savez(out, **d)
''') % (ROOT, os.path.join(ROOT, "tests"))


@pytest.fixture(scope="module")
def hole_chains():
    return child(HOLES_CHILD, no_native=False), child(HOLES_CHILD, no_native=True)


@pytest.mark.parametrize("D,alpha_sample", [(5, 0), (32, 1)])
def test_a_chain_with_holes_equals_the_restated_chain(hole_chains, O, D, alpha_sample):
    """20 % of the cells held out by assignToTest are holes, imputed before every iteration: samples, predictions, the alpha trace and
    the imputed matrix against the chain restated from the oracle's row sampler on the explicit listing of the imputed matrix (dense_restatement.run_chain),
    to 1e-9 relative / 1e-6 as the other latent-draw models are; both iteration paths: the same bits"""
    key = "%d%d_" % (D, alpha_sample)
    nat, step = _take(hole_chains[0], key), _take(hole_chains[1], key)
    for k in nat:
        assert np.array_equal(nat[k], step[k]), k
    Y = DR.table(37, 29, seed=7)
    held = np.sort(np.random.default_rng(2).choice(37 * 29, size=215, replace=False))
    Yh = Y.copy()
    Yh[held // 29, held % 29] = np.nan
    test_ids = np.stack([held // 29 + 1, held % 29 + 1], axis=1)
    ref = DR.run_chain(Yh, D, 91, 6, alpha=2.0, alpha_sample=bool(alpha_sample), test_ids=test_ids, burnin=3)
    assert nat["holes"] == 215 and np.isfinite(nat["lpd"]) and nat["rmse_train"] > 0
    for got, want, name in ((nat["S0"], ref["S"][0], "U"), (nat["S1"], ref["S"][1], "V"), (nat["pred"], ref["pred"], "pred"),
                            (nat["trace"], ref["trace"][3:], "alpha"), (nat["R"], ref["R"], "R")):
        err = np.abs(got - want).max()
        print(f"dense chain with holes D={D} alpha_sample={alpha_sample}: {name} max |difference| {err:.2e}")
        assert np.allclose(got, want, rtol=1e-9, atol=1e-6), name


# ---- (g) it learns -----------------------------------------------------------------------------------------------------------------------
def test_dense_with_holes_learns_what_the_sparse_path_learns(B):
    """Planted rank-4 data, N = 150, M = 40, noise sd 0.3, 20 % held out, D = 8, alpha = 10 fixed, 20 + 20 iterations: the held-out
    RMSE of the dense chain with imputed holes against the sparse path on the same cells, over chain seeds 0 .. 3.  Both sample the
    same posterior.  The numpy restatement on the CPU (dense_restatement.gibbs_holes_rmse) gave 0.3265 and 0.3270 for seeds 0 and 1
    (the noise floor is 0.3).  The margin is the seed-to-seed spread of the sparse path, max - min over the four seeds: 0.0050 on an
    MI355X, where the means differed by 0.0033 (DESIGN.md section 25 has the values)."""
    Y, held = DR.planted(0)

    def run(dense, seed):
        ents = [B.Entity("u"), B.Entity("v")]
        if dense:
            rel = B.denseRelation(Y, "panel", ents, alpha=10.0)
        else:
            ids, y = DR.listing(Y)
            rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "panel", ents, alpha=10.0, dims=list(Y.shape))
        B.assignToTest(rel, held)
        rd = B.RelationData(rel)
        res = B.macau(rd, num_latent=8, burnin=20, psamples=20, verbose=False, seed=seed)
        rd._engine.close()
        return float(res["RMSE"])

    d, s = [run(True, k) for k in range(4)], [run(False, k) for k in range(4)]
    spread = max(s) - min(s)
    print(f"planted dense data: held-out RMSE dense with holes {np.round(d, 4)}, sparse path {np.round(s, 4)}, spread {spread:.4f}")
    assert abs(np.mean(d) - np.mean(s)) <= spread and max(d) < 0.4
