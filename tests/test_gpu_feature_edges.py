"""The side-information kernels (K2-K5) at their tile and dispatch edges: every size-keyed branch of k_feat_ops.hip, k_feat_cg.hip and
k_feat_beta.hip (and the solvers they hand to, k_feat_eig.hip and k_chol.hip) against a plain float64 numpy / scipy statement of the
same operation -- A @ X, A.T @ Y, np.linalg.solve(A.T @ A + lb I, rhs) with the right-hand side of the CPU oracle's sample_beta on the
same noise streams.  tests/test_gpu_features.py visits the shapes the reference's tests and the benchmark use; this file visits the
shapes at which the dispatch changes.  The inputs are built by tests/feature_edge_inputs.py and checked on the host by
tests/test_feature_edge_inputs_host.py.

Tolerances (those of test_gpu_features.py): products 1e-12 of the largest expected entry; rhs against the oracle 1e-9; beta against
the oracle rtol 1e-7, atol 1e-9 max|beta|; beta from CG against the direct solve rtol 1e-6, atol 1e-7 max|beta|; iteration counts
within 2 of the oracle's (1 on the row-major state, as its existing test has it).  They mean something on well-conditioned systems
only: every solve case asserts cond(A'A + lb I) < 1e4.

THE MAP -- branch (file: function, condition) -> kernel and instantiation -> the case that reaches it
("ops" = k_feat_ops.hip, "cg" = k_feat_cg.hip, "beta" = k_feat_beta.hip)

Operand layouts by entry point (B = the right-hand operand, Y = the output):
  bdf_feat_mul                     B column-major, Y column-major                  (test_dense_products, test_sparse_products)
  bdf_uhat                         B column-major (beta), Y ROW-major + biased Y2  (test_dense_uhat, test_sparse_uhat, test_panel_products)
  bdf_sample_beta, its rhs         transposed product: B ROW-major (T is D x N), Y column-major     (every solve case; test_sparse_rhs)
  feat_cg_solve, two products      F P: B column-major, Y row-major;  F' Tm: B row-major, Y column-major          (test_cg_dense)
  feat_cg_solve, row-major state   both products row-major in and out             (test_cg_sparse[300-8200-2-csr])
  feat_eig_solve / F'F operator    feat_dense_nn on a square matrix, B and Y column-major           (test_direct_solves, test_cg_dense)

ops: feat_apply (k_feat_ops.hip:660; the branches at :663, :664, :679)
  kind 0, ncol <= 64, m, n > 0  -> dense_apply                                     test_dense_products (ncol <= 64), test_dense_uhat
  kind 0, ncol > 64             -> feat_gemm                                       test_dense_products (ncol 65, 70)
  kind 0, m or n == 0           -> feat_gemm returns at once (M or N == 0)         not a kernel: test_gpu_features.py has no such case either
  kind 1 / 2                    -> spmm, with / without values                     test_sparse_products[csr / bin]
ops: dense_apply (:275; forward :279, the CB switch of the transposed product :289)
  forward                       -> feat_dense_nn                                   below
  transposed                    -> k_dense_tn<CB>, CB = ceil(ncol / 16) = 1 .. 4, then k_gemm_reduce (always: one chunk or several)
        CB 1: (1,1,1) (17,5,16) (250,65,15) (17,16,1)   CB 2: (17,17,17) (250,63,32) (250,5,17)
        CB 3: (15,65,33) (17,130,48) (1,16,33) (15,3,48)      CB 4: (250,17,49) (17,63,64) (250,130,64) (15,1,64)
        -- (rows of F, numF, ncol) of test_dense_products; the rows are the K of this direction (1, 15, 17: one 64-row tile with a
        tail; 250: four tiles, the last a tail), numF its output rows (1, 3, 5: one tile of 16 features with a tail; 17, 63, 65, 130)
        B row-major: the rhs of test_direct_solves / test_cg_dense (D = 1 .. 64: every CB)
ops: feat_dense_nn (:256; CM :260, the CB switch :264)
  CB = 1 .. 4 x CM (B column-major: brs == 1 and bcs != 1)
        k_dense_nn<CB, true>: the same fifteen shapes, forward (K = numF: 1, 3, 5 < 16; 16, 17; 63, 65, 130 split over four waves,
        K < 64 leaves waves without work; rows 1, 15, 17, 250: row tails);  row-major Y + Y2: test_dense_uhat D = 1, 17, 33, 64
        k_dense_nn<CB, false>: B has bcs == 1, which bdf_feat_mul gives for numF == 1: (1,1,1) CB 1, (15,1,64) CB 4 -- the only
        single-rank callers with another layout are the row-major CG products, which are sparse.  CB 2, 3 with CM false: no caller.
ops: feat_gemm (:83; the split-K condition :88)
  tiles >= 512 or K < 128       -> k_gemm in one pass                              test_dense_products (17,5,65) both ways, (15,63,65),
                                                                                   (250,3,70) forward; F'F of test_direct_solves[705-17] (529 tiles)
  tiles < 512 and K >= 128      -> k_gemm split-K + k_gemm_reduce                  test_dense_products (250,130,70) both ways, (250,3,70)
                                                                                   transposed; F'F of every other solve case (K = 300 rows)
ops: spmm (:587; layouts :590, wide :607, panels :617, the general kernel :652, the transpose back :654)
  B not row-major               -> k_to_rowmajor                                   test_sparse_products ncol >= 2 (ncol == 1 counts as row-major)
  Y not row-major               -> k_from_rowmajor (+ the biased copy: no caller asks a column-major Y for Y2)   the same
  wide (even ncol 2 .. 32)      -> k_spmm_rm16<HASV>                               test_sparse_products ncol 2, 16, 30, 32; test_sparse_uhat D 2, 32 (Y2, row tail)
  otherwise                     -> k_spmm_rm                                       ncol 1, 3, 33, 34, 64, 65; test_sparse_uhat D 17, 64 (Y2); test_sparse_rhs D 33
  wide, >= 2 panels, B >= 8 MiB -> k_spmm_rm16p<HASV>                              test_panel_products (ncol 32, 30, both ways; bdf_uhat D = 32: Y2)
  wide, panels but B < 8 MiB    -> k_spmm_rm16                                     test_panel_products' operator at ncol = 2 (0.6 MiB)
beta: bdf_sample_beta_ranks, single rank (k_feat_beta.hip:221; DP :232 / :250, the solver chain :263-267, ff_op :274, ranks :279)
  DP = 16 / 32 / 64             -> k_noise_prep<DP>, k_noise_rows<DP>              D 1, 16 / 17, 32, 33 / 64 of test_direct_solves
  use_ff, numF <= 16 / 32 / 64  -> k_solve_small<16 / 32 / 64>                     test_direct_solves numF 1, 15, 16 / 17, 31, 32 / 33, 63, 64
  use_ff, numF <= 640           -> feat_eig_solve                                  numF 65, 130, 640
  use_ff, above (or BDF_NO_EIG) -> bdf_chol_solve                                  numF 641, 704, 705; 65, 128, 129 under BDF_NO_EIG
        k_chol_backward groups of 16 right-hand sides: 1 (D 1), 2 (D 17), 3 (D 33), 4 (D 64)
  CG, ff_op (numF <= 1024 and numF^2 <= nnz)   -> F'F through feat_ensure_FF       test_cg_dense rows >= numF
  CG, world > 1                 -> multi-rank only
  sample_lambda                 -> k_lambda_beta: test_gpu_features.py::test_lambda_beta_draw_matches_oracle (no size-keyed branch)
beta: bdf_sample_beta_rel_impl (:442; the solver chain :487-490)
  numF <= 16 / 32 / 64 / above  -> k_solve_small<16 / 32 / 64> / bdf_chol_solve    test_sample_beta_rel numF 16 / 17, 32 / 33, 64 / 65
  world > 1 (sum_ff, gather)    -> multi-rank only
cg: feat_cg_solve (k_feat_cg.hip:689; threads :708, resident :711, rm :728, the operator :788-803, the step chain :806-817)
  resident (F'F, 128 <= numF <= 512, D <= min(32, ceil(numF / 16)))   -> k_cg_resident<1 / 2>      test_cg_one_launch_limits (128,8) (129,5) / (512,32)
        just outside: (128, 9) takes k_cg_step_short<2>                            test_cg_one_launch_refused
  rm (sparse, no F'F, numF > 2048, D <= 32)     -> k_cg_rm_zero / _init / _a / _b / _c          test_cg_sparse[300-8200-2-csr] (33 chunks of 256 rows)
  otherwise k_cg_init, k_cg_pre with 256 threads, 1,024 from 8,192 features       1,024: test_cg_sparse[300-8200-33-bin]; 256: every other CG case
        (8,200 sparse features at D <= 32 take the row-major state, so the 1,024-thread kernels need D > 32 or a dense F)
  operator: F'F, D <= 64        -> feat_dense_nn (k_dense_nn<CB, true>)            test_cg_dense (600,512,33) CB 3, (600,513,64) CB 4, (1030,1024,1) CB 1
            F'F, D > 64         -> feat_gemm: no caller (every entry point refuses D > 64)
            rm                  -> two row-major feat_apply                        test_cg_sparse[300-8200-2-csr]
            otherwise           -> feat_apply F P (Y row-major), F' Tm (B row-major)     dense: test_cg_dense rows 300; sparse: test_cg_sparse D 33
  step: numF <= 512             -> k_cg_step_short<2>                              test_cg_dense numF 512
        numF <= 1024            -> k_cg_step_short<4>                              numF 513, 1024
        numF <= 2048            -> k_cg_step_short<8>                              numF 1025, 2048
        rm                      -> k_cg_rm_a / _b / _c                             above
        otherwise               -> k_cg_long_a / _b / _c                           test_cg_dense numF 2049 (one chunk), test_cg_sparse[300-2600-33-csr] (one chunk),
                                                                                   [300-8200-33-bin] (three chunks)
  BDF_CG_STAMPS (:191)          -> diagnostic build only
(line numbers as of the commit that added this file: the conditions beside them are what to look for)
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile
import textwrap
import warnings

import numpy as np
import pytest

import feature_edge_inputs as I

pytestmark = pytest.mark.gpu
SEED = 1234            # the ctx fixture's seed


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _colmajor(ctx, A):
    """numpy (rows, cols) -> torch tensor holding the column-major matrix (shape (cols, rows))"""
    return ctx.tensor(np.ascontiguousarray(np.asarray(A, dtype=np.float64).T))


def _from_colmajor(t):
    return t.cpu().numpy().T


def _product_error(got, exp, what):
    """asserts |got - exp| <= 1e-12 max|exp| entry by entry; -> the largest error relative to max|exp|"""
    scale = max(np.abs(exp).max(), np.finfo(np.float64).tiny)
    assert got.shape == exp.shape, what
    np.testing.assert_allclose(got, exp, rtol=0, atol=1e-12 * scale, err_msg=str(what))
    return np.abs(got - exp).max() / scale


def _sample_beta(ctx, op, D, sample, mu, Lam, lb, use_ff, tol=None, tag=3):
    """bdf_sample_beta -> beta, rhs (numF x D), iteration counts; Context.sync raises its warnings under the caller's filter"""
    from bdf_amd._lib import check, lib
    import torch
    S_t, mu_t, Lam_t, lb_t = ctx.tensor(sample), ctx.tensor(mu), ctx.tensor(Lam), ctx.tensor([lb])
    beta_t, rhs_t = ctx.zeros(D, op.n), ctx.zeros(D, op.n)
    it_t = torch.zeros(D, dtype=torch.int32, device=ctx.device)
    check(lib().bdf_sample_beta(ctx.handle, op.handle, D, _p(S_t), _p(mu_t), _p(Lam_t), _p(lb_t), int(use_ff),
                                float("nan") if tol is None else tol, 0, 0, 1e-3, 1.0, tag, _p(beta_t), _p(rhs_t), _p(it_t)))
    ctx.sync()
    return _from_colmajor(beta_t), _from_colmajor(rhs_t), it_t.cpu().numpy()


def _uhat(ctx, op, beta, mu):
    from bdf_amd._lib import check, lib
    D = beta.shape[1]
    beta_t, mu_t = _colmajor(ctx, beta), ctx.tensor(mu)
    uhat_t, mm_t = ctx.zeros(op.m, D), ctx.zeros(op.m, D)
    check(lib().bdf_uhat(ctx.handle, op.handle, D, _p(beta_t), _p(mu_t), _p(uhat_t), _p(mm_t)))
    ctx.sync()
    return uhat_t.cpu().numpy(), mm_t.cpu().numpy()


def _check_uhat(ctx, op, A, D, rng, what):
    beta = rng.standard_normal((A.shape[1], D))
    mu = rng.standard_normal(D)
    uhat, mm = _uhat(ctx, op, beta, mu)
    exp = A @ beta
    return max(_product_error(uhat, exp, (what, "uhat")), _product_error(mm, exp + mu, (what, "mu + uhat")))


# ---- 1. dense operator products ----------------------------------------------------------------------------------------------------
# (rows of F, numF, ncol): both directions each
DENSE_PRODUCTS = [
    (1, 1, 1), (17, 5, 16), (250, 65, 15), (17, 16, 1),                    # CB 1
    (17, 17, 17), (250, 63, 32), (250, 5, 17),                              # CB 2
    (15, 65, 33), (17, 130, 48), (1, 16, 33), (15, 3, 48),                  # CB 3
    (250, 17, 49), (17, 63, 64), (250, 130, 64), (15, 1, 64),               # CB 4
    (17, 5, 65), (15, 63, 65), (250, 130, 70), (250, 3, 70),                # ncol > 64: k_gemm, one pass and split-K
]


def test_dense_products(B, ctx):
    """bdf_feat_mul on a dense F: k_dense_nn<CB, CM> forward, k_dense_tn<CB> + k_gemm_reduce transposed, k_gemm (+ k_gemm_reduce)
    beyond 64 columns -- the map above names the branch of every shape"""
    rng = np.random.default_rng(101)
    worst = 0.0
    for rows, numF, ncol in DENSE_PRODUCTS:
        F = rng.standard_normal((rows, numF))
        X, Y = rng.standard_normal((numF, ncol)), rng.standard_normal((rows, ncol))
        op = B.FeatOperator(ctx, F)
        worst = max(worst, _product_error(_from_colmajor(op.mul(_colmajor(ctx, X))), F @ X, (rows, numF, ncol, "forward")))
        worst = max(worst, _product_error(_from_colmajor(op.mul(_colmajor(ctx, Y), transpose=True)), F.T @ Y, (rows, numF, ncol, "transposed")))
        op.close()
    print(f"feature edges: dense products, largest error {worst:.2e} of the largest entry")


@pytest.mark.parametrize("rows,numF,D", [(17, 5, 1), (250, 63, 17), (15, 65, 33), (250, 130, 64)])
def test_dense_uhat(B, ctx, rows, numF, D):
    """bdf_uhat on a dense F: k_dense_nn<ceil(D / 16), true> writing a ROW-major output and the biased second one (Y2, bias[c])"""
    rng = np.random.default_rng(102 + D)
    F = rng.standard_normal((rows, numF))
    op = B.FeatOperator(ctx, F)
    err = _check_uhat(ctx, op, F, D, rng, (rows, numF, D))
    op.close()
    print(f"feature edges: dense uhat D = {D}, largest error {err:.2e}")


# ---- 2. sparse operator products, CSR and binary -----------------------------------------------------------------------------------
SPARSE_NCOL = [1, 2, 3, 16, 30, 32, 33, 34, 64, 65]


def _edge_operator(B, ctx, kind, transposed_matrix=False):
    rows, cols, vals, A, Abin = I.edge_sparse()
    m, n = I.EDGE_SHAPE
    if transposed_matrix:
        rows, cols, A, Abin, m, n = cols, rows, A.T, Abin.T, n, m
    rows1, cols1 = (rows + 1).astype(np.int32), (cols + 1).astype(np.int32)
    if kind == "bin":
        return B.FeatOperator(ctx, B.SparseBinMatrix(m, n, rows1, cols1)), Abin
    return B.FeatOperator(ctx, B.sparse_csr(rows1, cols1, np.array(vals), m, n)), A


@pytest.mark.parametrize("kind", ["csr", "bin"])
def test_sparse_products(B, ctx, kind):
    """bdf_feat_mul on the 67 x 53 matrix with rows of 0, 1, 4, 15, 16, 17, 32 and 33 entries (the first row 33, the last 17; three
    duplicated entries, summed) and on its transpose (so that the transposed product walks those row lengths too): k_spmm_rm16<HASV>
    for even ncol up to 32, k_spmm_rm otherwise, k_to_rowmajor / k_from_rowmajor around both (67 and 53 rows: a tail in every row
    block of 8, 16 and 32)"""
    rng = np.random.default_rng(201)
    worst = 0.0
    for tm in (False, True):
        op, A = _edge_operator(B, ctx, kind, tm)
        m, n = A.shape
        assert (op.m, op.n) == (m, n)
        for ncol in SPARSE_NCOL:
            X, Y = rng.standard_normal((n, ncol)), rng.standard_normal((m, ncol))
            worst = max(worst, _product_error(_from_colmajor(op.mul(_colmajor(ctx, X))), A @ X, (kind, tm, ncol, "forward")))
            worst = max(worst, _product_error(_from_colmajor(op.mul(_colmajor(ctx, Y), transpose=True)), A.T @ Y, (kind, tm, ncol, "transposed")))
        op.close()
    print(f"feature edges: sparse products ({kind}), largest error {worst:.2e} of the largest entry")


@pytest.mark.parametrize("kind", ["csr", "bin"])
def test_sparse_uhat(B, ctx, kind):
    """bdf_uhat with mu on the same matrix at D = 2, 32 (k_spmm_rm16: Y2 = acc + bias[c], bias[c + 1] with a row tail) and 17, 64
    (k_spmm_rm: Y2 over its column loop): the output is row-major as the caller gave it, only beta passes k_to_rowmajor"""
    rng = np.random.default_rng(202)
    op, A = _edge_operator(B, ctx, kind)
    worst = max(_check_uhat(ctx, op, A, D, rng, (kind, D)) for D in (2, 17, 32, 64))
    op.close()
    print(f"feature edges: sparse uhat ({kind}), largest error {worst:.2e}")


@pytest.mark.parametrize("kind,D", [("csr", 2), ("csr", 33), ("bin", 2), ("bin", 33)])
def test_sparse_rhs(B, O, ctx, kind, D):
    """The right-hand side of bdf_sample_beta on the same matrix: the transposed product takes T row-major (D x N) as it stands and
    leaves a column-major rhs through k_from_rowmajor -- k_spmm_rm16 at D = 2, k_spmm_rm at D = 33; the solve is k_solve_small<64>
    on the F'F that ensure_dense / feat_ensure_FF form from a 53-column product with the identity"""
    op, A = _edge_operator(B, ctx, kind)
    N, numF = A.shape
    sample, mu, Lam = I.solve_inputs(N, D, 203 + D)
    lb = I.lb_of(numF, D)
    assert I.cond_AtA(A, lb) < 1e4
    r, c = np.nonzero(A)
    ctx.set_sweep(5)
    beta_e, rhs_e, _ = O.sample_beta(O.Feat.from_csr(r, c, A[r, c], N, numF), sample, mu, Lam, lb, True, None, SEED, 5, 3)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        beta, rhs, _ = _sample_beta(ctx, op, D, sample, mu, Lam, lb, True)
    np.testing.assert_allclose(rhs, rhs_e, rtol=1e-9, atol=1e-9)
    scale = np.abs(beta_e).max()
    np.testing.assert_allclose(beta, beta_e, rtol=1e-7, atol=1e-9 * scale)
    np.testing.assert_allclose(beta, I.direct_solve(A, lb, rhs_e), rtol=1e-7, atol=1e-9 * scale)
    op.close()
    print(f"feature edges: sparse rhs ({kind}, D = {D}), rhs error {np.abs(rhs - rhs_e).max():.2e}, beta error {np.abs(beta - beta_e).max() / scale:.2e}")


# ---- 3. the panel kernel -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bin", "csr"])
def test_panel_products(B, ctx, kind):
    """k_spmm_rm16p<HASV>: 40,003 x 40,000 (2,500 row blocks and one of three rows; four 12,288-column panels in both directions), 24
    entries per row, a hundred and one rows empty, a hundred and one with 40 entries inside ONE panel (its "rare" inner reload: a row
    with more than sixteen entries in a panel), ncol = 32 and 30 forward and transposed and bdf_uhat at D = 32 (the biased output
    from the panel kernel) against scipy; ncol = 2 is below the 8 MiB of the panel path and takes k_spmm_rm16 on the same operator"""
    import scipy.sparse as sp
    rows, cols, lens, empty, panel_of = I.panel_sparse()
    m, n = I.PANEL_SHAPE
    vals = np.ones(len(rows)) if kind == "bin" else I.panel_values()
    A = sp.csr_matrix((vals, (rows, cols)), shape=(m, n))
    rows1, cols1 = (rows + 1).astype(np.int32), (cols + 1).astype(np.int32)
    op = B.FeatOperator(ctx, B.SparseBinMatrix(m, n, rows1, cols1) if kind == "bin" else B.sparse_csr(rows1, cols1, vals, m, n))
    rng = np.random.default_rng(301)
    worst = 0.0
    for ncol in (32, 30, 2):
        X, Y = rng.standard_normal((n, ncol)), rng.standard_normal((m, ncol))
        fwd = _from_colmajor(op.mul(_colmajor(ctx, X)))
        assert not fwd[empty].any()                      # an empty row is written, as zeros
        worst = max(worst, _product_error(fwd, A @ X, (kind, ncol, "forward")))
        worst = max(worst, _product_error(_from_colmajor(op.mul(_colmajor(ctx, Y), transpose=True)), A.T @ Y, (kind, ncol, "transposed")))
    beta, mu = rng.standard_normal((n, 32)), rng.standard_normal(32)
    uhat, mm = _uhat(ctx, op, beta, mu)
    exp = A @ beta
    worst = max(worst, _product_error(uhat, exp, (kind, "uhat")), _product_error(mm, exp + mu, (kind, "mu + uhat")))
    op.close()
    print(f"feature edges: panel products ({kind}), largest error {worst:.2e} of the largest entry")


# ---- 4. direct solves --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("numF,D,no_eig", I.DIRECT_CASES)
def test_direct_solves(B, O, ctx, monkeypatch, numF, D, no_eig):
    """bdf_sample_beta(use_ff=True) on a dense 300 x numF F: k_solve_small<16 / 32 / 64> up to 64 features, the eigen-solve up to 640,
    the blocked Cholesky above (641: ten blocks and one column; 704: eleven full blocks; 705) and, under BDF_NO_EIG (read on every
    call), at 65, 128 (two full blocks) and 129; every solver at D = 1, at one D in 17 .. 32 and at one above 32.  rhs (k_noise_prep /
    k_noise_rows<16 / 32 / 64>, k_dense_tn<CB> on a row-major operand) and beta against the oracle, beta against numpy's solve, and
    no warning left behind (the PD-failure flags of the factorisations stay clear)"""
    F = I.dense_features(I.DIRECT_ROWS, numF, 400 + numF)
    sample, mu, Lam = I.solve_inputs(I.DIRECT_ROWS, D, 401 + numF + D)
    lb = I.lb_of(numF, D)
    assert I.cond_AtA(F, lb) < 1e4
    if no_eig:
        monkeypatch.setenv("BDF_NO_EIG", "1")
    else:
        monkeypatch.delenv("BDF_NO_EIG", raising=False)
    ctx.set_sweep(6)
    op = B.FeatOperator(ctx, F)
    beta_e, rhs_e, _ = O.sample_beta(O.Feat.from_dense(F), sample, mu, Lam, lb, True, None, SEED, 6, 3)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        beta, rhs, iters = _sample_beta(ctx, op, D, sample, mu, Lam, lb, True)
    monkeypatch.delenv("BDF_NO_EIG", raising=False)
    np.testing.assert_allclose(rhs, rhs_e, rtol=1e-9, atol=1e-9)
    scale = np.abs(beta_e).max()
    np.testing.assert_allclose(beta, beta_e, rtol=1e-7, atol=1e-9 * scale)
    np.testing.assert_allclose(beta, I.direct_solve(F, lb, rhs_e), rtol=1e-7, atol=1e-9 * scale)
    assert not iters.any()
    op.close()
    print(f"feature edges: direct solve numF = {numF}, D = {D}{' (BDF_NO_EIG)' if no_eig else ''}: rhs error {np.abs(rhs - rhs_e).max():.2e}, "
          f"beta error {np.abs(beta - beta_e).max() / scale:.2e} of max|beta|")


@pytest.mark.parametrize("numF", I.REL_NUMF)
def test_sample_beta_rel(B, O, ctx, numF):
    """bdf_sample_beta_rel (one right-hand side): k_solve_small<16> at 16, <32> at 17 and 32, <64> at 33 and 64, the blocked Cholesky
    at 65 (no eigen-solve on this path); the products with one column are k_dense_tn<1> and k_dense_nn<1, true>"""
    from bdf_amd._lib import check, lib
    rng = np.random.default_rng(450 + numF)
    D, dims, n = 5, [25, 18], 500
    ids = np.stack([rng.integers(1, d + 1, n) for d in dims], axis=1)
    y = rng.standard_normal(n) * 2
    facs = [rng.standard_normal((d, D)) * 0.5 for d in dims]
    ft = [ctx.tensor(f) for f in facs]
    Fm = I.dense_features(n, numF, 451 + numF)
    mean, alpha, lam = 0.2, 1.7, 0.8 + numF / 100.0
    assert I.cond_AtA(Fm, lam / alpha) < 1e4
    op = B.FeatOperator(ctx, Fm)
    pairs = B.DevicePairs(ctx, ids, y)
    beta_t, lin_t, rhs_t = ctx.zeros(numF), ctx.zeros(n), ctx.zeros(numF)
    fp = (C.c_void_p * 2)(*[f.data_ptr() for f in ft])
    ctx.set_sweep(4)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        check(lib().bdf_sample_beta_rel(ctx.handle, op.handle, pairs.handle, D, fp, mean, alpha, lam, 2, _p(beta_t), _p(lin_t), _p(rhs_t)))
        ctx.sync()
    res = y - O.predict(ids, facs, mean)
    beta_e, rhs_e = O.sample_beta_rel(O.Feat.from_dense(Fm), res, alpha, lam, SEED, 4, 2)
    beta = beta_t.cpu().numpy()
    scale = np.abs(beta_e).max()
    np.testing.assert_allclose(rhs_t.cpu().numpy(), rhs_e, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(beta, beta_e, rtol=1e-7, atol=1e-9 * scale)
    np.testing.assert_allclose(beta, np.linalg.solve(Fm.T @ Fm + lam / alpha * np.eye(numF), rhs_e / alpha), rtol=1e-7, atol=1e-9 * scale)
    np.testing.assert_allclose(lin_t.cpu().numpy(), mean + Fm @ beta, rtol=1e-11, atol=1e-11)
    op.close()
    pairs.close()
    print(f"feature edges: sample_beta_rel numF = {numF}: beta error {np.abs(beta - beta_e).max() / scale:.2e} of max|beta|")


# ---- 5. CG solves ------------------------------------------------------------------------------------------------------------------
def _check_cg(O, ctx, op, A, ofeat, D, seed, it_margin, what):
    N, numF = A.shape
    sample, mu, Lam = I.solve_inputs(N, D, seed)
    lb = I.lb_of(numF, D)
    assert I.cond_AtA(A, lb) < 1e4
    ctx.set_sweep(8)
    beta_e, rhs_e, it_e = O.sample_beta(ofeat, sample, mu, Lam, lb, False, None, SEED, 8, 3)
    with warnings.catch_warnings():                       # no max-iterations warning is left behind
        warnings.simplefilter("error")
        beta, rhs, iters = _sample_beta(ctx, op, D, sample, mu, Lam, lb, False)
        ctx.sync()
    np.testing.assert_allclose(rhs, rhs_e, rtol=1e-9, atol=1e-9)
    scale = np.abs(beta_e).max()
    np.testing.assert_allclose(beta, beta_e, rtol=1e-7, atol=1e-9 * scale)
    direct = I.direct_solve(A, lb, rhs_e)
    np.testing.assert_allclose(beta, direct, rtol=1e-6, atol=1e-7 * scale)
    assert np.all(np.abs(iters - it_e) <= it_margin), (iters, it_e)
    assert iters.min() >= 4 and iters.max() < numF, iters       # the fused bottom-and-top step ran again and again, and converged
    print(f"feature edges: CG {what}: iterations {iters.min()}..{iters.max()} (oracle {it_e.min()}..{it_e.max()}), rhs error "
          f"{np.abs(rhs - rhs_e).max():.2e}, beta against the oracle {np.abs(beta - beta_e).max() / scale:.2e}, against the direct solve "
          f"{np.abs(beta - direct).max() / scale:.2e} of max|beta|")


@pytest.mark.parametrize("rows,numF,D", I.CG_DENSE_CASES)
def test_cg_dense(B, O, ctx, rows, numF, D):
    """bdf_sample_beta(use_ff=False) on a dense F.  300 rows and more features than rows: numF^2 > nnz, the operator is the two
    products (k_dense_nn<CB, true> into a row-major Tm, k_dense_tn<CB> from it) and the step k_cg_step_short<2> (512), <4> (513,
    1024), <8> (1025, 2048) or k_cg_long_a / _b / _c (2049).  rows >= numF <= 1024: the operator is F'F through feat_dense_nn --
    (600, 512) at D = 33 > 32 so that the one-launch solve does not take it, (600, 513) at D = 64 (k_dense_nn<4>), (1030, 1024)"""
    F = I.dense_features(rows, numF, 500 + numF + rows)
    op = B.FeatOperator(ctx, F)
    _check_cg(O, ctx, op, F, O.Feat.from_dense(F), D, 501 + numF + D, 2, f"dense {rows} x {numF}, D = {D}")
    op.close()


@pytest.mark.parametrize("rows,numF,D,kind", I.CG_SPARSE_CASES)
def test_cg_sparse(B, O, ctx, rows, numF, D, kind):
    """Sparse F, 300 rows, 40 entries each: 2,600 features at D = 33 -- the D = 32 neighbour is the row-major state of
    test_gpu_features.py -- fall to the column-major state with k_spmm_rm products and k_cg_long_* (one chunk); 8,200 features at
    D = 2 take the row-major state (k_cg_rm_*, 33 chunks, k_spmm_rm16 at two columns; iteration counts within 1 as that path's test
    has it); 8,200 binary features at D = 33 take k_cg_init / k_cg_pre with 1,024 threads and k_cg_long_* over three chunks"""
    r, c, v, A = I.sparse_features(rows, numF, I.CG_SPARSE_PER, 550 + numF + D, binary=kind == "bin")
    r1, c1 = (r + 1).astype(np.int32), (c + 1).astype(np.int32)
    op = B.FeatOperator(ctx, B.SparseBinMatrix(rows, numF, r1, c1) if kind == "bin" else B.sparse_csr(r1, c1, v, rows, numF))
    _check_cg(O, ctx, op, A, O.Feat.from_csr(r, c, v, rows, numF), D, 551 + numF + D, 1 if D <= 32 else 2, f"{kind} {rows} x {numF}, D = {D}")
    op.close()


# ---- 6. the one-launch solve at its limits -----------------------------------------------------------------------------------------
_CHILD = textwrap.dedent('''
    import numpy as np, sys, ctypes as C, torch
    sys.path.insert(0, %r); sys.path.insert(0, %r)
    import bdf_amd as B
    import feature_edge_inputs as I
    from bdf_amd._lib import check, lib
    N, numF, D = int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
    F = I.dense_features(N, numF, N + numF + D)
    sample, mu, Lam = I.solve_inputs(N, D, N + numF + D + 1)
    ctx = B.Context(seed=77); ctx.set_sweep(4)
    op = B.FeatOperator(ctx, F)
    p = lambda t: C.c_void_p(t.data_ptr())
    out = {}
    for name, tol in (("tight", float("nan")), ("loose", 1e-4)):
        S_t, mu_t, Lam_t, lb_t = ctx.tensor(sample), ctx.tensor(mu), ctx.tensor(Lam), ctx.tensor([I.RESIDENT_LB])
        beta_t, rhs_t = ctx.zeros(D, numF), ctx.zeros(D, numF)
        it_t = torch.zeros(D, dtype=torch.int32, device=ctx.device)
        check(lib().bdf_sample_beta(ctx.handle, op.handle, D, p(S_t), p(mu_t), p(Lam_t), p(lb_t), 0, tol, 0, 0, 1e-3, 1.0, 3,
                                    p(beta_t), p(rhs_t), p(it_t)))
        ctx.sync()                  # (warnings are errors in this child: -W error)
        out["beta_" + name] = beta_t.cpu().numpy(); out["rhs_" + name] = rhs_t.cpu().numpy(); out["it_" + name] = it_t.cpu().numpy()
    np.savez(sys.argv[1], F=F, sample=sample, mu=mu, Lam=Lam, **out)
''') % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)))


def _run_child(N, numF, D, resident):
    with tempfile.TemporaryDirectory() as td:
        f = os.path.join(td, "o.npz")
        env = dict(os.environ)
        env.pop("BDF_CG_RESIDENT", None)
        if resident is not None:
            env["BDF_CG_RESIDENT"] = resident
        subprocess.run([sys.executable, "-W", "error::RuntimeWarning", "-c", _CHILD, f, str(N), str(numF), str(D)], check=True, env=env, timeout=300)
        return dict(np.load(f))


def _against_oracle_and_direct(O, a, numF, D):
    assert I.cond_AtA(a["F"], I.RESIDENT_LB) < 1e4
    beta_o, rhs_o, it_o = O.sample_beta(O.Feat.from_dense(a["F"]), a["sample"], a["mu"], a["Lam"], I.RESIDENT_LB, False, None, 77, 4, 3)
    beta, rhs = a["beta_tight"].reshape(D, numF).T, a["rhs_tight"].reshape(D, numF).T
    scale = np.abs(beta_o).max()
    np.testing.assert_allclose(rhs, rhs_o, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(beta, beta_o, rtol=1e-7, atol=1e-9 * scale)
    np.testing.assert_allclose(beta, I.direct_solve(a["F"], I.RESIDENT_LB, rhs_o), rtol=1e-6, atol=1e-7 * scale)
    assert np.all(np.abs(a["it_tight"] - it_o) <= 2), (a["it_tight"], it_o)
    assert a["it_tight"].min() >= 4
    return np.abs(beta - beta_o).max() / scale


@pytest.mark.parametrize("N,numF,D", I.RESIDENT_CASES)
def test_cg_one_launch_limits(O, N, numF, D):
    """k_cg_resident at the limits of its domain -- 128 features with D = ceil(128 / 16) = 8 columns (k_cg_resident<1>, eight
    workgroups, every one a column owner), 129 (nine workgroups, the last with one row of the operator) and 512 features with 32
    columns (k_cg_resident<2>, 32 workgroups) -- after the pattern of test_cg_one_launch_solve_matches_the_two_launch_solve_and_the_oracle:
    the same iteration counts, the same rhs bit for bit and beta to 1e-9 as the two-launch solve (BDF_CG_RESIDENT=0, read once per
    process: a child each), fewer iterations at the loose tolerance, and the oracle and the direct solve on the same streams"""
    a, b = _run_child(N, numF, D, "1"), _run_child(N, numF, D, "0")
    for name in ("tight", "loose"):
        assert np.array_equal(a["it_" + name], b["it_" + name]), (name, a["it_" + name], b["it_" + name])
        np.testing.assert_array_equal(a["rhs_" + name], b["rhs_" + name])
        np.testing.assert_allclose(a["beta_" + name], b["beta_" + name], rtol=1e-9, atol=1e-11)
    assert a["it_loose"].max() < a["it_tight"].max()
    err = _against_oracle_and_direct(O, a, numF, D)
    print(f"feature edges: one-launch solve numF = {numF}, D = {D}: iterations {a['it_tight'].min()}..{a['it_tight'].max()}, beta against the oracle {err:.2e}")


def test_cg_one_launch_refused(O):
    """128 features and NINE columns: more columns than the ceil(128 / 16) = 8 workgroups that would own them, so feat_cg_solve must
    not take the one-launch path (the ninth column would have no owner) -- k_cg_step_short<2> on the F'F operator; one child with
    the switch unset, against the oracle and the direct solve"""
    N, numF, D = I.RESIDENT_REFUSED
    err = _against_oracle_and_direct(O, _run_child(N, numF, D, None), numF, D)
    print(f"feature edges: 128 features, 9 columns: beta against the oracle {err:.2e}")
