// feat.h -- what the units of the side-information path take from each other: the operators (k_feat_ops.hip), the batched
// conjugate-gradient solve (k_feat_cg.hip) and the eigen-decomposition solve (k_feat_eig.hip), as the beta update
// (k_feat_beta.hip) and each other call them.  Library-internal: nothing here is exported through include/bdf.h.
#pragma once
#include "bdf_common.h"

// ---- k_feat_ops.hip ------------------------------------------------------------------------------------------------
// strided dense GEMM: C(i,j) = sum_k A(i,k) B(k,j), optional second output C2 = C + bias[j]
struct GemmArgs {
    int64_t M, N, K;
    const double *A; int64_t ars, acs;
    const double *B; int64_t brs, bcs;
    double *C; int64_t crs, ccs;
    const double *bias; double *C2;
};
int feat_gemm(bdf_ctx *ctx, const GemmArgs &g);

// the accumulator of a v_mfma_f64_16x16x4_f64 (k_dense_nn, k_dense_tn; k_cg_resident keeps k_dense_nn's operand layout)
typedef double fd4 __attribute__((ext_vector_type(4)));

// Y = A B for a dense column-major M x K matrix A (a feature matrix, or the precomputed F'F), ncol <= 64
int feat_dense_nn(bdf_ctx *ctx, const double *A, int64_t M, int64_t K, const double *B, int64_t brs, int64_t bcs, int ncol,
                  double *Y, int64_t yrs, int64_t ycs, const double *bias, double *Y2);

// Y = op(F) B for any feature kind.  B(i,c) at B[i*brs + c*bcs], Y(r,c) at Y[r*yrs + c*ycs].
int feat_apply(bdf_ctx *ctx, const bdf_feat *f, bool transpose, const double *B, int64_t brs, int64_t bcs, int ncol,
               double *Y, int64_t yrs, int64_t ycs, const double *bias = nullptr, double *Y2 = nullptr);

// the tiled transposes' launches on ctx->stream (launch only: the caller asks hipGetLastError after its own launches)
// out[i*ncol + c] = in[i*irs + c*ics]
void feat_to_rowmajor(bdf_ctx *ctx, int64_t n, int ncol, const double *in, int64_t irs, int64_t ics, double *out, const int *skip);
// out[i*ors + c*ocs] = in[i*ncol + c]  (+ the biased copy out2)
void feat_from_rowmajor(bdf_ctx *ctx, int64_t n, int ncol, const double *in, double *out, int64_t ors, int64_t ocs,
                        const double *bias, double *out2, const int *skip);

// f->FF_dev = F'F (n x n), built on first use
int feat_ensure_FF(bdf_feat *f);

// ---- k_feat_cg.hip -------------------------------------------------------------------------------------------------
// D simultaneous cg_AtA solves of (F'F + lambda I) X = rhs (solve_cg2, parallel_matrix.jl:488-507); with use_ff the operator
// is the precomputed F'F.  R, P, Z: numF x D; Tm: N x D; scal: 3 D doubles; ints: 2 D + 1 ints.
int feat_cg_solve(bdf_ctx *ctx, bdf_feat *f, bool use_ff, int D, const double *lambda_beta_dev, const double *rhs,
                  double *beta_out, double tol, int maxiter, double *R, double *P, double *Z, double *Tm, double *scal,
                  int *ints, int **iters_dev, double *Xrm = nullptr /* numF x D spare (the row-major solve's X), or NULL */);

// ---- k_feat_eig.hip ------------------------------------------------------------------------------------------------
// beta (n x D column-major) = (F'F + lambda I) \ rhs
int feat_eig_solve(bdf_ctx *ctx, bdf_feat *f, int D, const double *lambda_dev, const double *rhs, double *beta_out);
