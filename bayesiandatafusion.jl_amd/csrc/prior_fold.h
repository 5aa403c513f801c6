// prior_fold.h -- what the two kernels share that fold a relation's unlisted cells into the prior the row kernels take (k_bg_fold of
// k_background.hip; k_dmat_fold of k_dense.hip, section 25): the term record and the head of their launch
// arguments with its host-side fill, the first half of both kernels up to the factorisation of Lambda_eff, the refined solve, and the
// fixed-order sum of a four-wave workgroup that their all-cells sums close with.  The refinement step, the identity on the padding and
// the order of every sum are why these kernels give the same bits on a rerun: they are stated here once.  File-local in every unit
// that includes it.
#pragma once
#include "bdf_common.h"
#include "background.h"
#include "wave_linalg.h"
#include <cmath>

namespace {

// ---- the launch arguments' head -----------------------------------------------------------------------------------------------
// The term is bdf_dense_term's field set; a background term is one with C == NULL.
struct FoldHead {
    int D, n;
    bdf_dense_term t[BDF_MAX_TERMS];
    const double *mu;          // nullable: per-row prior means
    const double *Lambda;
    double *Lambda_out, *alpha_rows_out;
    int *flag;
};

inline bdf_dense_term fold_term(const bdf_dense_term &t) { return t; }
inline bdf_dense_term fold_term(const bdf_background_term &t)
{
    bdf_dense_term d = {};
    d.gram = t.gram; d.sum = t.sum; d.alpha = t.alpha; d.alpha_dev = t.alpha_dev; d.weight = t.weight; d.resid = t.resid;
    return d;
}

// the shared checks and fields of bdf_background_prior and bdf_dense_prior, under the caller's name
template <class Term>
int fold_fill(const char *who, bdf_ctx *ctx, int D, int64_t N, int n, const Term *terms, const double *mu, int mu_is_matrix, const double *Lambda,
              double *Lambda_out, double *mu_out, double *alpha_rows_out, FoldHead &h)
{
    BDF_REQUIRE(ctx && terms && mu && Lambda && Lambda_out && mu_out && alpha_rows_out, BDF_ERR_ARG, "%s: NULL argument", who);
    BDF_REQUIRE(D >= 1 && D <= BDF_MAX_D, BDF_ERR_ARG, "%s: num_latent=%d must be in 1..%d", who, D, BDF_MAX_D);
    BDF_REQUIRE(n >= 1 && n <= BDF_MAX_TERMS, BDF_ERR_ARG, "%s: %d terms (1..%d)", who, n, BDF_MAX_TERMS);
    BDF_REQUIRE(N >= 0, BDF_ERR_ARG, "%s: N < 0", who);
    BDF_REQUIRE(Lambda_out != Lambda && mu_out != mu, BDF_ERR_ARG, "%s: the outputs may not alias mu and Lambda", who);
    h = {};
    h.D = D; h.n = n;
    for (int k = 0; k < n; k++) {
        const bdf_dense_term t = fold_term(terms[k]);
        BDF_REQUIRE(t.gram && (t.C != nullptr) != (t.sum != nullptr), BDF_ERR_ARG,
                    "%s: term %d needs a Gram matrix and either sum (a background term) or C (a dense term)", who, k);
        BDF_REQUIRE(t.weight > 0.0 && t.weight <= 1.0 && std::isfinite(t.resid) && (t.sum || t.weight == 1.0), BDF_ERR_ARG,
                    "%s: term %d: weight=%g must lie in (0, 1] (1 for a dense term) and resid=%g be finite", who, k, t.weight, t.resid);
        BDF_REQUIRE(t.alpha_dev || (t.alpha > 0.0 && std::isfinite(t.alpha)), BDF_ERR_ARG, "%s: term %d: alpha=%g must be positive and finite", who, k, t.alpha);
        h.t[k] = t;
    }
    h.mu = mu_is_matrix ? nullptr : mu;
    h.Lambda = Lambda; h.Lambda_out = Lambda_out; h.alpha_rows_out = alpha_rows_out;
    h.flag = ctx->flag_dev;
    BDF_HIP(hipSetDevice(ctx->device));
    return BDF_OK;
}

// ---- the first half of both kernels ---------------------------------------------------------------------------------------------
// One wave, lane = column c = lane % DP (the 64 / DP groups of a wave hold the same column).  ac[k] = alpha_k weight_k; column c of
// Lambda_eff = Lambda + sum_k ac[k] G_k, the terms added in their order, in col[] and in sA (sA[i + c * DP] = element (i, c);
// identity on the padding); t_c = the background terms' part of the right-hand side, sum_k ac[k] rb_k s_k[c]; then the
// factorisation as wave_linalg.h leaves it (col, p_own, rp_own, tri), a Lambda_eff that is not positive definite raising the flag.
// `writes`: this workgroup stores Lambda_out and alpha_rows_out -- alpha_k (1 - c0_k) of a background term, whose listed cells then
// count beside the Gram term, alpha_k of a dense term, which lists none.
template <int DP>
__device__ __forceinline__ void fold_head(const FoldHead &a, bool writes, double (&ac)[BDF_MAX_TERMS], double (&col)[DP], double &t_c, double &p_own,
                                          double &rp_own, double *tri, double *sA, int lane)
{
    const int c = lane % DP, grp = lane / DP;
    const int D = a.D;
    const bool in = c < D;
#pragma unroll
    for (int k = 0; k < BDF_MAX_TERMS; k++) {
        ac[k] = 0.0;
        if (k < a.n) {
            const double alpha = a.t[k].alpha_dev ? *a.t[k].alpha_dev : a.t[k].alpha;
            ac[k] = alpha * a.t[k].weight;
            if (lane == k && writes) a.alpha_rows_out[k] = a.t[k].C ? alpha : bdf_bg_alpha_rows(alpha, a.t[k].weight);
        }
    }
#pragma unroll
    for (int i = 0; i < DP; i++) {
        double v = (i == c) ? 1.0 : 0.0;
        if (i < D && in) {
            v = a.Lambda[i + (int64_t)c * D];
#pragma unroll
            for (int k = 0; k < BDF_MAX_TERMS; k++)
                if (k < a.n) v = v + ac[k] * a.t[k].gram[i + (int64_t)c * D];
            if (grp == 0 && writes) a.Lambda_out[i + (int64_t)c * D] = v;
        }
        col[i] = v;
        if (grp == 0) sA[i + c * DP] = v;
    }
    t_c = 0.0;
#pragma unroll
    for (int k = 0; k < BDF_MAX_TERMS; k++)
        if (k < a.n && a.t[k].sum && in) t_c = t_c + (ac[k] * a.t[k].resid) * a.t[k].sum[c];
    wave_sync();
    if (wl_factor<DP, true>(col, p_own, rp_own, tri, lane) && lane == 0) atomicOr_system(a.flag, 1);
}

// x = A^-1 b for the factored A (lane c of a group holds b_c and gets x_c; the groups of a wave solve side by side), refined once:
// r = b - A x with A from LDS (sA[c + k * DP] = A[k][c] = A[c][k]), x += A^-1 r.  The pivots' reciprocals are good to 1.5e-15
// (fast_rcp), and what the rows read is A x, the solve's right-hand side again -- its residual, not its forward error, reaches them.
template <int DP>
__device__ __forceinline__ double fold_solve(const double (&fac)[DP], const double *tri, const double *sA, double rp_own, double b, int lane)
{
    const int c = lane % DP, base = (lane / DP) * DP;
    const double x = wl_backward<DP, true>(tri, wl_forward<DP>(fac, b, rp_own, lane), rp_own, lane);
    double r = b;
#pragma unroll
    for (int k = 0; k < DP; k++) r = fma(-sA[c + k * DP], __shfl(x, base + k), r);
    return x + wl_backward<DP, true>(tri, wl_forward<DP>(fac, r, rp_own, lane), rp_own, lane);
}

// ---- a four-wave workgroup's sum of one value per thread, in a fixed order; valid in thread 0 -------------------------------------
// (the waves pairwise: block_sum of k_feat_cg.hip and block_sum_fixed of k_auc.hip add them left to right, which gives other bits)
__device__ __forceinline__ double block_sum4(double v, double *red)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();                                   // (red may still be read from the previous sum)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

}  // namespace
