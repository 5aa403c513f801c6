// k_dense.hip -- a dense two-mode relation (setDense): all N x M cells are observed and kept on the device
// as R (row-major doubles, the values without their mean).  Every row's conditional then reads the relation through the Gram
// matrix of the other entity's rows, which all rows share, and its own row of C = R V:
//
//   bdf_dense_product   k_dmat_product: C = R F (N x D) or C = R' F (M x D) on v_mfma_f64_16x16x4_f64, both from the one copy of
//                       R.  A workgroup owns 16 rows of the result; its 8 waves share the contraction out in 16-index pieces
//                       (wave w takes pieces w, w + 8, ...) and add their tiles through LDS in a fixed order.
//   bdf_dense_prior     k_dmat_fold: one wave per 64 / DP columns of the inverse.  Lambda_eff = Lambda + sum_k alpha_k c_k G_k in the order of the terms (c_k = 1 for a
//                       dense term, c0 for a background term of section 20), factored and solved as k_bg_fold does, each solve
//                       refined once: Lambda_eff^-1, Lambda_eff^-1 Lambda for per-row prior means, and w0.  Then k_dmat_mu_rows:
//                       mu_eff_i = Lambda_eff^-1 Lambda mu_i + Lambda_eff^-1 (sum_k alpha_k C_k,i) + w0 over the N rows on the matrix
//                       cores, rows past N and D off the tile by predication.
//   bdf_dense_impute    k_dmat_impute: a cell that is not listed (a hole) is a latent value of the augmented model, drawn before every
//                       iteration: r_ij = u_i.v_j + z / sqrt(alpha), the lane prologue and gather of pair_gather.h over the holes as
//                       pairs, one normal of the hole's own stream, one plain store into R, the sum of r^2 through block_stats.
//   bdf_dense_sse       sum over all cells of (r - u.v)^2 = sum r^2 - 2 sum_i u_i.C_i + <U'U, V'V>: the workgroups' sums of u_i.C_i,
//                       then one workgroup adds them, the Gram inner product and the closed form in a fixed order.
//
// What k_dmat_fold shares with k_bg_fold -- the term record and its checks, Lambda_eff and its factorisation, the refined solve, the
// closing kernels' four-wave sum -- is written once in prior_fold.h.
// Plain vector stores, no floating-point atomics; no scratch memory except k_dmat_fold<64>'s, which wl_factor<64> brings to every
// kernel that takes it.  Every sum has a fixed order: a rerun gives the same bits.
#include "bdf_common.h"
#include "dense.h"
#include "pair_gather.h"
#include "predict.h"
#include "prior_fold.h"
#include "rows.h"
#include "wave_linalg.h"

namespace {

typedef double dd4 __attribute__((ext_vector_type(4)));

constexpr int PW = 8;          // waves of a product workgroup

// ---- the products -------------------------------------------------------------------------------------------------------------
// out (T x D) = sum_c R(t, c) F[c][:], c < K; R(t, c) = R[t M + c], or R[c M + t] (TRANS).  Lane (ti = lane & 15, kk = lane >> 4)
// holds contraction index c0 + 4 kk + s in k-step s, for both operands: without TRANS its four A values are 32 consecutive bytes
// of row t (the 4 lanes of a row read 128), with TRANS the 16 lanes of a k-row read 128 consecutive bytes of row c.
template <int DB, bool TRANS>
__global__ __launch_bounds__(64 * PW) void k_dmat_product(const double *__restrict__ R, const double *__restrict__ F, double *__restrict__ out,
                                                           int64_t T, int64_t K, int64_t M, int D, int vec)
{
    __shared__ double red[PW - 1][DB * 4 * 64];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ti = lane & 15, kk = lane >> 4;
    const int64_t t0 = (int64_t)blockIdx.x * 16, t = t0 + ti;
    const bool tile_full = t0 + 16 <= T && D == 16 * DB;
    dd4 acc[DB];
#pragma unroll
    for (int blk = 0; blk < DB; blk++) acc[blk] = dd4{0.0, 0.0, 0.0, 0.0};

    auto load = [&](int64_t c0, double (&a)[4], double (&b)[DB][4]) {
        const int64_t c = c0 + 4 * kk;
        if (tile_full && c0 + 16 <= K) {               // (uniform over the wave) nothing to predicate
            if (!TRANS && vec) {
                const dd4 v = *(const dd4 *)(R + t * M + c);
                a[0] = v[0]; a[1] = v[1]; a[2] = v[2]; a[3] = v[3];
            } else {
#pragma unroll
                for (int s = 0; s < 4; s++) a[s] = TRANS ? R[(c + s) * M + t] : R[t * M + c + s];
            }
#pragma unroll
            for (int s = 0; s < 4; s++)
#pragma unroll
                for (int blk = 0; blk < DB; blk++) b[blk][s] = F[(c + s) * D + 16 * blk + ti];
            return;
        }
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const bool ok = c + s < K;
            a[s] = (ok && t < T) ? (TRANS ? R[(c + s) * M + t] : R[t * M + c + s]) : 0.0;
#pragma unroll
            for (int blk = 0; blk < DB; blk++) b[blk][s] = (ok && 16 * blk + ti < D) ? F[(c + s) * D + 16 * blk + ti] : 0.0;
        }
    };

    double a[4], b[DB][4];
    int64_t c0 = 16 * wave;
    if (c0 < K) load(c0, a, b);
    for (; c0 < K; c0 += 16 * PW) {
        double an[4], bn[DB][4];
        const bool more = c0 + 16 * PW < K;            // the next piece's loads, under this piece's matrix instructions
        if (more) load(c0 + 16 * PW, an, bn);
#pragma unroll
        for (int s = 0; s < 4; s++)
#pragma unroll
            for (int blk = 0; blk < DB; blk++) acc[blk] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], b[blk][s], acc[blk], 0, 0, 0);
        if (more) {
#pragma unroll
            for (int s = 0; s < 4; s++) {
                a[s] = an[s];
#pragma unroll
                for (int blk = 0; blk < DB; blk++) b[blk][s] = bn[blk][s];
            }
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int blk = 0; blk < DB; blk++)
#pragma unroll
            for (int r = 0; r < 4; r++) red[wave - 1][(blk * 4 + r) * 64 + lane] = acc[blk][r];
    }
    __syncthreads();
    if (wave != 0) return;
    // C layout: lane (column ti, h = kk), register r: tile row h + 4 r
#pragma unroll
    for (int blk = 0; blk < DB; blk++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int e = (blk * 4 + r) * 64 + lane;
            const double v = ((acc[blk][r] + red[0][e]) + (red[1][e] + red[2][e])) + ((red[3][e] + red[4][e]) + (red[5][e] + red[6][e]));
            const int64_t row = t0 + kk + 4 * r;
            const int col = 16 * blk + ti;
            if (row < T && col < D) out[row * D + col] = v;
        }
}

// ---- the prior of a dense entity ----------------------------------------------------------------------------------------------------
// the fold's own outputs behind the shared head (prior_fold.h)
struct DenseFoldArgs : FoldHead {       // mu NULL: per-row prior means -- Wt_out is written too
    double *coef_out;          // alpha_k weight_k of the terms, for k_dmat_mu_rows
    double *Ti_out, *Wt_out;   // [e * DP + d] = (Lambda_eff^-1)[d][e], (Lambda_eff^-1 Lambda)[d][e]: DP x DP row-major, zero outside D x D
    double *w0_out;            // DP, zero behind D: Lambda_eff^-1 (Lambda mu + t), or Lambda_eff^-1 t for per-row prior means
};

// fold_head (prior_fold.h) builds and factors Lambda_eff in every workgroup; what follows is the dense fold's own: the columns of the
// inverse over the workgroups
template <int DP>
__global__ __launch_bounds__(64) void k_dmat_fold(DenseFoldArgs a)
{
    using W = WL<DP>;
    constexpr int G = W::G;
    __shared__ double tri[W::TRI + 64];
    __shared__ double sA[DP * DP];          // Lambda_eff: sA[i + c * DP] = element (i, c); identity on the padding
    const int lane = threadIdx.x, c = lane % DP, grp = lane / DP;
    const int D = a.D;
    const bool in = c < D;
    const bool last = blockIdx.x == gridDim.x - 1;
    double ac[BDF_MAX_TERMS], col[DP], t_c, p_own, rp_own;
    fold_head<DP>(a, last, ac, col, t_c, p_own, rp_own, tri, sA, lane);
#pragma unroll
    for (int k = 0; k < BDF_MAX_TERMS; k++)
        if (last && lane == k && k < a.n) a.coef_out[k] = ac[k];

    // Lambda_eff^-1 and, for per-row prior means, Lambda_eff^-1 Lambda by columns, G of them side by side in this workgroup: every
    // workgroup factors for itself (one wave's latency, not D / G of them in a row); the last one takes w0, the padding and Lambda_out
    if (blockIdx.x + 1 < gridDim.x) {
        const int q = (int)blockIdx.x * G + grp;
        const double x = fold_solve<DP>(col, tri, sA, rp_own, (q < D && c == q) ? 1.0 : 0.0, lane);
        if (q < D) a.Ti_out[q * DP + c] = in ? x : 0.0;
        if (a.mu == nullptr) {
            const double xw = fold_solve<DP>(col, tri, sA, rp_own, (q < D && in) ? a.Lambda[c + (int64_t)q * D] : 0.0, lane);
            if (q < D) a.Wt_out[q * DP + c] = in ? xw : 0.0;
        }
        return;
    }
    for (int q = D + grp; q < DP; q += G) {
        a.Ti_out[q * DP + c] = 0.0;
        if (a.mu == nullptr) a.Wt_out[q * DP + c] = 0.0;
    }
    double b = t_c;
    if (a.mu != nullptr && in)
        for (int i = 0; i < D; i++) b = fma(a.Lambda[c + (int64_t)i * D], a.mu[i], b);
    const double x0 = fold_solve<DP>(col, tri, sA, rp_own, b, lane);
    if (grp == 0) a.w0_out[c] = in ? x0 : 0.0;
}

struct DenseRowsArgs {
    int D, n;
    const double *C[BDF_MAX_TERMS];        // NULL: not a dense term
    const double *coef;                    // alpha_k of the fold
    const double *X;                       // nullable: the per-row prior means
    const double *Ti, *Wt, *w0;
    double *Y;
    int64_t N;
};

// Y_i = Ti' S_i + Wt' X_i + w0 for the N rows of D doubles, S_i = sum_k alpha_k C_k,i in the order of the terms.  One wave per
// 16 rows; the contraction runs over e = kk DP / 4 + q (lane row kk, k-step q), so a lane's operand values are DP / 4 consecutive
// doubles of its row, read from global memory directly.
template <int DP>
__global__ __launch_bounds__(256) void k_dmat_mu_rows(DenseRowsArgs a)
{
    constexpr int DB = DP / 16, KQ = DP / 4;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = lane & 15, kk = lane >> 4;
    const int64_t r0 = ((int64_t)blockIdx.x * 4 + wave) * 16, row = r0 + i;
    const int D = a.D;
    if (r0 >= a.N) return;
    double coef[BDF_MAX_TERMS];
#pragma unroll
    for (int k = 0; k < BDF_MAX_TERMS; k++) coef[k] = (k < a.n && a.C[k]) ? a.coef[k] : 0.0;
    double s[KQ], x[KQ];
#pragma unroll
    for (int q = 0; q < KQ; q++) {
        const int e = kk * KQ + q;
        const bool ok = row < a.N && e < D;
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < BDF_MAX_TERMS; k++)
            if (k < a.n && a.C[k] && ok) v = fma(coef[k], a.C[k][row * D + e], v);
        s[q] = v;
        x[q] = (ok && a.X) ? a.X[row * D + e] : 0.0;
    }
#pragma unroll
    for (int cb = 0; cb < DB; cb++) {
        const int col = 16 * cb + i;
        dd4 acc = dd4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int q = 0; q < KQ; q++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(s[q], a.Ti[(kk * KQ + q) * DP + col], acc, 0, 0, 0);
        if (a.X) {
#pragma unroll
            for (int q = 0; q < KQ; q++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(x[q], a.Wt[(kk * KQ + q) * DP + col], acc, 0, 0, 0);
        }
        const double bias = a.w0[col];
        // C layout: lane (j = i, h = kk), register r: tile row h + 4 r, column 16 cb + j
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int64_t rowm = r0 + kk + 4 * r;
            if (rowm < a.N && col < D) a.Y[rowm * D + col] = acc[r] + bias;
        }
    }
}

// ---- the holes ------------------------------------------------------------------------------------------------------------------------
struct ImputeArgs {
    PairArgs pair;                 // the holes as pairs (two modes)
    uint64_t seed;
    uint32_t sweep, entity;        // pair_entity(rel_tag)
    double *R;
    int64_t N, M;
    double *partial;               // per-block statistics: [0] the sum of r^2 over the workgroup's holes
};

// one group of 8 lanes per 8 holes, no grid-stride loop (every lane reaches the sum's barrier): k_bg_sse's shape
template <int VEC, int NC>
__global__ __launch_bounds__(256, 3) void k_dmat_impute(ImputeArgs a)
{
    const double alpha = pair_alpha(a.pair);
    const int64_t trip = pair_trip();
    double st[4] = {0.0, 0.0, 0.0, 0.0};
    if (trip * 8 < a.pair.n) {
        PairLane<2> l;
        pair_lane(a.pair, trip, l);
        const double psi = pair_dot<2, VEC, NC>(a.pair, l);
        const int64_t i = l.my[0], j = l.my[1];
        if (l.ok && i >= 0 && i < a.N && j >= 0 && j < a.M) {
            // the hole's own normal: the stream is keyed by the caller's index, not by where the pair is stored
            const double z = bdf_normal(a.seed, a.sweep, BDF_P_DENSE, a.entity, (uint64_t)l.po, 0);
            const double r = bdf_dense_hole(psi, z, alpha);
            a.R[i * a.M + j] = r;
            st[0] = r * r;
        }
    }
    block_stats(a.partial, st);
}

// ---- the sum of e^2 over all N M cells ----------------------------------------------------------------------------------------------
constexpr int DOT_SLAB = 4096;             // elements of U and C per workgroup of k_dmat_dot

__global__ __launch_bounds__(256) void k_dmat_dot(const double *__restrict__ U, const double *__restrict__ C, int64_t n, double *partial)
{
    __shared__ double red[4];
    const int64_t base = (int64_t)blockIdx.x * DOT_SLAB;
    double s = 0.0;
#pragma unroll 4
    for (int j = 0; j < DOT_SLAB / 256; j++) {
        const int64_t e = base + j * 256 + threadIdx.x;
        if (e < n) s = fma(U[e], C[e], s);
    }
    s = block_sum4(s, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void k_dmat_sse_final(int nblocks, const double *partial, int D, const double *gramU, const double *gramV,
                                                         double sum_r2, const double *holes_r2, double *out)
{
    __shared__ double red[4];
    const int tid = threadIdx.x;
    double s = 0.0, g = 0.0;
    for (int b = tid; b < nblocks; b += 256) s += partial[b];
    for (int e = tid; e < D * D; e += 256) g = fma(gramU[e], gramV[e], g);
    s = block_sum4(s, red);
    g = block_sum4(g, red);
    if (tid == 0) *out = bdf_dense_all_cells(holes_r2 ? sum_r2 + *holes_r2 : sum_r2, s, g);
}

template <bool TRANS>
void launch_product(int DP, dim3 grid, hipStream_t st, const double *R, const double *F, double *out, int64_t T, int64_t K, int64_t M, int D, int vec)
{
    if (DP == 16) hipLaunchKernelGGL((k_dmat_product<1, TRANS>), grid, dim3(64 * PW), 0, st, R, F, out, T, K, M, D, vec);
    else if (DP == 32) hipLaunchKernelGGL((k_dmat_product<2, TRANS>), grid, dim3(64 * PW), 0, st, R, F, out, T, K, M, D, vec);
    else hipLaunchKernelGGL((k_dmat_product<4, TRANS>), grid, dim3(64 * PW), 0, st, R, F, out, T, K, M, D, vec);
}

}  // namespace

extern "C" int bdf_dense_product(bdf_ctx *ctx, const double *R, int64_t N, int64_t M, int D, const double *F, int transpose, double *out)
{
    BDF_REQUIRE(ctx && R && F && out, BDF_ERR_ARG, "bdf_dense_product: NULL argument");
    BDF_REQUIRE(D >= 1 && D <= BDF_MAX_D, BDF_ERR_ARG, "bdf_dense_product: num_latent=%d must be in 1..%d", D, BDF_MAX_D);
    BDF_REQUIRE(N >= 1 && M >= 1, BDF_ERR_ARG, "bdf_dense_product: N=%lld and M=%lld must be at least 1", (long long)N, (long long)M);
    const int64_t T = transpose ? M : N, K = transpose ? N : M;
    const int64_t tiles = (T + 15) / 16;
    BDF_REQUIRE(tiles <= 0x7fffffff, BDF_ERR_ARG, "bdf_dense_product: %lld rows of the result are more than one launch takes", (long long)T);
    BDF_HIP(hipSetDevice(ctx->device));
    const int vec = (M % 4 == 0) && (((uintptr_t)R) % 32 == 0);
    const dim3 grid((unsigned)tiles);
    if (transpose) launch_product<true>(bdf_rows_dp(D), grid, ctx->stream, R, F, out, T, K, M, D, vec);
    else launch_product<false>(bdf_rows_dp(D), grid, ctx->stream, R, F, out, T, K, M, D, vec);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}

extern "C" int bdf_dense_prior(bdf_ctx *ctx, int D, int64_t N, int n_terms, const bdf_dense_term *terms, const double *mu, int mu_is_matrix,
                               const double *Lambda, double *Lambda_out, double *mu_out, double *alpha_rows_out)
{
    DenseFoldArgs a = {};
    DenseRowsArgs ra = {};
    int rc = fold_fill("bdf_dense_prior", ctx, D, N, n_terms, terms, mu, mu_is_matrix, Lambda, Lambda_out, mu_out, alpha_rows_out, a);
    if (rc) return rc;
    ra.D = D; ra.n = n_terms;
    int n_dense = 0;
    for (int k = 0; k < n_terms; k++) {
        ra.C[k] = terms[k].C;
        n_dense += terms[k].C != nullptr;
    }
    BDF_REQUIRE(n_dense >= 1, BDF_ERR_ARG, "bdf_dense_prior: no dense term (bdf_background_prior folds background terms alone)");
    const int DP = bdf_rows_dp(D);
    void *sc;
    if ((rc = bdf_scratch(ctx, ((size_t)2 * DP * DP + DP + BDF_MAX_TERMS) * sizeof(double), &sc))) return rc;
    a.Ti_out = (double *)sc; a.Wt_out = a.Ti_out + (size_t)DP * DP; a.w0_out = a.Wt_out + (size_t)DP * DP; a.coef_out = a.w0_out + DP;
    const int G = 64 / DP, nfold = (D + G - 1) / G + 1;
    if (DP == 16) hipLaunchKernelGGL(k_dmat_fold<16>, dim3(nfold), dim3(64), 0, ctx->stream, a);
    else if (DP == 32) hipLaunchKernelGGL(k_dmat_fold<32>, dim3(nfold), dim3(64), 0, ctx->stream, a);
    else hipLaunchKernelGGL(k_dmat_fold<64>, dim3(nfold), dim3(64), 0, ctx->stream, a);
    if (N > 0) {
        ra.coef = a.coef_out; ra.X = mu_is_matrix ? mu : nullptr; ra.Ti = a.Ti_out; ra.Wt = a.Wt_out; ra.w0 = a.w0_out; ra.Y = mu_out; ra.N = N;
        const int64_t blocks = (N + 63) / 64;
        BDF_REQUIRE(blocks <= 0x7fffffff, BDF_ERR_ARG, "bdf_dense_prior: %lld rows are more than one launch takes", (long long)N);
        const dim3 grid((unsigned)blocks);
        if (DP == 16) hipLaunchKernelGGL(k_dmat_mu_rows<16>, grid, dim3(256), 0, ctx->stream, ra);
        else if (DP == 32) hipLaunchKernelGGL(k_dmat_mu_rows<32>, grid, dim3(256), 0, ctx->stream, ra);
        else hipLaunchKernelGGL(k_dmat_mu_rows<64>, grid, dim3(256), 0, ctx->stream, ra);
    }
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}

extern "C" int bdf_dense_sse(bdf_ctx *ctx, int D, int64_t N, const double *U, const double *C, const double *gramU, const double *gramV,
                             double sum_r2, const double *holes_r2, double *out)
{
    BDF_REQUIRE(ctx && U && C && gramU && gramV && out, BDF_ERR_ARG, "bdf_dense_sse: NULL argument");
    BDF_REQUIRE(D >= 1 && D <= BDF_MAX_D, BDF_ERR_ARG, "bdf_dense_sse: num_latent=%d must be in 1..%d", D, BDF_MAX_D);
    BDF_REQUIRE(N >= 1 && std::isfinite(sum_r2) && sum_r2 >= 0.0, BDF_ERR_ARG, "bdf_dense_sse: N=%lld must be at least 1 and sum_r2=%g finite and not negative", (long long)N, sum_r2);
    const int64_t n = N * (int64_t)D, nblocks = (n + DOT_SLAB - 1) / DOT_SLAB;
    BDF_REQUIRE(nblocks <= 0x7fffffff, BDF_ERR_ARG, "bdf_dense_sse: %lld rows are more than one launch takes", (long long)N);
    BDF_HIP(hipSetDevice(ctx->device));
    void *sc;
    int rc = bdf_scratch(ctx, (size_t)nblocks * sizeof(double), &sc);
    if (rc) return rc;
    hipLaunchKernelGGL(k_dmat_dot, dim3((unsigned)nblocks), dim3(256), 0, ctx->stream, U, C, n, (double *)sc);
    hipLaunchKernelGGL(k_dmat_sse_final, dim3(1), dim3(256), 0, ctx->stream, (int)nblocks, (const double *)sc, D, gramU, gramV, sum_r2, holes_r2, out);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}

extern "C" int bdf_dense_impute(bdf_ctx *ctx, const bdf_pairs *holes, int D, const double *const *factors, double alpha, const double *alpha_dev,
                                uint32_t rel_tag, double *R, int64_t N, int64_t M, double *stats_out)
{
    BDF_REQUIRE(R && stats_out, BDF_ERR_ARG, "bdf_dense_impute: NULL argument");
    BDF_REQUIRE(N >= 1 && M >= 1, BDF_ERR_ARG, "bdf_dense_impute: N=%lld and M=%lld must be at least 1", (long long)N, (long long)M);
    ImputeArgs a = {};
    int rc = pair_fill("bdf_dense_impute", ctx, holes, D, factors, 0.0, true, alpha, alpha_dev, a.pair);
    if (rc) return rc;
    BDF_REQUIRE(holes->n_modes == 2, BDF_ERR_ARG, "bdf_dense_impute: a dense relation has two modes, the holes have %d", holes->n_modes);
    a.seed = ctx->seed; a.sweep = ctx->sweep_host; a.entity = pair_entity(rel_tag);
    a.R = R; a.N = N; a.M = M;
    BDF_HIP(hipSetDevice(ctx->device));
    if (holes->n == 0) {
        BDF_HIP(hipMemsetAsync(stats_out, 0, 4 * sizeof(double), ctx->stream));
        return BDF_OK;
    }
    int nblocks;
    if ((rc = pair_blocks("bdf_dense_impute", "holes", holes->n, &nblocks))) return rc;
    return launch_reduced(ctx, nblocks, a.partial, stats_out, [&] {
        if (D & 3) hipLaunchKernelGGL((k_dmat_impute<1, 1>), dim3(nblocks), dim3(256), 0, ctx->stream, a);
        else if (D <= 32) hipLaunchKernelGGL((k_dmat_impute<4, 1>), dim3(nblocks), dim3(256), 0, ctx->stream, a);
        else hipLaunchKernelGGL((k_dmat_impute<4, 2>), dim3(nblocks), dim3(256), 0, ctx->stream, a);
    });
}
