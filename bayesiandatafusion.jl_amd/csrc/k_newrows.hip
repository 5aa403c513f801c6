// k_newrows.hip -- cells of rows that were not in training, predicted from their features (setNewRows / setNewTest; DESIGN.md
// section 24).  Given one posterior draw (mu, Lambda, beta, V, alpha) the factor of a new row with features f is
// u* ~ N(uhat, Lambda^-1), uhat = mu + beta' f (bdf_uhat on the new rows' features), and it is integrated out of every cell in
// closed form (newrows.h): nothing is drawn.
//
//   bdf_newrows_quad    q_j = v_j' Lambda^-1 v_j = |L^-1 v_j|^2 (Lambda = L L') for every row of V: the variance that the new row's own
//                       factor adds to a cell of column j.  k_newrows_prep: one wave factorises Lambda in LDS, once per call, and
//                       leaves W = L^-1 (lower triangular, zero-padded to DP x DP) in the context's buffer.  k_newrows_quad<DP>: a
//                       workgroup of four waves takes BDF_NEWROWS_TILE rows of V with W in LDS (leading dimension DP + 2: the 32
//                       lanes of a ds_read_b64 group fall on 32 different bank pairs); a wave forms its 16 rows of Z = V W' on
//                       v_mfma_f64_16x16x4_f64 -- only the k-steps under W's diagonal blocks -- and adds the squares of each row in
//                       a fixed order.  Z stays in the accumulators; only q is written.  |W v|^2 is non-negative by construction.
//   bdf_newrows_update  the pair gather of pair_gather.h with the new rows' uhat as the first mode's factor, the link, the fold
//                       into the running state of five doubles per cell (newrows.h) and eight scalars over the cells with a value,
//                       through per-workgroup statistics and a fixed-order sum.
//   bdf_newrows_update_cells  the same update on (m, q) per cell in the pairs' storage order (k_foldin.hip: a new row conditioned on
//                       cells of its own) instead of the gather.  What a draw does to a cell is one text, bdf_newrows_step of
//                       newrows.h; the checks, the state, the draw's constants, the statistics and their final sum are shared here.
//   bdf_newrows_result  (pred, stdev, lpd) per cell in the caller's order.
//
// Plain vector stores, no floating-point atomics, no scratch memory.
#include "bdf_common.h"
#include "newrows.h"
#include "predict.h"
#include "pair_gather.h"
#include "wave_linalg.h"

namespace {

typedef double bd4 __attribute__((ext_vector_type(4)));

// ---- W = L^-1, Lambda = L L' -----------------------------------------------------------------------------------------------------
// One wavefront; the matrix lives in LDS (the factorisation of k_lr_prep: lane c owns row c of the trailing triangle).  W goes out
// row-major with leading dimension DP: W[r * DP + k] = L^-1[r][k] for k <= r < D, zero elsewhere.  Only Lambda's lower triangle is
// read.  A pivot that is not positive raises bit 1 of the context's flag (BDF_ERR_NOTPD at the next sync); W then holds NaNs.
__global__ __launch_bounds__(64) void k_newrows_prep(int D, int DP, const double *__restrict__ Lambda, double *__restrict__ W, int *flag)
{
    constexpr int LDL = BDF_MAX_D + 1;
    // sA[i * LDL + c]: the Schur complement's lower triangle, then L in place; L^-1 goes TRANSPOSED into the strict upper triangle
    // -- X[i][c], i > c, at sA[c * LDL + i] -- and its diagonal, 1 / L[i][i], into sD
    __shared__ double sA[BDF_MAX_D * LDL];
    __shared__ double sD[BDF_MAX_D];
    const int c = threadIdx.x;
    for (int e = c; e < D * D; e += 64) {
        const int i = e / D, cc = e - i * D;
        sA[i * LDL + cc] = Lambda[e];
    }
    wave_sync();
    // No square root and no division on the steps' path: 1 / L[k][k] = rsqrt(pivot) (fast_rsqrt, two Newton steps: 1e-16) goes to sD,
    // L[c][k] = A[c][k] rsqrt(pivot), and the diagonal of sA is never rewritten (nothing reads L[k][k] itself again) -- two wave
    // barriers per step: the column's writes before the trailing update's reads, the update's writes before the next pivot's read
    bool bad = false;
    for (int k = 0; k < D; k++) {
        const double p = sA[k * LDL + k];
        if (!(p > 0.0)) bad = true;
        const double rs = fast_rsqrt(p);
        const double lck = (c < D && c > k) ? sA[c * LDL + k] * rs : 0.0;        // L[c][k]
        if (c == k) sD[k] = rs;
        else if (c < D && c > k) sA[c * LDL + k] = lck;
        wave_sync();
        // lane c updates ROW c of the trailing lower triangle: A[c][m] -= L[c][k] L[m][k], k < m <= c
        if (c < D && c > k)
            for (int m = k + 1; m <= c; m++) sA[c * LDL + m] = fma(-lck, sA[m * LDL + k], sA[c * LDL + m]);
        wave_sync();
    }
    if (bad && c == 0) atomicOr_system(flag, 1);
    // L^-1 by columns: lane c solves L x = e_c (x_i = 0 above the diagonal); its entries sit in row c of the upper triangle
    if (c < D) {
        const double xd = sD[c];
        for (int i = c + 1; i < D; i++) {
            double s = -sA[i * LDL + c] * xd;
            for (int m = c + 1; m < i; m++) s = fma(-sA[i * LDL + m], sA[c * LDL + m], s);
            sA[c * LDL + i] = s * sD[i];
        }
    }
    wave_sync();
    for (int e = c; e < DP * DP; e += 64) {
        const int r = e / DP, k = e - r * DP;
        double w = 0.0;
        if (r < D && k < r) w = sA[k * LDL + r];
        else if (r < D && k == r) w = sD[r];
        W[e] = w;
    }
}

// ---- q = row sums of squares of V W' ----------------------------------------------------------------------------------------------
// Operands of v_mfma_f64_16x16x4_f64: lane (j = lane & 15, h = lane >> 4) holds A[row j][k = h] = V[row0 + j][4 s + h] and
// B[k = h][column j] = W[16 cb + j][4 s + h]; the accumulator's register r is row h + 4 r, column j.  Column block cb of Z needs
// the k-steps s <= 4 cb + 3 only: W[c][d] = 0 for d > c.  Rows behind M and elements behind D are zero operands.
template <int DP>
__global__ __launch_bounds__(256) void k_newrows_quad(int D, int64_t M, const double *__restrict__ W, const double *__restrict__ V, double *__restrict__ q)
{
    constexpr int CBN = DP / 16, KQ = DP / 4, LDW = DP + 2;
    __shared__ double sW[DP * LDW];
    for (int e = threadIdx.x; e < DP * DP; e += 256) {
        const int r = e / DP, k = e - r * DP;
        sW[r * LDW + k] = W[e];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 15, h = lane >> 4;
    const int64_t row0 = (int64_t)blockIdx.x * BDF_NEWROWS_TILE + 16 * wave;
    if (row0 >= M) return;                                 // (wave-uniform, behind the kernel's only barrier)
    const int64_t row = row0 + j;
    const bool live = row < M;
    const double *vr = V + (live ? row : M - 1) * D;
    bd4 acc[CBN];
#pragma unroll
    for (int cb = 0; cb < CBN; cb++) acc[cb] = bd4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < KQ; s++) {
        if (4 * s < D) {                                   // (uniform)
            const int d = 4 * s + h;
            const double a = (live && d < D) ? vr[d] : 0.0;
#pragma unroll
            for (int cb = s / 4; cb < CBN; cb++) acc[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sW[(16 * cb + j) * LDW + d], acc[cb], 0, 0, 0);
        }
    }
    // a row's squares: the column blocks in ascending order in the lane, then the 16 lanes of the row by halving
#pragma unroll
    for (int r = 0; r < 4; r++) {
        double t = 0.0;
#pragma unroll
        for (int cb = 0; cb < CBN; cb++) t += acc[cb][r] * acc[cb][r];
        t += __shfl_xor(t, 8); t += __shfl_xor(t, 4); t += __shfl_xor(t, 2); t += __shfl_xor(t, 1);
        const int64_t orow = row0 + h + 4 * r;
        if (j == 0 && orow < M) q[orow] = t;
    }
}

// ---- the update -------------------------------------------------------------------------------------------------------------------
struct NewArgs {
    PairArgs pair;                 // fac[0]: uhat of the new rows, fac[1]: V
    const double *q;               // per row of V
    bdf_newrows_draw w;
    bdf_newrows_planes pl;
    double *partial;
};

// bdf_newrows_update_cells: (m, q) per cell in the pairs' storage order instead of the gather
struct NewCellArgs {
    int64_t n;
    const double *values, *m, *q;
    double alpha;
    const double *alpha_dev;
    bdf_newrows_draw w;
    bdf_newrows_planes pl;
    double *partial;
};

// the workgroup's eight sums, in fixed order, to partial[8 * block]; every lane of the workgroup calls it
__device__ inline void block_stats8(double *partial, const double (&st)[BDF_NEWROWS_STATS])
{
    __shared__ double red[BDF_NEWROWS_STATS][256 / 64];
    const int tid = threadIdx.x;
#pragma unroll
    for (int s = 0; s < BDF_NEWROWS_STATS; s++) {
        double v = st[s];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
        if ((tid & 63) == 0) red[s][tid >> 6] = v;
    }
    __syncthreads();
    if (tid < BDF_NEWROWS_STATS) partial[blockIdx.x * BDF_NEWROWS_STATS + tid] = red[tid][0] + red[tid][1] + red[tid][2] + red[tid][3];
}

// fixed-order sum of the per-block statistics: thread t the blocks t, t + 256, ... in rising order, then the 256 sums by halving
__global__ __launch_bounds__(256) void k_newrows_final(int nblocks, const double *__restrict__ partial, double *__restrict__ stats)
{
    __shared__ double red[BDF_NEWROWS_STATS][4];
    const int tid = threadIdx.x;
    double v[BDF_NEWROWS_STATS];
#pragma unroll
    for (int s = 0; s < BDF_NEWROWS_STATS; s++) v[s] = 0.0;
    for (int b = tid; b < nblocks; b += 256)
#pragma unroll
        for (int s = 0; s < BDF_NEWROWS_STATS; s++) v[s] += partial[b * BDF_NEWROWS_STATS + s];
#pragma unroll
    for (int s = 0; s < BDF_NEWROWS_STATS; s++) {
        double x = v[s];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off);
        if ((tid & 63) == 0) red[s][tid >> 6] = x;
    }
    __syncthreads();
    if (tid < BDF_NEWROWS_STATS) stats[tid] = red[tid][0] + red[tid][1] + red[tid][2] + red[tid][3];
}

// One group of 8 lanes per 8 cells and no grid-stride loop, as k_lpd and k_waic.  The state is read only after the gather and the
// link, so that its five doubles are not live across them.  Every lane reaches the statistics' barrier.
template <int VEC, int NC>
__global__ __launch_bounds__(256) void k_newrows_update(NewArgs a)
{
    double st[BDF_NEWROWS_STATS];
#pragma unroll
    for (int s = 0; s < BDF_NEWROWS_STATS; s++) st[s] = 0.0;
    const int64_t trip = pair_trip();
    if (trip * 8 < a.pair.n) {                             // (uniform over the group's 8 lanes)
        const double alpha = a.w.link == 1 ? 1.0 : pair_alpha(a.pair);
        PairLane<2> ln;
        pair_lane(a.pair, trip, ln);
        const double y = a.pair.values[ln.pm];
        const double q = a.q[ln.my[1]];
        const double m = pair_dot<2, VEC, NC>(a.pair, ln) + a.pair.mean;
        if (ln.ok) bdf_newrows_step(a.w, a.pl, ln.pm, y, m, q, alpha, st);
    }
    block_stats8(a.partial, st);
}

// The same cells on the same lanes as k_newrows_update -- cell 256 block + thread -- so that the workgroups' statistics and their
// fixed-order sum are the same sums; every lane reaches the statistics' barrier.
__global__ __launch_bounds__(256) void k_newrows_cells(NewCellArgs a)
{
    double st[BDF_NEWROWS_STATS];
#pragma unroll
    for (int s = 0; s < BDF_NEWROWS_STATS; s++) st[s] = 0.0;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < a.n) {
        const double alpha = a.w.link == 1 ? 1.0 : (a.alpha_dev ? *a.alpha_dev : a.alpha);
        bdf_newrows_step(a.w, a.pl, i, a.values[i], a.m[i], a.q[i], alpha, st);
    }
    block_stats8(a.partial, st);
}

struct NewReadArgs {
    int64_t n;
    const int32_t *orig;
    const double *values, *mean, *M2, *sq, *M, *A;
    double draws, log_draws;
    int link, score;
    double *out;
};

__global__ __launch_bounds__(256) void k_newrows_read(NewReadArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const double y = a.values[i];
    double *o = a.out + 3 * (a.orig ? (int64_t)a.orig[i] : i);
    o[0] = a.mean[i];
    o[1] = bdf_newrows_stdev(a.link, a.M2[i], a.sq[i], a.draws);
    o[2] = (a.score && y == y) ? a.M[i] + log(a.A[i]) - a.log_draws : NAN;
}

}  // namespace

extern "C" int bdf_newrows_quad(bdf_ctx *ctx, int D, int64_t M, const double *Lambda_dev, const double *V_dev, double *q_out)
{
    BDF_REQUIRE(ctx && Lambda_dev, BDF_ERR_ARG, "bdf_newrows_quad: NULL argument");
    BDF_REQUIRE(D >= 1 && D <= BDF_MAX_D, BDF_ERR_ARG, "bdf_newrows_quad: num_latent=%d must be in 1..%d", D, BDF_MAX_D);
    BDF_REQUIRE(M >= 0 && (M == 0 || (V_dev && q_out)), BDF_ERR_ARG, "bdf_newrows_quad: M=%lld rows need V_dev and q_out", (long long)M);
    const int64_t nblocks = (M + BDF_NEWROWS_TILE - 1) / BDF_NEWROWS_TILE;
    BDF_REQUIRE(nblocks <= INT32_MAX, BDF_ERR_ARG, "bdf_newrows_quad: %lld rows are more than one launch covers", (long long)M);
    if (M == 0) return BDF_OK;
    BDF_HIP(hipSetDevice(ctx->device));
    if (!ctx->newrows_W) { if (int rc = ctx->newrows_W.alloc((size_t)BDF_MAX_D * BDF_MAX_D)) return rc; }
    const int DP = D <= 16 ? 16 : (D <= 32 ? 32 : 64);
    hipLaunchKernelGGL(k_newrows_prep, dim3(1), dim3(64), 0, ctx->stream, D, DP, Lambda_dev, ctx->newrows_W, ctx->flag_dev);
    const double *W = ctx->newrows_W;
    if (DP == 16) hipLaunchKernelGGL(k_newrows_quad<16>, dim3((unsigned)nblocks), dim3(256), 0, ctx->stream, D, M, W, V_dev, q_out);
    else if (DP == 32) hipLaunchKernelGGL(k_newrows_quad<32>, dim3((unsigned)nblocks), dim3(256), 0, ctx->stream, D, M, W, V_dev, q_out);
    else hipLaunchKernelGGL(k_newrows_quad<64>, dim3((unsigned)nblocks), dim3(256), 0, ctx->stream, D, M, W, V_dev, q_out);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}

// ---- what the two updates share on the host ---------------------------------------------------------------------------------------
// the checks of the pairs, the phase and the call's per-cell inputs (`inputs`: what they are called, or NULL when they are there)
static int newrows_check(const char *who, const bdf_ctx *ctx, const bdf_pairs *p, int phase, int score_lpd, const double *stats_out, const char *inputs)
{
    BDF_REQUIRE(ctx && p && stats_out, BDF_ERR_ARG, "%s: NULL argument", who);
    BDF_REQUIRE(p->n_modes == 2, BDF_ERR_ARG, "%s: the cells of new rows belong to a two-mode relation, not %d modes", who, p->n_modes);
    BDF_REQUIRE(p->link <= 1, BDF_ERR_ARG, "%s: pairs with the logistic or the count link have no closed form for a new row", who);
    BDF_REQUIRE(!p->baseline_dev && !p->scale_dev, BDF_ERR_ARG, "%s: pairs with a baseline or a precision scale are not predicted for new rows", who);
    BDF_REQUIRE(phase >= 0 && phase <= 2, BDF_ERR_ARG, "%s: phase must be 0, 1 or 2", who);
    BDF_REQUIRE(p->n == 0 || !inputs, BDF_ERR_ARG, "%s: %s is NULL", who, inputs);
    BDF_REQUIRE(phase != 2 || p->newrows_draws >= 1.0, BDF_ERR_ARG, "%s: phase 2 before a phase 1: the pairs hold no draw", who);
    BDF_REQUIRE(phase != 2 || p->newrows_score == (score_lpd != 0), BDF_ERR_ARG, "%s: score_lpd changed between phase 1 and phase 2", who);
    return BDF_OK;
}

// the running state (allocated at the first phase 1 or 2), the draw's constants and the scratch of the workgroups' statistics
static int newrows_draw(bdf_ctx *ctx, bdf_pairs *p, int phase, double clamp_lo, double clamp_hi, double class_cut, int score_lpd, int nblocks,
                        bdf_newrows_draw &w, bdf_newrows_planes &pl, double **partial)
{
    const int64_t n = p->n;
    if (phase >= 1 && !p->newrows_dev) {
        if (int rc = p->newrows_dev.alloc((size_t)n * BDF_NEWROWS_PLANES)) return rc;
        BDF_HIP(hipMemsetAsync(p->newrows_dev, 0, (size_t)n * BDF_NEWROWS_PLANES * sizeof(double), ctx->stream));
    }
    if (p->newrows_dev) { pl.mean = p->newrows_dev; pl.M2 = pl.mean + n; pl.sq = pl.M2 + n; pl.M = pl.sq + n; pl.A = pl.M + n; }
    w.link = p->link; w.phase = phase; w.score = score_lpd != 0;
    w.draws = phase == 2 ? p->newrows_draws + 1.0 : 1.0;
    w.log_draws = log(w.draws);
    w.clamp_lo = clamp_lo; w.clamp_hi = clamp_hi; w.cut = class_cut;
    void *sc;
    int rc = bdf_scratch(ctx, (size_t)nblocks * BDF_NEWROWS_STATS * sizeof(double), &sc);
    if (rc) return rc;
    *partial = (double *)sc;
    return BDF_OK;
}

// behind the update's launch: the fixed-order sum of its statistics, and the draws the pairs hold
static int newrows_done(bdf_ctx *ctx, bdf_pairs *p, int phase, int score_lpd, int nblocks, const double *partial, double *stats_out)
{
    if (p->n > 0) {
        hipLaunchKernelGGL(k_newrows_final, dim3(1), dim3(256), 0, ctx->stream, nblocks, partial, stats_out);
        BDF_HIP(hipGetLastError());
    }
    if (phase == 1) { p->newrows_draws = 1.0; p->newrows_score = score_lpd != 0; }
    else if (phase == 2) p->newrows_draws += 1.0;
    return BDF_OK;
}

extern "C" int bdf_newrows_update(bdf_ctx *ctx, bdf_pairs *p, int D, const double *uhat_new_dev, const double *V_dev, const double *q_dev,
                                  double mean_value, double alpha, const double *alpha_dev, int phase, double clamp_lo, double clamp_hi,
                                  double class_cut, int score_lpd, double *stats_out)
{
    const char *who = "bdf_newrows_update";
    int rc = newrows_check(who, ctx, p, phase, score_lpd, stats_out, q_dev ? nullptr : "q_dev");
    if (rc) return rc;
    const double *fac[2] = {uhat_new_dev, V_dev};
    NewArgs a = {};
    int nblocks;
    if ((rc = pair_fill(who, ctx, p, D, fac, mean_value, p->link != 1, alpha, alpha_dev, a.pair))) return rc;
    if ((rc = pair_blocks(who, "cells", p->n, &nblocks, INT32_MAX / BDF_NEWROWS_STATS))) return rc;
    BDF_HIP(hipSetDevice(ctx->device));
    if (p->n == 0) {
        BDF_HIP(hipMemsetAsync(stats_out, 0, BDF_NEWROWS_STATS * sizeof(double), ctx->stream));
    } else {
        if ((rc = newrows_draw(ctx, p, phase, clamp_lo, clamp_hi, class_cut, score_lpd, nblocks, a.w, a.pl, &a.partial))) return rc;
        a.q = q_dev;
        if ((D & 3) != 0) hipLaunchKernelGGL((k_newrows_update<1, 1>), dim3(nblocks), dim3(256), 0, ctx->stream, a);
        else if (D <= 32) hipLaunchKernelGGL((k_newrows_update<4, 1>), dim3(nblocks), dim3(256), 0, ctx->stream, a);
        else hipLaunchKernelGGL((k_newrows_update<4, 2>), dim3(nblocks), dim3(256), 0, ctx->stream, a);
    }
    return newrows_done(ctx, p, phase, score_lpd, nblocks, a.partial, stats_out);
}

extern "C" int bdf_newrows_update_cells(bdf_ctx *ctx, bdf_pairs *p, const double *m_dev, const double *q_dev, double alpha, const double *alpha_dev,
                                        int phase, double clamp_lo, double clamp_hi, double class_cut, int score_lpd, double *stats_out)
{
    const char *who = "bdf_newrows_update_cells";
    int rc = newrows_check(who, ctx, p, phase, score_lpd, stats_out, (m_dev && q_dev) ? nullptr : "m_dev or q_dev");
    if (rc) return rc;
    BDF_REQUIRE(p->link == 1 || alpha_dev || (alpha > 0.0 && std::isfinite(alpha)), BDF_ERR_ARG, "%s: alpha=%g must be positive and finite", who, alpha);
    NewCellArgs a = {};
    int nblocks;
    if ((rc = pair_blocks(who, "cells", p->n, &nblocks, INT32_MAX / BDF_NEWROWS_STATS))) return rc;
    BDF_HIP(hipSetDevice(ctx->device));
    if (p->n == 0) {
        BDF_HIP(hipMemsetAsync(stats_out, 0, BDF_NEWROWS_STATS * sizeof(double), ctx->stream));
    } else {
        if ((rc = newrows_draw(ctx, p, phase, clamp_lo, clamp_hi, class_cut, score_lpd, nblocks, a.w, a.pl, &a.partial))) return rc;
        a.n = p->n; a.values = p->values_dev; a.m = m_dev; a.q = q_dev; a.alpha = alpha; a.alpha_dev = alpha_dev;
        hipLaunchKernelGGL(k_newrows_cells, dim3(nblocks), dim3(256), 0, ctx->stream, a);
    }
    return newrows_done(ctx, p, phase, score_lpd, nblocks, a.partial, stats_out);
}

extern "C" int bdf_newrows_result(bdf_ctx *ctx, const bdf_pairs *p, double *out_dev)
{
    BDF_REQUIRE(ctx && p, BDF_ERR_ARG, "bdf_newrows_result: NULL argument");
    BDF_REQUIRE(p->newrows_draws >= 1.0, BDF_ERR_ARG, "bdf_newrows_result: the pairs hold no posterior draw (bdf_newrows_update with phase 1 first)");
    if (p->n == 0) return BDF_OK;
    BDF_REQUIRE(out_dev != nullptr, BDF_ERR_ARG, "bdf_newrows_result: out_dev is NULL");
    BDF_REQUIRE((p->n + 255) / 256 <= INT32_MAX, BDF_ERR_ARG, "bdf_newrows_result: %lld cells are more than one launch covers", (long long)p->n);
    const int64_t n = p->n;
    NewReadArgs a;
    a.n = n; a.orig = p->orig_dev; a.values = p->values_dev;
    a.mean = p->newrows_dev; a.M2 = a.mean + n; a.sq = a.M2 + n; a.M = a.sq + n; a.A = a.M + n;
    a.draws = p->newrows_draws; a.log_draws = log(a.draws); a.link = p->link; a.score = p->newrows_score; a.out = out_dev;
    BDF_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_newrows_read, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, a);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}

extern "C" int bdf_newrows_state(const bdf_pairs *p, double **state_dev, double *draws)
{
    BDF_REQUIRE(p && state_dev && draws, BDF_ERR_ARG, "bdf_newrows_state: NULL argument");
    *state_dev = p->newrows_dev; *draws = p->newrows_draws;
    return BDF_OK;
}
