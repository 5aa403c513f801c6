// k_background.hip -- background cells of a two-mode relation (implicit feedback): every cell that is not
// listed observes a background value with precision alpha c0.  The dense part of every row's conditional is the Gram matrix of the
// other entity's rows, which all rows share, so it is folded into the PRIOR the existing row kernels take:
//
//   bdf_background_prior   k_bg_fold: one wave.  Lambda_eff = Lambda + sum_k alpha_k c0_k G_k, factored as wave_linalg.h factors
//                          (lane = column, the matrix in registers), then mu_eff = Lambda_eff^-1 (Lambda mu + sum_k alpha_k c0_k rb_k
//                          s_k) and the prior pack of (mu_eff, Lambda_eff) -- or, for per-row prior means, W = Lambda_eff^-1 Lambda
//                          and w0, and k_bg_mu_rows: mu_eff_i = W mu_i + w0 over the N rows on v_mfma_f64_16x16x4_f64, W through
//                          LDS once per workgroup, rows past N and D off the tile by predication.
//   bdf_background_sse     k_bg_sse: the gather of bdf_pairs_weighted_sse with the listed cell's second term, then one workgroup adds
//                          the workgroups' sums, the Gram inner product and the closed-form remainder in a fixed order.
//
// What k_bg_fold shares with k_dmat_fold of k_dense.hip -- the term record and its checks, Lambda_eff and its factorisation, the
// refined solve, the closing kernels' four-wave sum -- is written once in prior_fold.h.
// Every solve takes one step of iterative refinement: the pivots' reciprocals are good to 1.5e-15 (fast_rcp), and what the rows
// read is Lambda_eff mu_eff, the solve's right-hand side again -- its residual, not its forward error, is what reaches them.
// Plain vector stores, no floating-point atomics; no scratch memory except k_bg_fold<64>'s 528 bytes per lane, which wl_factor<64>
// brings to every kernel that takes it (k_solve_small<64> has the same).
#include "bdf_common.h"
#include "background.h"
#include "pair_gather.h"
#include "prior_fold.h"
#include "rows.h"
#include "wave_linalg.h"

namespace {

typedef double bd2 __attribute__((ext_vector_type(2)));
typedef double bd4 __attribute__((ext_vector_type(4)));

// the fold's own outputs behind the shared head (prior_fold.h)
struct BgFoldArgs : FoldHead {       // mu NULL: per-row prior means -- T_out and w0_out are written instead of mu_out and the pack
    double *mu_out, *pack_out;
    double *T_out, *w0_out;    // T[e * DP + d] = W[d][e] (DP x DP row-major, zero outside D x D), w0 (DP, zero behind D)
};

// fold_head (prior_fold.h) builds and factors Lambda_eff; what follows is the background's own: the shared mean with the prior pack,
// or W and w0 for per-row prior means
template <int DP>
__global__ __launch_bounds__(64) void k_bg_fold(BgFoldArgs a)
{
    using W = WL<DP>;
    constexpr int G = W::G;
    __shared__ double tri[W::TRI + 64];
    __shared__ double sA[DP * DP];          // Lambda_eff: sA[i + c * DP] = element (i, c); identity on the padding
    __shared__ double s_mu[DP];
    const int lane = threadIdx.x, c = lane % DP, grp = lane / DP;
    const int D = a.D;
    const bool in = c < D;
    double ac[BDF_MAX_TERMS], col[DP], t_c, p_own, rp_own;
    fold_head<DP>(a, true, ac, col, t_c, p_own, rp_own, tri, sA, lane);

    if (a.mu == nullptr) {
        // per-row prior means: W = Lambda_eff^-1 Lambda by columns, G of them side by side, and w0 = Lambda_eff^-1 t
        for (int q0 = 0; q0 < D; q0 += G) {
            const int q = q0 + grp;
            const double b = (q < D && in) ? a.Lambda[c + (int64_t)q * D] : 0.0;
            const double x = fold_solve<DP>(col, tri, sA, rp_own, b, lane);
            if (q < D) a.T_out[q * DP + c] = in ? x : 0.0;
        }
        for (int q = D + grp; q < DP; q += G) a.T_out[q * DP + c] = 0.0;
        const double x0 = fold_solve<DP>(col, tri, sA, rp_own, t_c, lane);
        if (grp == 0) a.w0_out[c] = in ? x0 : 0.0;
        return;
    }
    // a shared prior mean: mu_eff = Lambda_eff^-1 (Lambda mu + t)
    double b = t_c;
    if (in)
        for (int i = 0; i < D; i++) b = fma(a.Lambda[c + (int64_t)i * D], a.mu[i], b);
    const double x = fold_solve<DP>(col, tri, sA, rp_own, b, lane);
    if (grp == 0) {
        if (in) a.mu_out[c] = x;
        s_mu[c] = in ? x : 0.0;
    }
    if (a.pack_out == nullptr) return;
    wave_sync();
    // the prior pack of (mu_eff, Lambda_eff), bit for bit what k_prior (k_sample_rows.hip) derives from them: Lambda_eff mu_eff by
    // eight chains i = p, p + 8, ... and their butterfly as lane part 0 sees it, then the accumulator-layout image of the
    // index-reversed Lambda_eff, identity on the padding
    if (lane < D) {
        double v[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < DP; i++)
            if (i < D) v[i & 7] = fma(sA[lane + i * DP], s_mu[i], v[i & 7]);
        a.pack_out[lane] = ((v[0] + v[4]) + (v[2] + v[6])) + ((v[1] + v[5]) + (v[3] + v[7]));
    }
    constexpr int DB = DP / 16;
    for (int e = 0; e < DB * (DB + 1) / 2 * 4; e++) {
        const int blk = e >> 2, r = e & 3;
        int I = 0;
        while ((I + 1) * (I + 2) / 2 <= blk) I++;
        const int J = blk - I * (I + 1) / 2;
        const int row = 16 * I + (lane >> 4) + 4 * r, colm = 16 * J + (lane & 15);
        const int er = D - 1 - row, ecm = D - 1 - colm;
        double v = (row == colm) ? 1.0 : 0.0;
        if (er >= 0 && ecm >= 0) v = sA[er + ecm * DP];
        else if (er >= 0 || ecm >= 0) v = 0.0;
        a.pack_out[D + e * 64 + lane] = v;
    }
}

// Y_i = W X_i + w0 for the N rows of D doubles (X, Y row-major with leading dimension D): Y = X T + w0 with T = W' (DP x DP
// row-major, zero-padded).  A tile is 16 rows; the DB = DP / 16 waves of a tile each take one 16-column block of the result; the
// contraction runs over e = kk DP / 4 + s (lane row kk, k-step s), as k_rowmat of k_rows_lr.hip lays it out.  T comes through LDS
// once per workgroup (every wave then keeps its block in registers), the tiles come through LDS with 64 consecutive doubles per
// load instruction, the next tile's loads in flight under this tile's matrix instructions.
template <int DP>
__global__ __launch_bounds__(256) void k_bg_mu_rows(const double *__restrict__ X, double *__restrict__ Y, const double *__restrict__ T,
                                                    const double *__restrict__ w0, int D, int64_t n_rows, int64_t n_iters)
{
    constexpr int DB = DP / 16, KQ = DP / 4, TPW = 4 / DB, LDT = DP + 2;
    __shared__ __attribute__((aligned(16))) double tile[TPW][16 * LDT];
    __shared__ double sT[DP * DP];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = lane & 15, kk = lane >> 4;
    const int sub = wave / DB, cb = wave % DB;
    for (int e = threadIdx.x; e < DP * DP; e += 256) sT[e] = T[e];
    __syncthreads();
    double b[KQ];
#pragma unroll
    for (int s = 0; s < KQ; s++) b[s] = sT[(kk * KQ + s) * DP + 16 * cb + i];
    const int col = 16 * cb + i;
    const double bias = w0[col];
    // this wave's share of its tile's loads: rows cb * 16 / DB .. of the tile
    int trow[4], tcol[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int E = cb * (16 / DB) * DP + q * 64 + lane;
        trow[q] = E / DP; tcol[q] = E % DP;
    }
    auto tile_row = [&](int64_t it, int r16) -> int64_t {
        const int64_t r = (it * TPW + sub) * 16 + r16;
        return (it < n_iters && r < n_rows) ? r : -1;
    };
    auto tile_load = [&](double (&g)[4], int64_t it) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int64_t row = tile_row(it, trow[q]);
            g[q] = (row >= 0 && tcol[q] < D) ? X[row * D + tcol[q]] : 0.0;
        }
    };
    double g[4];
    tile_load(g, blockIdx.x);
    for (int64_t it = blockIdx.x; it < n_iters; it += gridDim.x) {
#pragma unroll
        for (int q = 0; q < 4; q++) tile[sub][trow[q] * LDT + tcol[q]] = g[q];
        __syncthreads();                               // the tile is in LDS
        tile_load(g, it + gridDim.x);                  // the next tile's rows, under this tile's matrix instructions
        double av[KQ];
        const double *src = &tile[sub][i * LDT + kk * KQ];
#pragma unroll
        for (int s = 0; s < KQ; s += 2) { const bd2 v = *(const bd2 *)(src + s); av[s] = v[0]; av[s + 1] = v[1]; }
        bd4 acc = bd4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < KQ; s++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], b[s], acc, 0, 0, 0);
        // C layout: lane (j = i, h = kk), register r: tile row h + 4 r, column 16 cb + j
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
            const int64_t rowm = tile_row(it, kk + 4 * rr);
            if (rowm >= 0 && col < D) Y[rowm * D + col] = acc[rr] + bias;
        }
        __syncthreads();                               // every wave has read the tile from LDS: the next one may be written
    }
}

// ---- the sum of c e^2 over all N M cells ---------------------------------------------------------------------------------
struct BgSseArgs {
    PairArgs pair;
    const double *weights;         // nullable: omega_k in the caller's order (else 1)
    double c0, rb;
    double *partial;               // one sum per workgroup
};

// one group of 8 lanes per 8 pairs, no grid-stride loop (every lane reaches the sum's barrier): k_weighted_sse's shape
template <int VEC, int NC>
__global__ __launch_bounds__(256, 3) void k_bg_sse(BgSseArgs a)
{
    __shared__ double red[4];
    const int tid = threadIdx.x;
    const int64_t trip = pair_trip();
    double term = 0.0;
    if (trip * 8 < a.pair.n) {
        PairLane<2> l;
        pair_lane(a.pair, trip, l);
        const double y = a.pair.values[l.pm];
        const double psi = pair_dot<2, VEC, NC>(a.pair, l);
        const double e = (y - a.pair.mean) - psi;
        if (l.ok) term = bdf_bg_term(a.weights ? a.weights[l.po] : 1.0, e, a.c0, a.rb, psi);
    }
    double v = term;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) a.partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// the workgroups' sums, (sum U).(sum V) and <U U', V V'> added in a fixed order, then the closed form
__global__ __launch_bounds__(256) void k_bg_sse_final(int nblocks, const double *partial, int D, const double *sumU, const double *gramU,
                                                      const double *sumV, const double *gramV, double c0, double rb, double cells, double *out)
{
    __shared__ double red[4];
    const int tid = threadIdx.x;
    double s = 0.0, d = 0.0, g = 0.0;
    for (int b = tid; b < nblocks; b += 256) s += partial[b];
    for (int e = tid; e < D; e += 256) d = fma(sumU[e], sumV[e], d);
    for (int e = tid; e < D * D; e += 256) g = fma(gramU[e], gramV[e], g);
    s = block_sum4(s, red);
    d = block_sum4(d, red);
    g = block_sum4(g, red);
    if (tid == 0) *out = s + bdf_bg_all_cells(c0, cells, rb, d, g);
}

}  // namespace

extern "C" int bdf_background_prior(bdf_ctx *ctx, int D, int64_t N, int n_bg, const bdf_background_term *bg, const double *mu, int mu_is_matrix,
                                    const double *Lambda, double *Lambda_out, double *mu_out, double *prior_pack_out, double *alpha_rows_out)
{
    BDF_REQUIRE(!(mu_is_matrix && prior_pack_out), BDF_ERR_ARG, "bdf_background_prior: per-row prior means have no prior pack");
    BgFoldArgs a = {};
    int rc = fold_fill("bdf_background_prior", ctx, D, N, n_bg, bg, mu, mu_is_matrix, Lambda, Lambda_out, mu_out, alpha_rows_out, a);
    if (rc) return rc;
    const int DP = bdf_rows_dp(D);
    a.mu_out = mu_out; a.pack_out = prior_pack_out;
    if (mu_is_matrix) {
        void *sc;
        if ((rc = bdf_scratch(ctx, ((size_t)DP * DP + DP) * sizeof(double), &sc))) return rc;
        a.T_out = (double *)sc; a.w0_out = a.T_out + (size_t)DP * DP;
    }
    if (DP == 16) hipLaunchKernelGGL(k_bg_fold<16>, dim3(1), dim3(64), 0, ctx->stream, a);
    else if (DP == 32) hipLaunchKernelGGL(k_bg_fold<32>, dim3(1), dim3(64), 0, ctx->stream, a);
    else hipLaunchKernelGGL(k_bg_fold<64>, dim3(1), dim3(64), 0, ctx->stream, a);
    if (mu_is_matrix && N > 0) {
        const int tpw = 4 / (DP / 16);
        const int64_t iters = (N + 16 * tpw - 1) / (16 * tpw);
        const dim3 grid((unsigned)std::min<int64_t>(iters, 4096));
        if (DP == 16) hipLaunchKernelGGL(k_bg_mu_rows<16>, grid, dim3(256), 0, ctx->stream, mu, mu_out, (const double *)a.T_out, (const double *)a.w0_out, D, N, iters);
        else if (DP == 32) hipLaunchKernelGGL(k_bg_mu_rows<32>, grid, dim3(256), 0, ctx->stream, mu, mu_out, (const double *)a.T_out, (const double *)a.w0_out, D, N, iters);
        else hipLaunchKernelGGL(k_bg_mu_rows<64>, grid, dim3(256), 0, ctx->stream, mu, mu_out, (const double *)a.T_out, (const double *)a.w0_out, D, N, iters);
    }
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}

extern "C" int bdf_background_sse(bdf_ctx *ctx, const bdf_pairs *train, int D, const double *const *factors, double mean_value,
                                  const double *weights, double value, double weight, const double *sumU, const double *gramU,
                                  const double *sumV, const double *gramV, int64_t N, int64_t M, double *out)
{
    BDF_REQUIRE(sumU && gramU && sumV && gramV && out, BDF_ERR_ARG, "bdf_background_sse: NULL argument");
    BDF_REQUIRE(weight > 0.0 && weight <= 1.0 && std::isfinite(value), BDF_ERR_ARG, "bdf_background_sse: weight=%g must lie in (0, 1] and value=%g be finite", weight, value);
    BDF_REQUIRE(N >= 0 && M >= 0, BDF_ERR_ARG, "bdf_background_sse: N or M < 0");
    BgSseArgs a = {};
    int rc = pair_fill("bdf_background_sse", ctx, train, D, factors, mean_value, false, 0.0, nullptr, a.pair);
    if (rc) return rc;
    BDF_REQUIRE(train->n_modes == 2, BDF_ERR_ARG, "bdf_background_sse: a background takes a two-mode relation, not %d modes", train->n_modes);
    a.weights = weights; a.c0 = weight; a.rb = value - mean_value;
    int nblocks;
    if ((rc = pair_blocks("bdf_background_sse", "observations", train->n, &nblocks))) return rc;
    BDF_HIP(hipSetDevice(ctx->device));
    void *sc;
    if ((rc = bdf_scratch(ctx, (size_t)std::max(nblocks, 1) * sizeof(double), &sc))) return rc;
    a.partial = (double *)sc;
    if (nblocks > 0) {
        if (D & 3) hipLaunchKernelGGL((k_bg_sse<1, 1>), dim3(nblocks), dim3(256), 0, ctx->stream, a);
        else if (D <= 32) hipLaunchKernelGGL((k_bg_sse<4, 1>), dim3(nblocks), dim3(256), 0, ctx->stream, a);
        else hipLaunchKernelGGL((k_bg_sse<4, 2>), dim3(nblocks), dim3(256), 0, ctx->stream, a);
    }
    hipLaunchKernelGGL(k_bg_sse_final, dim3(1), dim3(256), 0, ctx->stream, nblocks, (const double *)a.partial, D, sumU, gramU, sumV, gramV,
                       weight, a.rb, (double)N * (double)M, out);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}
