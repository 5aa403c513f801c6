// k_sample_rows.hip -- K1: the latent-row sampler.
//
// Replaces sample_user_basic (src/sampling.jl:200-212 matrix, :215-234 tensor) and sample_user2
// (src/sampling.jl:266-289, sum over the entity's relations) of the reference, for every row of an
// entity at once (sample_latent_all2! :149-172, sample_user2_all! :251-264).
//
// Per row i:
//   S   = sum over the row's observations of w w',  w = Hadamard product of the other modes' factor rows
//   P_i = Lambda + sum_r alpha_r S_r          b_i = Lambda mu_i + sum_r alpha_r sum w (y - base)
//   x_i = chol(inv(P_i))' z + inv(P_i) b_i    (the reference's map from z to the sample)
//
// The reference forms inv(P_i) by LU and then a Cholesky factor of the covariance.  Here P_i is factored
// once as P_i = U U' with U UPPER triangular (a Cholesky factorisation run from the last index to the
// first).  Then inv(P_i) = U^-T U^-1 with U^-T lower triangular and positive diagonal, so by uniqueness
// of the Cholesky factor chol(inv(P_i))' == U^-T, and  x_i = U^-T (U^-1 b_i + z):  one factorisation and
// two triangular solves give exactly the reference's function of z (to fp64 rounding).
// All of it runs in index-reversed coordinates (e -> D-1-e), where U U' becomes an ordinary lower
// Cholesky L L' and the two solves become forward then backward substitution.
//
// Work decomposition (ragged rows: MovieLens rows have 0..1668 observations):
//   * a row's observations are cut into ITEMS of at most T observations; ONE WAVEFRONT PER ITEM.
//   * a row with a single item is DIRECT: the wave that accumulated it also factors, solves and draws.
//   * a row with several items (long rows, or several relations) is SPLIT: its items write partial (S, b) to a
//     scratch slab and count themselves in; the wave whose arrival completes the row adds the row's partials in slot
//     order and finishes it, inside the same launch.
//   so no wave ever owns more than T observations and results do not depend on scheduling.
//
// Accumulation: the rank-4 update S += W W' (W = D x 4 gathered factor rows) is one v_mfma_f64_16x16x4_f64 per
// 16x16 block of the lower block-triangle.  The MFMA A/B operand of lane l is element (l & 15) of observation
// (l >> 4): exactly what a coalesced 128-byte-per-16-lanes gather of the factor row delivers, so operands go from
// global memory to the matrix pipe with no LDS staging and no cross-lane traffic (measured on MI355X: 64 cycles
// per MFMA, 77 TFLOP/s chip-wide against 64 TFLOP/s for v_fma_f64 which would also need every operand broadcast).
//
// Finishing happens IN THE ACCUMULATOR LAYOUT, with the matrix never leaving the registers the MFMAs left it in:
// lane (j = l & 15, h = l >> 4), register r of block (I, J) holds element (16 I + h + 4 r, 16 J + j) -- a lane owns
// DB columns (j, 16 + j, ...) and of each the rows of its class h (mod 4): 12 doubles for D <= 32.  Step k of the
// right-looking factorisation needs, in lane (j, h), the entries of column k in the lane's rows -- they sit in lane
// (k % 16, h), same row of 16 lanes, same registers: a DPP row broadcast folded into the fma (v_fmac_f64_dpp
// row_newbcast) -- and the multipliers of the lane's columns, read from the copy of column k that its four owner
// lanes put in LDS (the packed factor that the backward solve reads anyway).  b rides along as one more matrix row,
// which makes the forward solve part of the factorisation.  The low register count (about a third of a
// column-per-lane layout) is what lets 5-6 waves share a SIMD and hide each other's dependent-step latencies.
//
// This unit holds K1 alone; the device code it shares with k_rows_ss.hip (the gathers, the accumulation, the work item) is in
// k1_accumulate.h.  Which rows it gets -- and which go to k_rows_lr, k_rows_small or k_rows_col instead -- is decided
// by the router (rows_plan.hip: bdf_launch_sample_rows), which also cuts them into the items of PlanDev (rows.h).
#include "k1_accumulate.h"

namespace {

// ---- prior: a small pre-launch writes Lambda mu_i (the prior part of b) and the image of the index-reversed Lambda in
// the accumulator layout ([block * 4 + r][lane], identity on the padding), which every wave adds with coalesced loads. ----
__global__ __launch_bounds__(256) void k_prior(int D, int DP, int64_t nrows, const double *Lambda, const double *mu,
                                               int mu_is_matrix, double *out_b, double *out_c)
{
    // groups of eight lanes 0 .. nrows*D-1: out_b[row*D + e] = sum_i Lambda[e][i] mu_row[i]  (nrows = 1 for a shared prior
    // mean); lane part p adds i = p, p+8, ... in order, then a three-step butterfly (the order k_hyper_sample uses too).
    // Then NB*4 waves, one per (block, register) of the image.
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int DB = DP / 16;
    const int64_t nb8 = (nrows * D + 7) / 8;                  // waves used by the first part
    if ((t >> 6) < nb8) {
        const int64_t o = t >> 3;
        const int part = (int)(t & 7);
        double v = 0.0;
        if (o < nrows * D) {
            const int64_t row = o / D;
            const int e = (int)(o % D);
            const double *m = mu_is_matrix ? mu + row * D : mu;
            for (int i = part; i < D; i += 8) v = fma(Lambda[e + (int64_t)i * D], m[i], v);
        }
        v += __shfl_xor(v, 4);
        v += __shfl_xor(v, 2);
        v += __shfl_xor(v, 1);
        if (part == 0 && o < nrows * D) out_b[o] = v;
        return;
    }
    const int64_t idx = (t >> 6) - nb8 + nrows * D;
    const int e = (int)(idx - nrows * D);
    if (e >= DB * (DB + 1) / 2 * 4) return;
    const int b = e >> 2, r = e & 3;
    int I = 0;
    while ((I + 1) * (I + 2) / 2 <= b) I++;
    const int J = b - I * (I + 1) / 2;
    const int row = 16 * I + (lane >> 4) + 4 * r, colm = 16 * J + (lane & 15);
    const int er = D - 1 - row, ecm = D - 1 - colm;
    double v = (row == colm) ? 1.0 : 0.0;
    if (er >= 0 && ecm >= 0) v = Lambda[er + (int64_t)ecm * D];
    else if (er >= 0 || ecm >= 0) v = 0.0;
    out_c[e * 64 + lane] = v;
}

template <int DP, bool DUMP, bool MATRIX, bool CODED = false>
__global__ __launch_bounds__(64 * Geo<DP>::WPB, CODED ? Geo<DP>::WAVES_CODED : (MATRIX ? Geo<DP>::WAVES_MATRIX : Geo<DP>::WAVES))
void k_rows(SampleArgs a, PlanDev p)
{
    using GG = Geo<DP>;
    constexpr int WPB = GG::WPB;
    constexpr int WLDS = K1Local<DP>::value ? GeoL<DP>::WAVE_LDS : GG::WAVE_LDS;
    __shared__ __attribute__((aligned(16))) double lds[WPB * WLDS];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t w = (int64_t)blockIdx.x * WPB + wave;
    if (w < (int64_t)p.n_split + p.n_direct)
        process_item<DP, DUMP, MATRIX, CODED>(a, p, p.order[w], lane, lds + wave * WLDS);
}

// The launch of a call with per-observation precision weights (TermDev::weight: known weights, or the omega of the Student-t
// model -- k_robust.hip): the general variant's workgroup shape and finish around the weighted gather.
// (Waves per SIMD: the weights' square roots and their run-ahead copies sit beside the gather's registers -- under the general
// variant's bounds of 8 and 5 waves the compiler spills; 6 and 4 hold it free of scratch.)
template <int DP>
struct K1WavesW { static constexpr int value = DP == 64 ? 2 : (DP == 32 ? 4 : 6); };

template <int DP, bool DUMP>
__global__ __launch_bounds__(64 * Geo<DP>::WPB, K1WavesW<DP>::value)
void k_rows_w(SampleArgs a, PlanDev p)
{
    using GG = Geo<DP>;
    constexpr int WPB = GG::WPB;
    constexpr int WLDS = K1Local<DP>::value ? GeoL<DP>::WAVE_LDS : GG::WAVE_LDS;
    __shared__ __attribute__((aligned(16))) double lds[WPB * WLDS];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t w = (int64_t)blockIdx.x * WPB + wave;
    if (w < (int64_t)p.n_split + p.n_direct)
        process_item<DP, DUMP, false, false, true>(a, p, p.order[w], lane, lds + wave * WLDS);
}

// Lambda mu_i for MANY rows (per-row prior means: an entity with side information, macau.jl:104) -- one thread per output element with
// its row of Lambda in registers and the rows' means broadcast from LDS, where k_prior spends eight lanes and a butterfly on every
// element (100,000 rows at D = 32: 214 us -> ~20).  The same sums in the same order: the eight chains i = p, p + 8, ... by fma, then
// ((v0 + v4) + (v2 + v6)) + ((v1 + v5) + (v3 + v7)) -- the butterfly as k_prior's lane part 0 sees it.
template <int DPAD>
__global__ __launch_bounds__(256) void k_prior_rows(int D, int64_t nrows, const double *__restrict__ Lambda, const double *__restrict__ mu,
                                                    double *__restrict__ out_b)
{
    __shared__ double m_s[256];
    const int tid = threadIdx.x;
    const int RP = 256 / D;                                // rows per pass
    const int r = tid / D, e = tid - r * D;
    const bool mine = r < RP;
    double L[DPAD];
#pragma unroll
    for (int i = 0; i < DPAD; i++) L[i] = (mine && i < D) ? Lambda[e + (int64_t)i * D] : 0.0;
    for (int64_t row0 = (int64_t)blockIdx.x * RP; row0 < nrows; row0 += (int64_t)gridDim.x * RP) {
        const bool ok = mine && row0 + r < nrows;
        if (ok) m_s[tid] = mu[(row0 + r) * D + e];         // (tid == r * D + e: the pass's rows are contiguous)
        __syncthreads();
        if (ok) {
            const double *m = m_s + r * D;
            double v[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int i = 0; i < DPAD; i++)
                if (i < D) v[i & 7] = fma(L[i], m[i], v[i & 7]);
            out_b[(row0 + r) * D + e] = ((v[0] + v[4]) + (v[2] + v[6])) + ((v[1] + v[5]) + (v[3] + v[7]));
        }
        __syncthreads();
    }
}

// which k_rows variant a launch takes: every term a two-mode relation on the lean gather path (matrix), and of those the
// launches with ONE relation whose values are coded (ratings)
void launch_kind(const SampleArgs &a, bool dump, bool &matrix, bool &coded, bool &weighted, bool wide_ok = false)
{
    weighted = false;          // any term with per-observation weights: the whole launch takes k_rows_w
    for (int r = 0; r < a.n_terms; r++) weighted = weighted || a.t[r].weight != nullptr;
    matrix = true;             // (wide_ok: D > 32, where the two-mode variant also takes factor matrices of 4 GiB or more -- lean == 2)
    for (int r = 0; r < a.n_terms; r++) matrix = matrix && (a.t[r].lean == 1 || (wide_ok && a.t[r].lean == 2)) && a.t[r].n_other == 1;
    static const bool no_matrix = getenv("BDF_K1_GENERAL_KERNEL") != nullptr;      // test hook: the general variant
    matrix = matrix && !no_matrix && !weighted;
    static const bool no_coded = getenv("BDF_K1_NO_CODED") != nullptr;               // test hook: the uncoded two-mode variant
    coded = matrix && !dump && !no_coded && a.n_terms == 1 && a.t[0].lean == 1 && a.t[0].packed != nullptr && a.t[0].n_codes <= BDF_K1_CODES;
}

template <int DP>
int launch(bdf_ctx *ctx, const SampleArgs &a, const PlanDev &p, bool dump, hipEvent_t e0, hipEvent_t e1)
{
    constexpr int WPB = Geo<DP>::WPB;
    bool matrix, coded, weighted;
    launch_kind(a, dump, matrix, coded, weighted, DP == 64);
    const int64_t waves = (int64_t)p.n_split + p.n_direct;
    const dim3 grid((unsigned)((waves + WPB - 1) / WPB)), block(64 * WPB);
    auto kern = dump ? (matrix ? k_rows<DP, true, true> : k_rows<DP, true, false>)
                     : (coded ? k_rows<DP, false, true, true> : (matrix ? k_rows<DP, false, true> : k_rows<DP, false, false>));
    if (weighted) kern = dump ? k_rows_w<DP, true> : k_rows_w<DP, false>;
    // start / stop events (bdf_ctx_time_next_rows) ride on the dispatch packet itself: the kernel's own begin and end,
    // no marker packets around it
    hipExtLaunchKernelGGL(kern, grid, block, 0, ctx->stream, e0, e1, 0, a, p);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}

}  // namespace

// K1 over the items of `p` (at least one), one wave each
int bdf_k1_launch(bdf_ctx *ctx, const SampleArgs &a, const PlanDev &p, bool dump, hipEvent_t e0, hipEvent_t e1)
{
    const int DP = bdf_rows_dp(a.D);
    if (DP == 16) return launch<16>(ctx, a, p, dump, e0, e1);
    if (DP == 32) return launch<32>(ctx, a, p, dump, e0, e1);
    return launch<64>(ctx, a, p, dump, e0, e1);
}

int bdf_prior_launch(bdf_ctx *ctx, int D, const double *Lambda, const double *mu, int64_t nrows, int mu_is_matrix, double *out_b, double *out_c)
{
    const int DPp = bdf_rows_dp(D);
    const int nimg = bdf_prior_image_doubles(D) / 64;          // (block, register) pairs of the image
    const bool many = mu_is_matrix && nrows >= 4096;
    if (many) {
        // many rows: Lambda mu_i by k_prior_rows (the same sums in the same order), the image alone by k_prior (nrows = 0)
        const int RP = 256 / D;
        const unsigned grid = (unsigned)std::min<int64_t>((nrows + RP - 1) / RP, 4096);
        if (DPp == 16) hipLaunchKernelGGL(k_prior_rows<16>, dim3(grid), dim3(256), 0, ctx->stream, D, nrows, Lambda, mu, out_b);
        else if (DPp == 32) hipLaunchKernelGGL(k_prior_rows<32>, dim3(grid), dim3(256), 0, ctx->stream, D, nrows, Lambda, mu, out_b);
        else hipLaunchKernelGGL(k_prior_rows<64>, dim3(grid), dim3(256), 0, ctx->stream, D, nrows, Lambda, mu, out_b);
    }
    const int64_t nr = many ? 0 : nrows;
    const int64_t waves = (nr * D + 7) / 8 + nimg;
    hipLaunchKernelGGL(k_prior, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, ctx->stream, D, DPp, nr, Lambda, mu, many ? 0 : mu_is_matrix, out_b, out_c);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}
