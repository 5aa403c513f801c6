// k_rows_small.hip -- K1s: D <= 16, short rows of ONE two-mode relation, FOUR ROWS PER WAVE.
//
// At D <= 16 a row of ten observations costs the wave-per-row kernel ~570 vector and ~340 scalar instructions, nearly all of
// them per-row overhead that 64 lanes execute for one 16 x 16 system (normals, index arithmetic, 15 factorisation steps on
// a quarter-filled block): that kernel is issue-bound there (the reference's own benchmark shape: 1.5 M rows of ~10
// observations).  Here every 16-lane row of the wave owns one entity row; lane j of it holds COLUMN j of the index-reversed
// system (16 doubles) and b_j.  Observations come 16 at a time (lane j loads the id and value of observation c0 + j, the ids
// are broadcast inside the 16-lane row by DPP and the 16 gathers are all in flight); the rank-1 updates, the LDL'
// factorisation with the forward solve riding along as one more row, and the backward solve are DPP row-broadcast fmas
// (v_fmac_f64_dpp row_newbcast: lane k of each 16-lane row).  Same arithmetic contract as k_rows: the sample is
// x~ = L~^-T (D^-1 L~^-1 b~ + D^-1/2 z~) of the reversed system P~ = L~ D L~', lane j drawing number D - 1 - j of the row's
// stream; sums over observations run in observation order.
// The rows arrive as RowItem records (rows.h), padded to a multiple of four with row = -1.
#include "rows.h"
#include "dpp_rows16.h"

namespace {

// eight observations of a chunk: ids broadcast inside the 16-lane row, all eight gathers issued (observations past the row's
// end gather row 0 and are masked to zero), then the rank-1 updates
template <int H, int K>
__device__ __forceinline__ void small_gather(double (&v)[8], uint32_t idw, const char *fac, uint32_t rowb, uint32_t eoff)
{
    if constexpr (K < 8) {
        v[K] = *(const double *)(fac + (__umul24(row_bcast_u32<8 * H + K>(idw), rowb) + eoff));      // (lean gather: 32-bit offsets)
        small_gather<H, K + 1>(v, idw, fac, rowb, eoff);
    }
}
template <int DR, int H, int K>
__device__ __forceinline__ void small_chunk(double (&A)[16], double &b, const double (&v)[8], double r, int n_here, bool jok)
{
    if constexpr (K < 8) {
        const double vk = (jok && 8 * H + K < n_here) ? v[K] : 0.0;
        b = fma(vk, row_bcast_f64<8 * H + K>(r), b);
        small_rank1<DR, 0>(A, vk);
        small_chunk<DR, H, K + 1>(A, b, v, r, n_here, jok);
    }
}

#ifndef BDF_SMALL_BLOCKS
#define BDF_SMALL_BLOCKS 1
#endif
template <bool CODED, int DR>
__global__ __launch_bounds__(256, BDF_SMALL_BLOCKS) void k_rows_small(SampleArgs a, const RowItem *items, int64_t n_items)
{
    const int lane = threadIdx.x & 63, j = lane & 15;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w * 4 >= n_items) return;
    const RowItem it = items[w * 4 + (lane >> 4)];
    const bool live = it.row >= 0;
    const int D = a.D;
    const TermDev &T = a.t[0];
    const int ec = D - 1 - j;                   // natural index of reversed element j
    const bool jok = ec >= 0;
    double z = 0.0;
    if (live && jok) z = bdf_normal(a.seed, a.sweep, BDF_P_ROW, a.entity_tag, (uint64_t)(uint32_t)it.orig, ec);
    double A[16];
#pragma unroll
    for (int i = 0; i < 16; i++) A[i] = 0.0;
    double b = 0.0;
    const int n = live ? it.count : 0;
    int nmax = n;
    nmax = max(nmax, __shfl_xor(nmax, 16));
    nmax = max(nmax, __shfl_xor(nmax, 32));
    nmax = __builtin_amdgcn_readfirstlane(nmax);
    const char *fac = (const char *)T.fac[0];
    const uint32_t rowb = (uint32_t)D * 8u, eoff = (uint32_t)(jok ? ec : 0) * 8u;
    const double mean = T.mean;
    for (int c0 = 0; c0 < nmax; c0 += 16) {
        const int o = c0 + j;
        uint32_t idw = 0;
        double r = 0.0;
        if (o < n) {
            if (CODED) {
                const uint32_t pw = T.packed[it.q_begin + o];
                idw = pw & 0xffffffu;
                r = T.table[pw >> 24] - mean;
            } else {
                idw = (uint32_t)T.colidx[it.q_begin + o];
                r = T.vals[it.q_begin + o] - mean;
            }
        }
        const int left = nmax - c0;                       // (wave-uniform: the longest of the four rows)
        double v0[8];
        small_gather<0, 0>(v0, idw, fac, rowb, eoff);
        if (left > 8) {
            double v1[8];
            small_gather<1, 0>(v1, idw, fac, rowb, eoff);
            small_chunk<DR, 0, 0>(A, b, v0, r, n - c0, jok);
            small_chunk<DR, 1, 0>(A, b, v1, r, n - c0, jok);
        } else small_chunk<DR, 0, 0>(A, b, v0, r, n - c0, jok);
    }
    // prior: the image of the index-reversed Lambda is in k_rows' accumulator layout -- element (i, j) of a one-block system
    // sits at [(i / 4) * 64 + (i % 4) * 16 + j]; read past the caches when the draw was polled for (as k_rows does)
    const double alpha = term_alpha(T);
    if (a.ready) {
        int spins = 0;
        while ((int32_t)(__hip_atomic_load(a.ready, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - a.ready_want) < 0) {
            __builtin_amdgcn_s_sleep(16);
            if (++spins > (1 << 22)) { if (lane == 0) atomicOr_system(a.flag, 16); break; }
        }
#pragma unroll
        for (int i = 0; i < DR; i++)
            A[i] = fma(alpha, A[i], __hip_atomic_load(a.prior_c + (i / 4) * 64 + (i % 4) * 16 + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        b = fma(alpha, b, jok ? __hip_atomic_load(a.prior_b + ec, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0);
    } else {
#pragma unroll
        for (int i = 0; i < DR; i++) A[i] = fma(alpha, A[i], a.prior_c[(i / 4) * 64 + (i % 4) * 16 + j]);
        b = fma(alpha, b, (jok && live) ? a.prior_b[(a.mu_is_matrix ? (int64_t)it.row * D : 0) + ec] : 0.0);
    }
#pragma unroll
    for (int i = 0; i < DR; i++)
        if (i >= D || !jok) A[i] = (i == j) ? 1.0 : 0.0;          // padding: identity
    if (!jok) b = 0.0;
    double dj = 1.0;
    small_factor<DR, 0>(A, b, dj, j);
    if (live && jok && !(dj > 0.0)) atomicOr_system(a.flag, 1);
    const double rdj = fast_rcp(dj);
    double y = fma(z, fast_rsqrt(dj), b * rdj);
    small_backward<DR - 1>(A, y, rdj, j);
    if (live && jok) a.out[(int64_t)it.row * D + ec] = y;
}

}  // namespace

int bdf_small_launch(bdf_ctx *ctx, const SampleArgs &a, const RowItem *items, int64_t n_items, hipEvent_t e0, hipEvent_t e1)
{
    const dim3 grid((unsigned)((n_items + 15) / 16)), block(256);
    const bool coded = a.t[0].packed != nullptr;
#define SMALL_LAUNCH(DRV)                                                                                                        \
    do {                                                                                                                         \
        if (coded) hipExtLaunchKernelGGL((k_rows_small<true, DRV>), grid, block, 0, ctx->stream, e0, e1, 0, a, items, n_items);  \
        else hipExtLaunchKernelGGL((k_rows_small<false, DRV>), grid, block, 0, ctx->stream, e0, e1, 0, a, items, n_items);       \
    } while (0)
    if (a.D <= 4) SMALL_LAUNCH(4); else if (a.D <= 8) SMALL_LAUNCH(8); else if (a.D <= 12) SMALL_LAUNCH(12); else SMALL_LAUNCH(16);
#undef SMALL_LAUNCH
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}
