// k_update_runs.hip -- the prediction update of the sweep (bdf_predict_update on pairs stored sorted by one mode, two-mode relation,
// D a multiple of 4 up to 32, no raw predictions, no per-pair baseline) in a register budget that lets a wave of it run BESIDE two
// waves of the row kernel on a SIMD: 2 x 208 (k_rows_col.hip) + 96 = the lane's 512.  The update's waves spend their lives waiting
// for gathers; what they cost the row launch they run under is the register space they hold meanwhile, and
// k_predict_runs' 126 registers kept the second row wave off a SIMD.
//
// The same values as k_predict_runs (k_predict.hip), bit for bit -- the per-lane products (x x + y y) + (z z + w w), the xor 4, 2, 1
// sums, pair_finish, 512 pairs per partial in block_stats' order -- from fewer registers:
//   * a pair's value and running state are loaded when the pair is finished, not before the first gather (they were held
//     across both batches of gathers: 2 pairs x (position, index, value, mean, sum of squares, baseline));
//   * orig[] is not read at all: it indexes `out` and `linear`, which this path does not have;
//   * a batch of gathers is the other mode's rows of FOUR pairs (32 registers), not eight.
//
// Single-wave workgroups.  Launched as 256 lanes, a workgroup is placed only where all four SIMDs of a CU have the update's registers
// free at the same moment; beside 2 x 208 that is a CU whose four SIMDs are each between row waves or short of one.  Nothing in the
// update needs four waves together -- the barrier and the LDS were block_stats' cross-wave sum alone -- so the kernel is launched as
// four times as many workgroups of 64 lanes, which take any one SIMD's free registers.  Workgroup w takes the pairs that wave w & 3
// of workgroup w >> 2 took: every lane keeps its pairs, its gathers and its keep[].  A wave leaves its four sums (block_stats'
// butterfly, xor 32 .. 1) in partial[4 w ..], no LDS and no barrier; k_update_waves_final adds the four waves of a former workgroup
// left to right -- block_stats' last line -- and goes on as k_predict_final does, expression for expression.  The statistics keep
// their bits.  The narrower launch bound would let the compiler take more registers: UPD_VGPR_HALF holds it to the 96 the row
// kernel leaves.
#include "bdf_common.h"
#include "predict.h"

namespace {

constexpr int RUN = 16;            // pairs per group of 8 lanes: a lane owns pairs p0 + sub and p0 + 8 + sub (k_predict_runs' shape)
constexpr int NB = 4;              // pairs per batch of gathers
// (amdgpu_num_vgpr counts in halves of the unified file, as for k_rows_col: 48 stands for 96 = 512 - 2 x 208)
#define UPD_VGPR_HALF 48

__global__ __launch_bounds__(64) __attribute__((amdgpu_num_vgpr(UPD_VGPR_HALF))) void k_update_runs(PredArgs a)
{
    const int tid = threadIdx.x, sub = tid & 7;            // (a workgroup is one wave)
    const int ks = a.sorted_mode, ko = 1 - ks;
    const int32_t *ids_s = a.ids + (int64_t)ks * a.n, *ids_o = a.ids + (int64_t)ko * a.n;
    const double *fs = a.fac[ks], *fo = a.fac[ko];
    const bool live = sub * 4 < a.D;                      // lanes beyond D / 4 hold zeros
    const int eoff = live ? sub * 4 : 0;
    const int64_t p0 = ((int64_t)blockIdx.x * 8 + tid / 8) * RUN;
    int32_t cur = -1;
    double4 srow = {0.0, 0.0, 0.0, 0.0};
    double keep[2] = {0.0, 0.0};
#pragma unroll
    for (int q = 0; q < 2; q++) {
        if (p0 + 8 * q >= a.n) break;                      // group-uniform
        const int64_t pm = p0 + 8 * q + sub < a.n ? p0 + 8 * q + sub : a.n - 1;
        const int32_t my_s = ids_s[pm], my_o = ids_o[pm];
#pragma unroll
        for (int u0 = 0; u0 < 8; u0 += NB) {
            double4 orow[NB];
#pragma unroll
            for (int u = 0; u < NB; u++) orow[u] = *(const double4 *)(fo + (int64_t)__shfl(my_o, u0 + u, 8) * a.D + eoff);
#pragma unroll
            for (int u = 0; u < NB; u++) {
                const int32_t is = __shfl(my_s, u0 + u, 8);
                if (is != cur) { srow = *(const double4 *)(fs + (int64_t)is * a.D + eoff); cur = is; }
                double s = live ? (srow.x * orow[u].x + srow.y * orow[u].y) + (srow.z * orow[u].z + srow.w * orow[u].w) : 0.0;
                s += __shfl_xor(s, 4); s += __shfl_xor(s, 2); s += __shfl_xor(s, 1);
                if (sub == u0 + u) keep[q] = s;
            }
        }
    }
    __builtin_amdgcn_sched_barrier(0);                     // (the pairs' state is not to be loaded ahead of the gathers)
    double st[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < 2; q++) {
        PairState ps;
        const int64_t p = p0 + 8 * q + sub;
        ps.ok = p < a.n;
        ps.pm = ps.ok ? p : a.n - 1;
        ps.po = ps.pm;                                     // (out and linear are NULL here: nothing is indexed by the caller's order)
        ps.base = a.mean;
        ps.y = a.values[ps.pm];
        ps.av = 0.0; ps.sv = 0.0;
        if (a.phase == 2) { ps.av = a.avg[ps.pm]; ps.sv = a.sq[ps.pm]; }
        pair_finish(a, ps, keep[q], st);
    }
    // the wave's four sums, block_stats' butterfly: every lane ends with the same bits, lane 0 stores them
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) st[q] += __shfl_xor(st[q], off);
    if (tid == 0) {
        double *w = a.partial + (int64_t)blockIdx.x * 4;
        w[0] = st[0]; w[1] = st[1]; w[2] = st[2]; w[3] = st[3];
    }
}

// fixed-order sum of the per-wave statistics: the partial of former workgroup b is its four waves left to right (block_stats' last
// line), then k_predict_final's stride over b, butterfly and red[q][0] + .. + red[q][3]
__global__ __launch_bounds__(256) void k_update_waves_final(int nblocks, const double *wave, double *stats)
{
    __shared__ double red[4][4];
    const int tid = threadIdx.x;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int b = tid; b < nblocks; b += 256) {
        const double *w = wave + (int64_t)b * 16;
#pragma unroll
        for (int q = 0; q < 4; q++) v[q] += w[q] + w[4 + q] + w[8 + q] + w[12 + q];
    }
#pragma unroll
    for (int q = 0; q < 4; q++) {
        double x = v[q];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off);
        if ((tid & 63) == 0) red[q][tid >> 6] = x;
    }
    __syncthreads();
    if (tid < 4) stats[tid] = red[tid][0] + red[tid][1] + red[tid][2] + red[tid][3];
}

}  // namespace

// bdf_predict_update's launch for such pairs (k_predict.hip decides): phase 0 .. 2, `count` the pairs' counter before it
int bdf_update_runs(bdf_ctx *ctx, const bdf_pairs *p, int D, const double *const *factors, double mean_value, int phase, double count,
                    double clamp_lo, double clamp_hi, double class_cut, double *stats_out)
{
    PredArgs a;
    int rc = fill("bdf_predict_update", ctx, p, D, factors, a);
    if (rc) return rc;
    BDF_REQUIRE(a.sorted_mode >= 0 && a.n_modes == 2 && (D & 3) == 0 && D <= 32 && a.linear == nullptr && phase >= 0 && phase <= 2,
                BDF_ERR_ARG, "bdf_update_runs: not the sorted two-mode update");
    if (a.n == 0) return BDF_OK;
    a.mean = mean_value; a.avg = p->avg_dev; a.sq = p->sq_dev; a.phase = phase; a.count = count;
    a.clamp_lo = clamp_lo; a.clamp_hi = clamp_hi; a.cut = class_cut; a.stats = stats_out;
    a.orig = nullptr; a.out = nullptr;
    // 512 pairs per partial as before, left by four workgroups of one wave each: 4 x nblocks x 4 doubles of scratch
    const int nblocks = (int)((a.n + 32 * RUN - 1) / (32 * RUN));
    void *sc;
    rc = bdf_scratch(ctx, (size_t)nblocks * 16 * sizeof(double), &sc);
    if (rc) return rc;
    a.partial = (double *)sc;
    hipLaunchKernelGGL(k_update_runs, dim3(4 * (unsigned)nblocks), dim3(64), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_update_waves_final, dim3(1), dim3(256), 0, ctx->stream, nblocks, (const double *)a.partial, a.stats);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}
