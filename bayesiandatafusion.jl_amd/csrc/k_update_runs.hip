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
#include "bdf_common.h"
#include "predict.h"

namespace {

constexpr int RUN = 16;            // pairs per group of 8 lanes: a lane owns pairs p0 + sub and p0 + 8 + sub (k_predict_runs' shape)
constexpr int NB = 4;              // pairs per batch of gathers

__global__ __launch_bounds__(256) void k_update_runs(PredArgs a)
{
    const int tid = threadIdx.x, sub = tid & 7;
    const int ks = a.sorted_mode, ko = 1 - ks;
    const int32_t *ids_s = a.ids + (int64_t)ks * a.n, *ids_o = a.ids + (int64_t)ko * a.n;
    const double *fs = a.fac[ks], *fo = a.fac[ko];
    const bool live = sub * 4 < a.D;                      // lanes beyond D / 4 hold zeros
    const int eoff = live ? sub * 4 : 0;
    const int64_t p0 = ((int64_t)blockIdx.x * 32 + tid / 8) * RUN;
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
    block_stats(a, st);
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
    const int nblocks = (int)((a.n + 32 * RUN - 1) / (32 * RUN));
    return launch_reduced(ctx, nblocks, a.partial, a.stats,
                          [&] { hipLaunchKernelGGL(k_update_runs, dim3(nblocks), dim3(256), 0, ctx->stream, a); });
}
