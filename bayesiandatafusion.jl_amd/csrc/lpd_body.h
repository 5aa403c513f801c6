// lpd_body.h -- the launch arguments and the body of the kernel behind bdf_pairs_lpd_update, shared by its two units: k_lpd.hip
// instantiates it as it always was (k_lpd), k_lpd_scaled.hip with a precision scale per row of one mode (k_lpd_scaled: the per-row
// noise model).  SCALED is a template parameter, and the scaled kernels a unit of their own, so that k_lpd
// and its unit's resource listing stay exactly what they were.  File-local in both units.
#pragma once
#include "bdf_common.h"
#include "predict.h"
#include "pair_gather.h"

namespace {

struct LpdArgs {
    RecordArgs rec;
    double log_draws;              // phase 2: log of the draws the state holds after this one
    double *M, *A;                 // the running state, storage order
    const double *scale;           // k_lpd_scaled: a precision scale per row of mode scale_mode (the per-row noise model's tau)
    int scale_mode;
};

// No grid-stride loop, as k_interval_draw and for its reason: around a loop the constants of the two erfc, of exp, log, log1p and
// expm1 stay in VGPRs across the gather's BATCH x NM x NC double4.  Every lane reaches the statistics' barrier.
template <int NM, int VEC, int NC, bool SCALED>
__device__ __forceinline__ void lpd_body(const LpdArgs &a)
{
    double st[4] = {0.0, 0.0, 0.0, 0.0};
    int64_t pm;
    double l;
    if (record_loglik<NM, VEC, NC, SCALED>(a.rec, pm, l, a.scale, a.scale_mode)) {
        double lpd = l;
        if (a.rec.phase == 1) { a.M[pm] = l; a.A[pm] = 1.0; }
        else if (a.rec.phase == 2) {
            const double M = a.M[pm], Mn = fmax(M, l);
            const double A = a.A[pm] * exp(M - Mn) + exp(l - Mn);
            a.M[pm] = Mn; a.A[pm] = A;
            lpd = Mn + log(A) - a.log_draws;
        }
        st[0] = l; st[1] = lpd;
    }
    block_stats(a.rec.partial, st);
}

}  // namespace

// k_lpd_scaled.hip: the update's launch for pairs with a scale.  args: the LpdArgs that bdf_pairs_lpd_update filled (the type is
// file-local in either unit, with this one text behind it), copied before it is changed.
int bdf_lpd_launch_scaled(bdf_ctx *ctx, int n_modes, int D, int nblocks, const void *args, size_t args_bytes, double *stats_out);
