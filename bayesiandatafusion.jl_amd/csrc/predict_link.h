// predict_link.h -- what the prediction kernels with a link share (the probit link of k_probit.hip, the logistic and the count
// link of k_pg.hip): the kernel's body, with the link a template parameter of what the owning lane does (pair_finish<LINK>), and
// the host side around the launch.  Every link's kernels are instantiated in the link's own unit.  File-local in every unit
// that includes it.
#pragma once
#include "predict.h"
#include "pair_gather.h"

namespace {

// k_predict<NM, VEC, NC> of k_predict.hip with pair_finish<LINK> in what the owning lane does
template <int NM, int VEC, int NC, int LINK>
__device__ __forceinline__ void predict_link_body(const PredArgs &a)
{
    const int tid = threadIdx.x, sub = tid & 7;
    double st[4] = {0.0, 0.0, 0.0, 0.0};
    const int64_t ngroups = (int64_t)gridDim.x * 32, ntrips = (a.n + 7) / 8;
    for (int64_t trip = (int64_t)blockIdx.x * 32 + tid / 8; trip < ntrips; trip += ngroups) {
        const int64_t p0 = trip * 8;
        PairState ps;
        pair_load(a, p0 + sub, ps);
        int32_t my[NM];
#pragma unroll
        for (int k = 0; k < NM; k++) my[k] = a.ids[(int64_t)k * a.n + ps.pm];
        const double keep = group_dots<NM, VEC, NC>(a.fac, a.D, a.n, p0, sub, my);
        pair_finish<LINK>(a, ps, keep, st);
    }
    if (a.phase >= 0) block_stats(a, st);
}

// the arguments, the geometry and, for phase >= 0, the statistics' scratch and fixed-order sum; launch(a, nblocks) starts the
// link's kernel for the shape
template <class Launch>
int predict_link_launch(const char *who, bdf_ctx *ctx, const bdf_pairs *p, int D, const double *const *factors, double mean_value,
                        const double *linear, double *out, int phase, double count, double clamp_lo, double clamp_hi, double class_cut,
                        double *stats_out, Launch launch)
{
    PredArgs a;
    int rc = fill(who, ctx, p, D, factors, a);
    if (rc) return rc;
    a.mean = mean_value; a.out = out; a.phase = phase; a.count = count; a.link_r = p->link_r;
    if (linear) a.linear = linear;
    if (phase >= 0) {
        a.avg = p->avg_dev; a.sq = p->sq_dev; a.clamp_lo = clamp_lo; a.clamp_hi = clamp_hi; a.cut = class_cut; a.stats = stats_out;
    }
    if (a.n == 0) return BDF_OK;
    const int nblocks = pair_blocks_strided(a.n);
    if (phase >= 0) return launch_reduced(ctx, nblocks, a.partial, a.stats, [&] { launch(a, nblocks); });
    launch(a, nblocks);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}

}  // namespace
