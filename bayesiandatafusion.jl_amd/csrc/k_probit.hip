// k_probit.hip -- the probit noise model for 0/1 relations: y = 1[z > 0], z ~ N(udot + mean_value, 1).
//
// bdf_probit_draw: the latent z of every training observation given the current factors -- the lane prologue, gather and dot
// product of pair_gather.h and, in the lane that owns the pair, one uniform of the observation's own stream mapped to the
// truncated normal (probit.h).  It writes linear[k] = y_k - z_k: the row kernels, which form b_i = Lambda mu_i + alpha sum w (y - base) with
// the per-observation base = linear_values[k], then sample the rows of z's Gaussian model with alpha = 1, unchanged.
//
// The probit link of the prediction kernels (bdf_pairs_set_link): p = Phi(udot + base) in place of udot + base, in kernels of
// this unit, so that the instantiations of k_predict.hip stay as they are.
//
// Layout as k_predict.hip: 8 lanes share a pair and read 32 bytes each; ids and values are loaded 8 consecutive pairs per
// group before the first gather; BATCH pairs' rows are in flight.  No LDS in the draw, no scratch, plain vector stores.
#include "bdf_common.h"
#include "predict_link.h"
#include <algorithm>

namespace {

struct DrawArgs {
    PairArgs pair;                 // (no alpha: the latent's variance is 1)
    uint64_t seed;
    uint32_t sweep, entity;        // pair_entity(rel_tag)
    double *linear, *z;            // z nullable
};

// (Registers: the gather holds BATCH x NM x NC double4 and the owner's erfc / inverse-CDF polynomials want ~60 more; bounded to
// three waves per SIMD -- 168 registers, no scratch -- except the widest gather, which k_predict.hip also runs at two.  At four
// waves the 3- and 4-mode variants spill.)
template <int NM, int VEC, int NC>
__global__ __launch_bounds__(256, (VEC == 4 && NM * NC >= 8) ? 2 : 3) void k_probit_draw(DrawArgs a)
{
    const int64_t ngroups = (int64_t)gridDim.x * 32, ntrips = (a.pair.n + 7) / 8;
    for (int64_t trip = pair_trip(); trip < ntrips; trip += ngroups) {
        PairLane<NM> l;
        pair_lane(a.pair, trip, l);
        const double y = a.pair.values[l.pm];
        const double dot = pair_dot<NM, VEC, NC>(a.pair, l);
        if (!l.ok) continue;
        // the observation's own uniform: the stream is keyed by the caller's index, not by where the pair is stored
        const double u = bdf_uniform(a.seed, a.sweep, BDF_P_PROBIT, a.entity, (uint64_t)l.po, 0);
        const double z = bdf_probit_z(dot + a.pair.mean, y, u);
        a.linear[l.po] = y - z;
        if (a.z) a.z[l.po] = z;
    }
}

// k_predict<NM, VEC, NC> of k_predict.hip with the probit link in what the owning lane does (pair_finish<1>).  (Unbounded: with
// the running state and the four statistics live beside erfc, any bound above two waves per SIMD spills the VEC = 4 variants.)
template <int NM, int VEC, int NC>
__global__ __launch_bounds__(256) void k_predict_link(PredArgs a)
{
    predict_link_body<NM, VEC, NC, 1>(a);
}

}  // namespace

int bdf_predict_link(bdf_ctx *ctx, const bdf_pairs *p, int D, const double *const *factors, double mean_value, const double *linear,
                     double *out, int phase, double count, double clamp_lo, double clamp_hi, double class_cut, double *stats_out)
{
    if (p && p->link >= 2) return bdf_predict_link_pg(ctx, p, D, factors, mean_value, linear, out, phase, count, clamp_lo, clamp_hi, class_cut, stats_out);
    return predict_link_launch("bdf_predict (probit link)", ctx, p, D, factors, mean_value, linear, out, phase, count, clamp_lo, clamp_hi,
                               class_cut, stats_out,
                               [&](const PredArgs &a, int nblocks) { BDF_BY_SHAPE(k_predict_link, a.n_modes, D, nblocks, ctx->stream, a); });
}

extern "C" int bdf_probit_draw(bdf_ctx *ctx, const bdf_pairs *train, int D, const double *const *factors, double mean_value,
                               uint32_t rel_tag, double *linear_out, double *z_out)
{
    BDF_REQUIRE(linear_out, BDF_ERR_ARG, "bdf_probit_draw: NULL argument");
    DrawArgs a = {};
    int rc = pair_fill("bdf_probit_draw", ctx, train, D, factors, mean_value, false, 0.0, nullptr, a.pair);
    if (rc) return rc;
    a.seed = ctx->seed; a.sweep = ctx->sweep_host; a.entity = pair_entity(rel_tag);
    a.linear = linear_out; a.z = z_out;
    if (train->n == 0) return BDF_OK;
    BDF_BY_SHAPE(k_probit_draw, train->n_modes, D, pair_blocks_strided(train->n), ctx->stream, a);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}
