// k_pg.hip -- the Polya-Gamma noise models: a logit link for 0/1 relations and negative-binomial counts with a
// fixed dispersion r.  With psi = udot + mean_value, omega ~ PG(b, psi) makes the cell a Gaussian pseudo-observation kappa / omega of
// psi with precision omega (pg.h has b and kappa of the two models).
//
// bdf_pg_draw: the lane prologue, gather and dot product of pair_gather.h and, in the lane that owns the pair, the draw of pg.h on
// the observation's own stream (BDF_P_PG, row = the caller's index): one cursor over the stream's blocks pair = 0, 1, 2, ..., so
// that what a cell draws depends neither on where it is stored nor on the launch.  It writes omega and mean + y - kappa / omega in
// the caller's order: bdf_term.obs_precision and bdf_term.linear_values of the unchanged weighted row kernel (k_rows_w), alpha = 1.
//
// The logistic and the count link of the prediction kernels (bdf_pairs_set_logistic_link, bdf_pairs_set_count_link), in kernels of this
// unit, so that the instantiations of k_predict.hip and k_probit.hip stay as they are.
//
// One group of 8 lanes per 8 pairs and no grid-stride loop; the gather's registers are dead before the draw starts.  Lanes diverge
// on b = y + r: a wave costs its largest b.  No LDS in the draw, no scratch, plain vector stores, no atomics.
#include "bdf_common.h"
#include "predict_link.h"
#include "pg.h"
#include <algorithm>

namespace {

struct PgArgs {
    PairArgs pair;                 // (no alpha: the pseudo-observation's precision is omega)
    int model;                     // 1 logit, 2 counts
    double r;
    uint64_t seed;
    uint32_t sweep, entity;        // pair_entity(rel_tag)
    double *precision, *linear;    // the caller's order
};

// the cursor of pg.h over the observation's stream: every request takes the next block (the stream's pair index is 16 bits wide:
// it wraps after 65,536 blocks, a hundred times what 170 variates take)
struct PgCursor {
    uint64_t seed, row;
    uint32_t sweep, entity, pair;
    __device__ __forceinline__ u32x4 block() { return bdf_draw(seed, sweep, BDF_P_PG, entity, row, (pair++) & 0xffffu); }
    __device__ __forceinline__ double uniform() { const u32x4 o = block(); return bdf_u01(o.x, o.y); }
    __device__ __forceinline__ double expo() { return -bdf_log01(uniform()); }
    __device__ __forceinline__ void expo2(double &E, double &F)
    {
        const u32x4 o = block();
        E = -bdf_log01(bdf_u01(o.x, o.y));
        F = -bdf_log01(bdf_u01(o.z, o.w));
    }
    __device__ __forceinline__ double normal() { return bdf_normal(seed, sweep, BDF_P_PG, entity, row, (int)(2u * ((pair++) & 0xffffu))); }
};

// (Registers: k_robust_draw's bounds -- the gather's BATCH x NM x NC double4 are dead when the owner's Philox / erfc / exp
// arithmetic starts; DESIGN.md section 19 has the listing.)
template <int NM, int VEC, int NC>
__global__ __launch_bounds__(256, (VEC == 4 && NM * NC >= 8) ? 2 : 3) void k_pg_draw(PgArgs a)
{
    const int64_t trip = pair_trip();
    if (trip * 8 >= a.pair.n) return;              // (group-uniform)
    PairLane<NM> l;
    pair_lane(a.pair, trip, l);
    const double y = a.pair.values[l.pm];
    const double psi = pair_dot<NM, VEC, NC>(a.pair, l) + a.pair.mean;
    if (!l.ok) return;
    // the observation's own stream: keyed by the caller's index, not by where the pair is stored
    PgCursor rng = {a.seed, (uint64_t)l.po, a.sweep, a.entity, 0u};
    const double w = bdf_pg_omega(bdf_pg_b(a.model, y, a.r), psi, rng);
    a.precision[l.po] = w;
    a.linear[l.po] = bdf_pg_linear(a.pair.mean, y, bdf_pg_kappa(a.model, y, a.r), w);
}

// k_predict_link of k_probit.hip with the logistic (LINK 2) and the count link (LINK 3)
template <int NM, int VEC, int NC>
__global__ __launch_bounds__(256) void k_predict_logit(PredArgs a)
{
    predict_link_body<NM, VEC, NC, 2>(a);
}

template <int NM, int VEC, int NC>
__global__ __launch_bounds__(256) void k_predict_count(PredArgs a)
{
    predict_link_body<NM, VEC, NC, 3>(a);
}

}  // namespace

// bdf_predict_link (k_probit.hip) for pairs with link 2 or 3
int bdf_predict_link_pg(bdf_ctx *ctx, const bdf_pairs *p, int D, const double *const *factors, double mean_value, const double *linear,
                        double *out, int phase, double count, double clamp_lo, double clamp_hi, double class_cut, double *stats_out)
{
    const bool logit = p && p->link == 2;
    return predict_link_launch(logit ? "bdf_predict (logistic link)" : "bdf_predict (count link)", ctx, p, D, factors, mean_value, linear, out,
                               phase, count, clamp_lo, clamp_hi, class_cut, stats_out, [&](const PredArgs &a, int nblocks) {
                                   if (logit) BDF_BY_SHAPE(k_predict_logit, a.n_modes, D, nblocks, ctx->stream, a);
                                   else BDF_BY_SHAPE(k_predict_count, a.n_modes, D, nblocks, ctx->stream, a);
                               });
}

extern "C" int bdf_pg_draw(bdf_ctx *ctx, const bdf_pairs *train, int D, const double *const *factors, double mean_value, int model, double r,
                           uint32_t rel_tag, double *precision_out, double *linear_out)
{
    BDF_REQUIRE(precision_out && linear_out, BDF_ERR_ARG, "bdf_pg_draw: NULL argument");
    BDF_REQUIRE(model == 1 || model == 2, BDF_ERR_ARG, "bdf_pg_draw: model=%d must be 1 (logit) or 2 (counts)", model);
    BDF_REQUIRE(model != 2 || (r >= 1.0 && r <= 2147483648.0 && r == std::floor(r)), BDF_ERR_ARG,
                "bdf_pg_draw: r=%g must be an integer, at least 1 (and at most 2^31)", r);
    PgArgs a = {};
    int rc = pair_fill("bdf_pg_draw", ctx, train, D, factors, mean_value, false, 0.0, nullptr, a.pair);
    if (rc) return rc;
    BDF_REQUIRE(std::isfinite(mean_value), BDF_ERR_ARG, "bdf_pg_draw: mean_value must be finite");
    a.model = model; a.r = model == 2 ? r : 0.0;
    a.seed = ctx->seed; a.sweep = ctx->sweep_host; a.entity = pair_entity(rel_tag);
    a.precision = precision_out; a.linear = linear_out;
    int nblocks;
    if ((rc = pair_blocks("bdf_pg_draw", "observations", train->n, &nblocks))) return rc;
    if (nblocks == 0) return BDF_OK;
    BDF_HIP(hipSetDevice(ctx->device));
    BDF_BY_SHAPE(k_pg_draw, train->n_modes, D, nblocks, ctx->stream, a);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}
