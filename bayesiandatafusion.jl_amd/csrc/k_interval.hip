// k_interval.hip -- the interval-censored noise model: observation k carries bounds lo_k <= hi_k, either of
// which may be infinite; lo_k < hi_k says "the value lies somewhere in [lo_k, hi_k]" (a rating's bin, an assay's range), lo_k ==
// hi_k that the stored value is the measurement.  Given the rows the latent of a bounded observation is
// z ~ N(udot + mean_value, 1 / alpha) truncated to [lo_k, hi_k].
//
// bdf_interval_draw: the lane prologue, gather and dot product of pair_gather.h and, in the lane that owns the pair, one uniform
// of the observation's own stream mapped to the doubly truncated normal (interval.h).  It writes linear[k] = mean_value +
// (y_k - z_k): the row kernels form y - base with the per-observation base = linear_values[k] and so see z - mean_value, with the
// relation's alpha, unchanged; bdf_predict_sse over pairs that carry `linear` as their baseline gives the residual of z that
// sample_alpha needs.  For a measurement linear[k] is mean_value, bit for bit.  alpha is read on the device when it was sampled
// there.  The owning lane fetches its (lo, hi) with one 16-byte load.
//
// A group of 8 lanes whose 8 pairs are all measurements gathers nothing: what it writes does not depend on the rows.
// No LDS, no scratch, plain vector stores.
#include "bdf_common.h"
#include "interval.h"
#include "pair_gather.h"

namespace {

struct IntvArgs {
    PairArgs pair;
    const double2 *bounds;         // the caller's order: (lo, hi) per observation, lo == hi a measurement
    uint64_t seed;
    uint32_t sweep, entity;        // pair_entity(rel_tag)
    double *linear, *z;            // z nullable
};

// One group of 8 lanes per 8 pairs and no grid-stride loop: around a loop the compiler keeps the ~70 double constants of the three
// erfc and the inverse-CDF polynomials in VGPRs across the gather's BATCH x NM x NC double4 and spills (up to 164 bytes per lane
// under these launch bounds); without one it forms them where they are used.  DESIGN.md section 14 has the listing.
template <int NM, int VEC, int NC>
__global__ __launch_bounds__(256, (VEC == 4 && NM * NC >= 8) ? 2 : 3) void k_interval_draw(IntvArgs a)
{
    const double alpha = pair_alpha(a.pair);
    const int64_t trip = pair_trip();
    if (trip * 8 < a.pair.n) {
        PairLane<NM> l;
        pair_lane(a.pair, trip, l);
        const double y = a.pair.values[l.pm];
        const double2 bd = a.bounds[l.po];
        const bool open = l.ok && bd.x != bd.y;
        double dot = 0.0;
        if (group_any(open)) dot = pair_dot<NM, VEC, NC>(a.pair, l);
        if (!l.ok) return;
        double z = y;
        if (open) {
            // the observation's own uniform: the stream is keyed by the caller's index, not by where the pair is stored
            const double u = bdf_uniform(a.seed, a.sweep, BDF_P_INTERVAL, a.entity, (uint64_t)l.po, 0);
            z = bdf_interval_z(dot + a.pair.mean, y, bd.x, bd.y, alpha, u);
        }
        latent_store(a.linear, a.z, l.po, a.pair.mean, y, z);
    }
}

}  // namespace

extern "C" int bdf_interval_draw(bdf_ctx *ctx, const bdf_pairs *train, const double *bounds_dev, int D, const double *const *factors,
                                 double mean_value, double alpha, const double *alpha_dev, uint32_t rel_tag, double *linear_out, double *z_out)
{
    BDF_REQUIRE(bounds_dev && linear_out, BDF_ERR_ARG, "bdf_interval_draw: NULL argument");
    BDF_REQUIRE(((uintptr_t)bounds_dev & 15) == 0, BDF_ERR_ARG, "bdf_interval_draw: bounds_dev must be aligned to 16 bytes");
    IntvArgs a = {};
    int rc = pair_fill("bdf_interval_draw", ctx, train, D, factors, mean_value, true, alpha, alpha_dev, a.pair);
    if (rc) return rc;
    a.bounds = (const double2 *)bounds_dev;
    a.seed = ctx->seed; a.sweep = ctx->sweep_host; a.entity = pair_entity(rel_tag);
    a.linear = linear_out; a.z = z_out;
    if (train->n == 0) return BDF_OK;
    int nblocks;
    if ((rc = pair_blocks("bdf_interval_draw", "observations", train->n, &nblocks))) return rc;
    BDF_BY_SHAPE(k_interval_draw, train->n_modes, D, nblocks, ctx->stream, a);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}
