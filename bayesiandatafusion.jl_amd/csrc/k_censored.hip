// k_censored.hip -- the censored (Tobit) noise model: an observation flagged +1 says "the value is at least
// y", one flagged -1 "at most y", one flagged 0 is the measurement.  Given the rows the latent of a flagged observation is
// z ~ N(udot + mean_value, 1 / alpha) truncated to its side of y.
//
// bdf_censored_draw: the lane prologue, gather and dot product of pair_gather.h and, in the lane that owns the pair, one uniform
// of the observation's own stream mapped to the truncated normal (censored.h).  It writes linear[k] = mean_value + (y_k - z_k):
// the row kernels form y - base with the per-observation base = linear_values[k] and so see z - mean_value, with the relation's
// alpha, unchanged; bdf_predict_sse over pairs that carry `linear` as their baseline gives the residual of z that sample_alpha
// needs.  For a measurement linear[k] is mean_value, bit for bit.  alpha is read on the device when it was sampled there.
//
// A group of 8 lanes whose 8 pairs are all measurements gathers nothing: what it writes does not depend on the rows.
// No LDS, no scratch, plain vector stores.
#include "bdf_common.h"
#include "censored.h"
#include "pair_gather.h"

namespace {

struct CensArgs {
    PairArgs pair;
    const int8_t *censor;          // the caller's order: 0 measurement, +1 at least, -1 at most
    uint64_t seed;
    uint32_t sweep, entity;        // pair_entity(rel_tag)
    double *linear, *z;            // z nullable
};

// (Registers: as k_probit_draw -- the gather's BATCH x NM x NC double4 beside the owner's erfc / inverse-CDF polynomials; the
// same bounds hold it free of scratch: DESIGN.md section 13 has the listing.)
template <int NM, int VEC, int NC>
__global__ __launch_bounds__(256, (VEC == 4 && NM * NC >= 8) ? 2 : 3) void k_censored_draw(CensArgs a)
{
    const double alpha = pair_alpha(a.pair);
    const int64_t ngroups = (int64_t)gridDim.x * 32, ntrips = (a.pair.n + 7) / 8;
    for (int64_t trip = pair_trip(); trip < ntrips; trip += ngroups) {
        PairLane<NM> l;
        pair_lane(a.pair, trip, l);
        const double y = a.pair.values[l.pm];
        const int c = l.ok ? (int)a.censor[l.po] : 0;
        double dot = 0.0;
        if (group_any(c != 0)) dot = pair_dot<NM, VEC, NC>(a.pair, l);
        if (!l.ok) continue;
        double z = y;
        if (c != 0) {
            // the observation's own uniform: the stream is keyed by the caller's index, not by where the pair is stored
            const double u = bdf_uniform(a.seed, a.sweep, BDF_P_CENSORED, a.entity, (uint64_t)l.po, 0);
            z = bdf_censored_z(dot + a.pair.mean, y, c, alpha, u);
        }
        latent_store(a.linear, a.z, l.po, a.pair.mean, y, z);
    }
}

}  // namespace

extern "C" int bdf_censored_draw(bdf_ctx *ctx, const bdf_pairs *train, const int8_t *censor_dev, int D, const double *const *factors,
                                 double mean_value, double alpha, const double *alpha_dev, uint32_t rel_tag, double *linear_out, double *z_out)
{
    BDF_REQUIRE(censor_dev && linear_out, BDF_ERR_ARG, "bdf_censored_draw: NULL argument");
    CensArgs a = {};
    int rc = pair_fill("bdf_censored_draw", ctx, train, D, factors, mean_value, true, alpha, alpha_dev, a.pair);
    if (rc) return rc;
    a.censor = censor_dev;
    a.seed = ctx->seed; a.sweep = ctx->sweep_host; a.entity = pair_entity(rel_tag);
    a.linear = linear_out; a.z = z_out;
    if (train->n == 0) return BDF_OK;
    BDF_BY_SHAPE(k_censored_draw, train->n_modes, D, pair_blocks_strided(train->n), ctx->stream, a);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}
