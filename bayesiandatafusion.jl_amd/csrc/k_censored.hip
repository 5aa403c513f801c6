// k_censored.hip -- the censored (Tobit) noise model: an observation flagged +1 says "the value is at least
// y", one flagged -1 "at most y", one flagged 0 is the measurement.  Given the rows the latent of a flagged observation is
// z ~ N(udot + mean_value, 1 / alpha) truncated to its side of y.
//
// bdf_censored_draw: the gather and dot product of k_probit_draw (pair_gather.h) and, in the lane that owns the pair, one uniform
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
#include <algorithm>
#include <cmath>

namespace {

struct CensArgs {
    int D;
    int64_t n;
    const int32_t *ids;            // n_modes planes of n, 0-based
    const double *fac[BDF_MAX_MODES];
    const double *values;
    const int32_t *orig;           // nullable: the pairs are stored sorted; orig[pair] = the caller's index
    const int8_t *censor;          // the caller's order: 0 measurement, +1 at least, -1 at most
    double mean, alpha;
    const double *alpha_dev;       // nullable: wins over alpha
    uint64_t seed;
    uint32_t sweep, entity;        // entity = 0x800000 | rel_tag
    double *linear, *z;            // z nullable
};

// (Registers: as k_probit_draw -- the gather's BATCH x NM x NC double4 beside the owner's erfc / inverse-CDF polynomials; the
// same bounds hold it free of scratch: DESIGN.md section 13 has the listing.)
template <int NM, int VEC, int NC>
__global__ __launch_bounds__(256, (VEC == 4 && NM * NC >= 8) ? 2 : 3) void k_censored_draw(CensArgs a)
{
    const int tid = threadIdx.x, sub = tid & 7;
    const double alpha = a.alpha_dev ? *a.alpha_dev : a.alpha;
    const int64_t ngroups = (int64_t)gridDim.x * 32, ntrips = (a.n + 7) / 8;
    for (int64_t trip = (int64_t)blockIdx.x * 32 + tid / 8; trip < ntrips; trip += ngroups) {
        const int64_t p0 = trip * 8, p = p0 + sub;
        const bool ok = p < a.n;
        const int64_t pm = ok ? p : a.n - 1;
        const int64_t po = a.orig ? (int64_t)a.orig[pm] : pm;
        const double y = a.values[pm];
        const int c = ok ? (int)a.censor[po] : 0;
        int32_t my[NM];
#pragma unroll
        for (int k = 0; k < NM; k++) my[k] = a.ids[(int64_t)k * a.n + pm];
        // the flags of the group's 8 pairs: its 8 lanes are 8 neighbours of one wave, so the test is the same in all of them
        const unsigned flagged = (unsigned)(__ballot(c != 0) >> (tid & 56)) & 0xffu;
        double dot = 0.0;
        if (flagged) dot = group_dots<NM, VEC, NC>(a.fac, a.D, a.n, p0, sub, my);
        if (!ok) continue;
        double z = y;
        if (c != 0) {
            // the observation's own uniform: the stream is keyed by the caller's index, not by where the pair is stored
            const double u = bdf_uniform(a.seed, a.sweep, BDF_P_CENSORED, a.entity, (uint64_t)po, 0);
            z = bdf_censored_z(dot + a.mean, y, c, alpha, u);
        }
        a.linear[po] = a.mean + (y - z);
        if (a.z) a.z[po] = z;
    }
}

}  // namespace

extern "C" int bdf_censored_draw(bdf_ctx *ctx, const bdf_pairs *train, const int8_t *censor_dev, int D, const double *const *factors,
                                 double mean_value, double alpha, const double *alpha_dev, uint32_t rel_tag, double *linear_out, double *z_out)
{
    BDF_REQUIRE(ctx && train && censor_dev && factors && linear_out, BDF_ERR_ARG, "bdf_censored_draw: NULL argument");
    BDF_REQUIRE(D >= 1 && D <= BDF_MAX_D, BDF_ERR_ARG, "bdf_censored_draw: num_latent=%d must be in 1..%d", D, BDF_MAX_D);
    BDF_REQUIRE(alpha_dev || (alpha > 0.0 && std::isfinite(alpha)), BDF_ERR_ARG, "bdf_censored_draw: alpha=%g must be positive and finite", alpha);
    CensArgs a;
    memset(&a, 0, sizeof(a));
    a.D = D; a.n = train->n; a.ids = train->ids_dev; a.values = train->values_dev; a.orig = train->orig_dev; a.censor = censor_dev;
    for (int k = 0; k < train->n_modes; k++) {
        BDF_REQUIRE(factors[k] != nullptr, BDF_ERR_ARG, "bdf_censored_draw: factors[%d] is NULL", k);
        a.fac[k] = factors[k];
    }
    a.mean = mean_value; a.alpha = alpha; a.alpha_dev = alpha_dev;
    a.seed = ctx->seed; a.sweep = ctx->sweep_host; a.entity = 0x800000u | rel_tag;
    a.linear = linear_out; a.z = z_out;
    if (a.n == 0) return BDF_OK;
    const int64_t ntrips = (a.n + 7) / 8;
    const int nblocks = (int)std::min<int64_t>((ntrips + 31) / 32, 8192);
    BDF_BY_SHAPE(k_censored_draw, train->n_modes, D, nblocks, ctx->stream, a);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}
