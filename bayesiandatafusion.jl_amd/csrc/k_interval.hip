// k_interval.hip -- the interval-censored noise model: observation k carries bounds lo_k <= hi_k, either of
// which may be infinite; lo_k < hi_k says "the value lies somewhere in [lo_k, hi_k]" (a rating's bin, an assay's range), lo_k ==
// hi_k that the stored value is the measurement.  Given the rows the latent of a bounded observation is
// z ~ N(udot + mean_value, 1 / alpha) truncated to [lo_k, hi_k].
//
// bdf_interval_draw: the gather and dot product of k_censored_draw (pair_gather.h) and, in the lane that owns the pair, one uniform
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
#include <cmath>

namespace {

struct IntvArgs {
    int D;
    int64_t n;
    const int32_t *ids;            // n_modes planes of n, 0-based
    const double *fac[BDF_MAX_MODES];
    const double *values;
    const int32_t *orig;           // nullable: the pairs are stored sorted; orig[pair] = the caller's index
    const double2 *bounds;         // the caller's order: (lo, hi) per observation, lo == hi a measurement
    double mean, alpha;
    const double *alpha_dev;       // nullable: wins over alpha
    uint64_t seed;
    uint32_t sweep, entity;        // entity = 0x800000 | rel_tag
    double *linear, *z;            // z nullable
};

// One group of 8 lanes per 8 pairs and no grid-stride loop: around a loop the compiler keeps the ~70 double constants of the three
// erfc and the inverse-CDF polynomials in VGPRs across the gather's BATCH x NM x NC double4 and spills (up to 164 bytes per lane
// under these launch bounds); without one it forms them where they are used.  DESIGN.md section 14 has the listing.
template <int NM, int VEC, int NC>
__global__ __launch_bounds__(256, (VEC == 4 && NM * NC >= 8) ? 2 : 3) void k_interval_draw(IntvArgs a)
{
    const int tid = threadIdx.x, sub = tid & 7;
    const double alpha = a.alpha_dev ? *a.alpha_dev : a.alpha;
    const int64_t p0 = ((int64_t)blockIdx.x * 32 + tid / 8) * 8, p = p0 + sub;
    if (p0 < a.n) {
        const bool ok = p < a.n;
        const int64_t pm = ok ? p : a.n - 1;
        const int64_t po = a.orig ? (int64_t)a.orig[pm] : pm;
        const double y = a.values[pm];
        const double2 bd = a.bounds[po];
        const bool open = ok && bd.x != bd.y;
        int32_t my[NM];
#pragma unroll
        for (int k = 0; k < NM; k++) my[k] = a.ids[(int64_t)k * a.n + pm];
        // the bounded ones of the group's 8 pairs: its 8 lanes are 8 neighbours of one wave, so the test is the same in all of them
        const unsigned bounded = (unsigned)(__ballot(open) >> (tid & 56)) & 0xffu;
        double dot = 0.0;
        if (bounded) dot = group_dots<NM, VEC, NC>(a.fac, a.D, a.n, p0, sub, my);
        if (!ok) return;
        double z = y;
        if (open) {
            // the observation's own uniform: the stream is keyed by the caller's index, not by where the pair is stored
            const double u = bdf_uniform(a.seed, a.sweep, BDF_P_INTERVAL, a.entity, (uint64_t)po, 0);
            z = bdf_interval_z(dot + a.mean, y, bd.x, bd.y, alpha, u);
        }
        a.linear[po] = a.mean + (y - z);
        if (a.z) a.z[po] = z;
    }
}

}  // namespace

extern "C" int bdf_interval_draw(bdf_ctx *ctx, const bdf_pairs *train, const double *bounds_dev, int D, const double *const *factors,
                                 double mean_value, double alpha, const double *alpha_dev, uint32_t rel_tag, double *linear_out, double *z_out)
{
    BDF_REQUIRE(ctx && train && bounds_dev && factors && linear_out, BDF_ERR_ARG, "bdf_interval_draw: NULL argument");
    BDF_REQUIRE(((uintptr_t)bounds_dev & 15) == 0, BDF_ERR_ARG, "bdf_interval_draw: bounds_dev must be aligned to 16 bytes");
    BDF_REQUIRE(D >= 1 && D <= BDF_MAX_D, BDF_ERR_ARG, "bdf_interval_draw: num_latent=%d must be in 1..%d", D, BDF_MAX_D);
    BDF_REQUIRE(alpha_dev || (alpha > 0.0 && std::isfinite(alpha)), BDF_ERR_ARG, "bdf_interval_draw: alpha=%g must be positive and finite", alpha);
    IntvArgs a;
    memset(&a, 0, sizeof(a));
    a.D = D; a.n = train->n; a.ids = train->ids_dev; a.values = train->values_dev; a.orig = train->orig_dev;
    a.bounds = (const double2 *)bounds_dev;
    for (int k = 0; k < train->n_modes; k++) {
        BDF_REQUIRE(factors[k] != nullptr, BDF_ERR_ARG, "bdf_interval_draw: factors[%d] is NULL", k);
        a.fac[k] = factors[k];
    }
    a.mean = mean_value; a.alpha = alpha; a.alpha_dev = alpha_dev;
    a.seed = ctx->seed; a.sweep = ctx->sweep_host; a.entity = 0x800000u | rel_tag;
    a.linear = linear_out; a.z = z_out;
    if (a.n == 0) return BDF_OK;
    const int64_t ntrips = (a.n + 7) / 8;
    BDF_REQUIRE((ntrips + 31) / 32 <= INT32_MAX, BDF_ERR_ARG, "bdf_interval_draw: %lld observations are more than one launch covers", (long long)a.n);
    const int nblocks = (int)((ntrips + 31) / 32);
    BDF_BY_SHAPE(k_interval_draw, train->n_modes, D, nblocks, ctx->stream, a);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}
