// k_lpd.hip -- the held-out log pointwise predictive density: for every test cell t the log-likelihood
// l_t = log p(y_t | the rows of this draw, alpha) of its kind of record, and over the posterior draws
// lpd_t = log((1 / S) sum_s exp(l_t,s)), the score that puts the Gaussian, probit, censored and interval noise models on one footing.
//
// bdf_pairs_lpd_update: the gather and dot product of k_interval_draw (pair_gather.h) and, in the lane that owns the pair, the
// record's log-likelihood (lpd.h): the probit map when the pairs carry the probit link, the interval's mass where the pair's bounds
// differ, the Gaussian density at the stored value otherwise.  The owning lane fetches its (lo, hi) with one 16-byte load.  The
// running state is a streaming log-sum-exp, two doubles per pair in storage order: M the largest l so far and A = sum exp(l - M).
// The two sums over the pairs -- of l and of lpd -- go through the per-workgroup statistics and the fixed-order sum of predict.h.
//
// bdf_pairs_lpd: lpd_t = M + log A - log(draws) in the caller's order.
//
// No LDS beyond the statistics' reduction, no scratch, plain vector stores.
#include "bdf_common.h"
#include "lpd.h"
#include "predict.h"
#include "pair_gather.h"
#include <cmath>

namespace {

struct LpdArgs {
    int D;
    int64_t n;
    const int32_t *ids;            // n_modes planes of n, 0-based
    const double *fac[BDF_MAX_MODES];
    const double *values;
    const int32_t *orig;           // nullable: the pairs are stored sorted; orig[pair] = the caller's index (bounds, baseline)
    const double *baseline;        // nullable: per-pair baseline instead of mean (the caller's order)
    const double2 *bounds;         // nullable; the caller's order: (lo, hi) per pair, lo == hi a measurement
    double mean, alpha;
    const double *alpha_dev;       // nullable: wins over alpha
    int link, phase;
    double log_draws;              // phase 2: log of the draws the state holds after this one
    double *M, *A;                 // the running state, storage order
    double *partial;               // per-block statistics
};

// One group of 8 lanes per 8 pairs and no grid-stride loop, as k_interval_draw and for its reason: around a loop the constants of
// the two erfc, of exp, log, log1p and expm1 stay in VGPRs across the gather's BATCH x NM x NC double4.  Every lane reaches the
// statistics' barrier.
template <int NM, int VEC, int NC>
__global__ __launch_bounds__(256, (VEC == 4 && NM * NC >= 8) ? 2 : 3) void k_lpd(LpdArgs a)
{
    const int tid = threadIdx.x, sub = tid & 7;
    const double alpha = a.alpha_dev ? *a.alpha_dev : a.alpha;
    const int64_t p0 = ((int64_t)blockIdx.x * 32 + tid / 8) * 8, p = p0 + sub;
    double st[4] = {0.0, 0.0, 0.0, 0.0};
    if (p0 < a.n) {
        const bool ok = p < a.n;
        const int64_t pm = ok ? p : a.n - 1;
        const int64_t po = a.orig ? (int64_t)a.orig[pm] : pm;
        const double y = a.values[pm];
        const double base = a.baseline ? a.baseline[po] : a.mean;
        double lo = y, hi = y;
        if (a.bounds) { const double2 bd = a.bounds[po]; lo = bd.x; hi = bd.y; }
        int32_t my[NM];
#pragma unroll
        for (int k = 0; k < NM; k++) my[k] = a.ids[(int64_t)k * a.n + pm];
        const double m = group_dots<NM, VEC, NC>(a.fac, a.D, a.n, p0, sub, my) + base;
        if (ok) {
            double l;
            if (a.link == 1) l = bdf_lpd_probit(y, m);
            else if (lo != hi) l = bdf_lpd_mass(m, lo, hi, alpha);
            else l = bdf_lpd_gauss(y, m, alpha);
            double lpd = l;
            if (a.phase == 1) { a.M[pm] = l; a.A[pm] = 1.0; }
            else if (a.phase == 2) {
                const double M = a.M[pm], Mn = fmax(M, l);
                const double A = a.A[pm] * exp(M - Mn) + exp(l - Mn);
                a.M[pm] = Mn; a.A[pm] = A;
                lpd = Mn + log(A) - a.log_draws;
            }
            st[0] = l; st[1] = lpd;
        }
    }
    PredArgs red;                      // (block_stats reads nothing of it but where the workgroup's four sums go)
    red.partial = a.partial;
    block_stats(red, st);
}

struct LpdReadArgs {
    int64_t n;
    const int32_t *orig;
    const double *M, *A;
    double log_draws;
    double *out;
};

__global__ __launch_bounds__(256) void k_lpd_read(LpdReadArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < a.n) a.out[a.orig ? (int64_t)a.orig[i] : i] = a.M[i] + log(a.A[i]) - a.log_draws;
}

}  // namespace

extern "C" int bdf_pairs_lpd_update(bdf_ctx *ctx, bdf_pairs *p, const double *bounds_dev, int D, const double *const *factors,
                                    double mean_value, double alpha, const double *alpha_dev, int phase, double *stats_out)
{
    BDF_REQUIRE(ctx && p && factors && stats_out, BDF_ERR_ARG, "bdf_pairs_lpd_update: NULL argument");
    BDF_REQUIRE(!(bounds_dev && p->link == 1), BDF_ERR_ARG, "bdf_pairs_lpd_update: pairs with the probit link take no bounds");
    BDF_REQUIRE(((uintptr_t)bounds_dev & 15) == 0, BDF_ERR_ARG, "bdf_pairs_lpd_update: bounds_dev must be aligned to 16 bytes");
    BDF_REQUIRE(D >= 1 && D <= BDF_MAX_D, BDF_ERR_ARG, "bdf_pairs_lpd_update: num_latent=%d must be in 1..%d", D, BDF_MAX_D);
    BDF_REQUIRE(phase >= 0 && phase <= 2, BDF_ERR_ARG, "bdf_pairs_lpd_update: phase must be 0, 1 or 2");
    BDF_REQUIRE(alpha_dev || (alpha > 0.0 && std::isfinite(alpha)), BDF_ERR_ARG, "bdf_pairs_lpd_update: alpha=%g must be positive and finite", alpha);
    BDF_REQUIRE(phase != 2 || p->lpd_draws >= 1.0, BDF_ERR_ARG, "bdf_pairs_lpd_update: phase 2 before a phase 1: the pairs hold no draw");
    LpdArgs a;
    memset(&a, 0, sizeof(a));
    a.D = D; a.n = p->n; a.ids = p->ids_dev; a.values = p->values_dev; a.orig = p->orig_dev; a.baseline = p->baseline_dev;
    a.bounds = (const double2 *)bounds_dev;
    for (int k = 0; k < p->n_modes; k++) {
        BDF_REQUIRE(factors[k] != nullptr, BDF_ERR_ARG, "bdf_pairs_lpd_update: factors[%d] is NULL", k);
        a.fac[k] = factors[k];
    }
    a.mean = mean_value; a.alpha = alpha; a.alpha_dev = alpha_dev; a.link = p->link; a.phase = phase;
    const int64_t ntrips = (a.n + 7) / 8;
    BDF_REQUIRE((ntrips + 31) / 32 <= INT32_MAX, BDF_ERR_ARG, "bdf_pairs_lpd_update: %lld pairs are more than one launch covers", (long long)a.n);
    const int nblocks = (int)((ntrips + 31) / 32);
    BDF_HIP(hipSetDevice(ctx->device));
    if (a.n == 0) {
        BDF_HIP(hipMemsetAsync(stats_out, 0, 4 * sizeof(double), ctx->stream));
    } else {
        if (phase >= 1 && !p->lpd_dev) {
            BDF_HIP(hipMalloc((void **)&p->lpd_dev, (size_t)a.n * 2 * sizeof(double)));
            BDF_HIP(hipMemsetAsync(p->lpd_dev, 0, (size_t)a.n * 2 * sizeof(double), ctx->stream));
        }
        a.M = p->lpd_dev; a.A = p->lpd_dev ? p->lpd_dev + a.n : nullptr;
        a.log_draws = phase == 2 ? log(p->lpd_draws + 1.0) : 0.0;
        void *sc;
        int rc = bdf_scratch(ctx, (size_t)nblocks * 4 * sizeof(double), &sc);
        if (rc) return rc;
        a.partial = (double *)sc;
        BDF_BY_SHAPE(k_lpd, p->n_modes, D, nblocks, ctx->stream, a);
        hipLaunchKernelGGL(k_predict_final, dim3(1), dim3(256), 0, ctx->stream, nblocks, (const double *)a.partial, stats_out);
        BDF_HIP(hipGetLastError());
    }
    if (phase == 1) p->lpd_draws = 1.0;
    else if (phase == 2) p->lpd_draws += 1.0;
    return BDF_OK;
}

extern "C" int bdf_pairs_lpd(bdf_ctx *ctx, const bdf_pairs *p, double *out_dev)
{
    BDF_REQUIRE(ctx && p && out_dev, BDF_ERR_ARG, "bdf_pairs_lpd: NULL argument");
    BDF_REQUIRE(p->lpd_draws >= 1.0, BDF_ERR_ARG, "bdf_pairs_lpd: the pairs hold no posterior draw (bdf_pairs_lpd_update with phase 1 first)");
    if (p->n == 0) return BDF_OK;
    BDF_REQUIRE((p->n + 255) / 256 <= INT32_MAX, BDF_ERR_ARG, "bdf_pairs_lpd: %lld pairs are more than one launch covers", (long long)p->n);
    LpdReadArgs a;
    a.n = p->n; a.orig = p->orig_dev; a.M = p->lpd_dev; a.A = p->lpd_dev + p->n; a.log_draws = log(p->lpd_draws); a.out = out_dev;
    BDF_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_lpd_read, dim3((unsigned)((p->n + 255) / 256)), dim3(256), 0, ctx->stream, a);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}
