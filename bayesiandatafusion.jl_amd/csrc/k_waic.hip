// k_waic.hip -- the widely applicable information criterion on the training cells: for every training cell t
// and the S posterior draws the log-likelihood l_t,s of its kind of record (lpd.h), folded into
//   lppd_t = log((1 / S) sum_s exp(l_t,s))   and   V_t = the sample variance of l_t,s over the draws (divisor S - 1),
// from which elpd_t = lppd_t - V_t, WAIC = -2 sum_t elpd_t and its standard error.  Nothing is kept per draw.
//
// bdf_pairs_waic_update: k_lpd's gather, dot product and choice of the record's kind in the owning lane (k_lpd.hip), and a running
// state of four doubles per pair in storage order, four planes of n: the streaming log-sum-exp (M, A) exactly as k_lpd keeps it,
// and Welford's (mean, M2) of l (waic.h).  The four sums over the pairs -- of l, of lppd, of V and the count of V > 0.4 -- go through the
// per-workgroup statistics and the fixed-order sum of predict.h.
//
// bdf_pairs_waic: (lppd_t, V_t) in the caller's order, and in two fixed-order passes sum lppd, sum V, then sum (elpd_t - mean elpd)^2
// about the mean the first pass gave: the standard error is never the difference of two sums of squares.
//
// No LDS beyond the statistics' reduction, no scratch, plain vector stores.
#include "bdf_common.h"
#include "waic.h"
#include "predict.h"
#include "pair_gather.h"
#include <cmath>

namespace {

struct WaicArgs {
    int D;
    int64_t n;
    const int32_t *ids;            // n_modes planes of n, 0-based
    const double *fac[BDF_MAX_MODES];
    const double *values;
    const int32_t *orig;           // nullable: the pairs are stored sorted; orig[pair] = the caller's index (bounds, baseline)
    const double *baseline;        // nullable: per-pair baseline instead of mean (the caller's order); NULL whenever bounds are given
    const double2 *bounds;         // nullable; the caller's order: (lo, hi) per pair, lo == hi a measurement
    double mean, alpha;
    const double *alpha_dev;       // nullable: wins over alpha
    int link, phase;
    double draws, log_draws;       // phase 2: the draws the state holds after this one, and their logarithm
    double *M, *A, *mu, *M2;       // the running state, storage order
    double *partial;               // per-block statistics
};

// One group of 8 lanes per 8 pairs and no grid-stride loop, as k_lpd and for its reason.  The state is read only after the
// record's log-likelihood is formed, so that its four doubles are not live across the gather and the maps.  Every lane reaches
// the statistics' barrier.
template <int NM, int VEC, int NC>
__global__ __launch_bounds__(256, (VEC == 4 && NM * NC >= 8) ? 2 : 3) void k_waic(WaicArgs a)
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
            double lppd = l, V = 0.0;
            if (a.phase >= 1) {
                bdf_waic_cell c;
                if (a.phase == 1) bdf_waic_start(l, c);
                else {
                    c.M = a.M[pm]; c.A = a.A[pm]; c.mu = a.mu[pm]; c.M2 = a.M2[pm];
                    bdf_waic_fold(l, a.draws, a.log_draws, c, lppd, V);
                }
                a.M[pm] = c.M; a.A[pm] = c.A; a.mu[pm] = c.mu; a.M2[pm] = c.M2;
            }
            st[0] = l; st[1] = lppd; st[2] = V; st[3] = V > BDF_WAIC_HIGH ? 1.0 : 0.0;
        }
    }
    PredArgs red;                      // (block_stats reads nothing of it but where the workgroup's four sums go)
    red.partial = a.partial;
    block_stats(red, st);
}

struct WaicReadArgs {
    int64_t n;
    const int32_t *orig;
    const double *M, *A, *M2;
    double draws, log_draws;
    const double *first;           // nullable: the first pass's sums {sum lppd, sum V, ., .}; given, [2] is (elpd - their mean)^2
    double *out;                   // nullable: (n, 2) in the caller's order
    double *partial;
};

// every lane reaches the statistics' barrier
__global__ __launch_bounds__(256) void k_waic_read(WaicReadArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double st[4] = {0.0, 0.0, 0.0, 0.0};
    if (i < a.n) {
        const double lppd = a.M[i] + log(a.A[i]) - a.log_draws;
        const double V = a.draws >= 2.0 ? a.M2[i] / (a.draws - 1.0) : 0.0;
        st[0] = lppd; st[1] = V; st[3] = V > BDF_WAIC_HIGH ? 1.0 : 0.0;
        if (a.first) {
            const double e = (lppd - V) - (a.first[0] - a.first[1]) / (double)a.n;
            st[2] = e * e;
        }
        if (a.out) {
            const int64_t o = a.orig ? (int64_t)a.orig[i] : i;
            *(double2 *)(a.out + 2 * o) = double2{lppd, V};
        }
    }
    PredArgs red;
    red.partial = a.partial;
    block_stats(red, st);
}

}  // namespace

extern "C" int bdf_pairs_waic_update(bdf_ctx *ctx, bdf_pairs *p, const double *bounds_dev, int D, const double *const *factors,
                                     double mean_value, double alpha, const double *alpha_dev, int phase, double *stats_out)
{
    BDF_REQUIRE(ctx && p && factors && stats_out, BDF_ERR_ARG, "bdf_pairs_waic_update: NULL argument");
    BDF_REQUIRE(!(bounds_dev && p->link == 1), BDF_ERR_ARG, "bdf_pairs_waic_update: pairs with the probit link take no bounds");
    BDF_REQUIRE(((uintptr_t)bounds_dev & 15) == 0, BDF_ERR_ARG, "bdf_pairs_waic_update: bounds_dev must be aligned to 16 bytes");
    BDF_REQUIRE(D >= 1 && D <= BDF_MAX_D, BDF_ERR_ARG, "bdf_pairs_waic_update: num_latent=%d must be in 1..%d", D, BDF_MAX_D);
    BDF_REQUIRE(phase >= 0 && phase <= 2, BDF_ERR_ARG, "bdf_pairs_waic_update: phase must be 0, 1 or 2");
    BDF_REQUIRE(alpha_dev || (alpha > 0.0 && std::isfinite(alpha)), BDF_ERR_ARG, "bdf_pairs_waic_update: alpha=%g must be positive and finite", alpha);
    BDF_REQUIRE(phase != 2 || p->waic_draws >= 1.0, BDF_ERR_ARG, "bdf_pairs_waic_update: phase 2 before a phase 1: the pairs hold no draw");
    WaicArgs a;
    memset(&a, 0, sizeof(a));
    a.D = D; a.n = p->n; a.ids = p->ids_dev; a.values = p->values_dev; a.orig = p->orig_dev;
    // Training pairs that are scored with bounds belong to a censored, interval or ordinal relation, whose baseline is the latent
    // draw's (mean + y - z: what the row kernels read), not a mean: with bounds m = udot + mean_value, as bdf_ordinal_step takes it
    a.baseline = bounds_dev ? nullptr : p->baseline_dev;
    a.bounds = (const double2 *)bounds_dev;
    for (int k = 0; k < p->n_modes; k++) {
        BDF_REQUIRE(factors[k] != nullptr, BDF_ERR_ARG, "bdf_pairs_waic_update: factors[%d] is NULL", k);
        a.fac[k] = factors[k];
    }
    a.mean = mean_value; a.alpha = alpha; a.alpha_dev = alpha_dev; a.link = p->link; a.phase = phase;
    const int64_t ntrips = (a.n + 7) / 8;
    BDF_REQUIRE((ntrips + 31) / 32 <= INT32_MAX, BDF_ERR_ARG, "bdf_pairs_waic_update: %lld pairs are more than one launch covers", (long long)a.n);
    const int nblocks = (int)((ntrips + 31) / 32);
    BDF_HIP(hipSetDevice(ctx->device));
    if (a.n == 0) {
        BDF_HIP(hipMemsetAsync(stats_out, 0, 4 * sizeof(double), ctx->stream));
    } else {
        if (phase >= 1 && !p->waic_dev) {
            BDF_HIP(hipMalloc((void **)&p->waic_dev, (size_t)a.n * 4 * sizeof(double)));
            BDF_HIP(hipMemsetAsync(p->waic_dev, 0, (size_t)a.n * 4 * sizeof(double), ctx->stream));
        }
        if (p->waic_dev) { a.M = p->waic_dev; a.A = a.M + a.n; a.mu = a.A + a.n; a.M2 = a.mu + a.n; }
        a.draws = phase == 2 ? p->waic_draws + 1.0 : 1.0;
        a.log_draws = log(a.draws);
        void *sc;
        int rc = bdf_scratch(ctx, (size_t)nblocks * 4 * sizeof(double), &sc);
        if (rc) return rc;
        a.partial = (double *)sc;
        BDF_BY_SHAPE(k_waic, p->n_modes, D, nblocks, ctx->stream, a);
        hipLaunchKernelGGL(k_predict_final, dim3(1), dim3(256), 0, ctx->stream, nblocks, (const double *)a.partial, stats_out);
        BDF_HIP(hipGetLastError());
    }
    if (phase == 1) p->waic_draws = 1.0;
    else if (phase == 2) p->waic_draws += 1.0;
    return BDF_OK;
}

extern "C" int bdf_pairs_waic(bdf_ctx *ctx, const bdf_pairs *p, double *out_dev, double *stats_out)
{
    BDF_REQUIRE(ctx && p && stats_out, BDF_ERR_ARG, "bdf_pairs_waic: NULL argument");
    BDF_REQUIRE(((uintptr_t)out_dev & 15) == 0, BDF_ERR_ARG, "bdf_pairs_waic: out_dev must be aligned to 16 bytes");
    BDF_REQUIRE(p->waic_draws >= 1.0, BDF_ERR_ARG, "bdf_pairs_waic: the pairs hold no posterior draw (bdf_pairs_waic_update with phase 1 first)");
    BDF_REQUIRE((p->n + 255) / 256 <= INT32_MAX, BDF_ERR_ARG, "bdf_pairs_waic: %lld pairs are more than one launch covers", (long long)p->n);
    BDF_HIP(hipSetDevice(ctx->device));
    if (p->n == 0) {
        BDF_HIP(hipMemsetAsync(stats_out, 0, 4 * sizeof(double), ctx->stream));
        return BDF_OK;
    }
    const int nblocks = (int)((p->n + 255) / 256);
    WaicReadArgs a;
    a.n = p->n; a.orig = p->orig_dev; a.M = p->waic_dev; a.A = a.M + p->n; a.M2 = a.M + 3 * p->n; a.draws = p->waic_draws; a.log_draws = log(a.draws);
    void *sc;
    int rc = bdf_scratch(ctx, (size_t)nblocks * 4 * sizeof(double), &sc);
    if (rc) return rc;
    a.partial = (double *)sc;
    // first pass: sum lppd and sum V into stats_out; second pass: the squares about the mean elpd those two give (read from
    // stats_out before the fixed-order sum behind it on the stream overwrites it), and the pointwise table
    a.first = nullptr; a.out = nullptr;
    hipLaunchKernelGGL(k_waic_read, dim3(nblocks), dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_predict_final, dim3(1), dim3(256), 0, ctx->stream, nblocks, (const double *)a.partial, stats_out);
    a.first = stats_out; a.out = out_dev;
    hipLaunchKernelGGL(k_waic_read, dim3(nblocks), dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_predict_final, dim3(1), dim3(256), 0, ctx->stream, nblocks, (const double *)a.partial, stats_out);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}
