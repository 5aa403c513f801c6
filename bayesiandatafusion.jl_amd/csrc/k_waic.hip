// k_waic.hip -- the widely applicable information criterion on the training cells: for every training cell t
// and the S posterior draws the log-likelihood l_t,s of its kind of record (lpd.h), folded into
//   lppd_t = log((1 / S) sum_s exp(l_t,s))   and   V_t = the sample variance of l_t,s over the draws (divisor S - 1),
// from which elpd_t = lppd_t - V_t, WAIC = -2 sum_t elpd_t and its standard error.  Nothing is kept per draw.
//
// bdf_pairs_waic_update: in the lane that owns the pair the record's log-likelihood by its kind, as k_lpd takes it (record_loglik of
// pair_gather.h), and a running state of four doubles per pair in storage order, four planes of n: the streaming log-sum-exp
// (M, A) exactly as k_lpd keeps it, and Welford's (mean, M2) of l (waic.h).  The four sums over the pairs -- of l, of lppd, of V and
// the count of V > 0.4 -- go through the per-workgroup statistics and the fixed-order sum of predict.h.
//
// bdf_pairs_waic: (lppd_t, V_t) in the caller's order, and in two fixed-order passes sum lppd, sum V, then sum (elpd_t - mean elpd)^2
// about the mean the first pass gave: the standard error is never the difference of two sums of squares.
//
// No LDS beyond the statistics' reduction, no scratch, plain vector stores.
#include "bdf_common.h"
#include "waic.h"
#include "predict.h"
#include "pair_gather.h"

namespace {

struct WaicArgs {
    RecordArgs rec;                // (its baseline is NULL whenever bounds are given)
    double draws, log_draws;       // phase 2: the draws the state holds after this one, and their logarithm
    double *M, *A, *mu, *M2;       // the running state, storage order
};

// No grid-stride loop, as k_lpd and for its reason.  The state is read only after the
// record's log-likelihood is formed, so that its four doubles are not live across the gather and the maps.  Every lane reaches
// the statistics' barrier.
template <int NM, int VEC, int NC>
__global__ __launch_bounds__(256, (VEC == 4 && NM * NC >= 8) ? 2 : 3) void k_waic(WaicArgs a)
{
    double st[4] = {0.0, 0.0, 0.0, 0.0};
    int64_t pm;
    double l;
    if (record_loglik<NM, VEC, NC>(a.rec, pm, l)) {
        double lppd = l, V = 0.0;
        if (a.rec.phase >= 1) {
            bdf_waic_cell c;
            if (a.rec.phase == 1) bdf_waic_start(l, c);
            else {
                c.M = a.M[pm]; c.A = a.A[pm]; c.mu = a.mu[pm]; c.M2 = a.M2[pm];
                bdf_waic_fold(l, a.draws, a.log_draws, c, lppd, V);
            }
            a.M[pm] = c.M; a.A[pm] = c.A; a.mu[pm] = c.mu; a.M2[pm] = c.M2;
        }
        st[0] = l; st[1] = lppd; st[2] = V; st[3] = V > BDF_WAIC_HIGH ? 1.0 : 0.0;
    }
    block_stats(a.rec.partial, st);
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
    block_stats(a.partial, st);
}

}  // namespace

extern "C" int bdf_pairs_waic_update(bdf_ctx *ctx, bdf_pairs *p, const double *bounds_dev, int D, const double *const *factors,
                                     double mean_value, double alpha, const double *alpha_dev, int phase, double *stats_out)
{
    WaicArgs a = {};
    int nblocks;
    // Training pairs that are scored with bounds belong to a censored, interval or ordinal relation, whose baseline is the latent
    // draw's (mean + y - z: what the row kernels read), not a mean: with bounds m = udot + mean_value, as bdf_ordinal_step takes it
    int rc = record_fill("bdf_pairs_waic_update", ctx, p, bounds_dev, (bounds_dev || !p) ? nullptr : p->baseline_dev, D, factors, mean_value, alpha,
                         alpha_dev, phase, stats_out, a.rec, &nblocks);
    if (rc) return rc;
    BDF_REQUIRE(phase != 2 || p->waic_draws >= 1.0, BDF_ERR_ARG, "bdf_pairs_waic_update: phase 2 before a phase 1: the pairs hold no draw");
    BDF_REQUIRE(!p->scale_dev, BDF_ERR_ARG, "bdf_pairs_waic_update: pairs with a precision scale (bdf_pairs_set_precision_scale) are not scored yet");
    const int64_t n = p->n;
    BDF_HIP(hipSetDevice(ctx->device));
    if (n == 0) {
        BDF_HIP(hipMemsetAsync(stats_out, 0, 4 * sizeof(double), ctx->stream));
    } else {
        if (phase >= 1 && !p->waic_dev) {
            if (int rc = p->waic_dev.alloc((size_t)n * 4)) return rc;
            BDF_HIP(hipMemsetAsync(p->waic_dev, 0, (size_t)n * 4 * sizeof(double), ctx->stream));
        }
        if (p->waic_dev) { a.M = p->waic_dev; a.A = a.M + n; a.mu = a.A + n; a.M2 = a.mu + n; }
        a.draws = phase == 2 ? p->waic_draws + 1.0 : 1.0;
        a.log_draws = log(a.draws);
        if ((rc = launch_reduced(ctx, nblocks, a.rec.partial, stats_out, [&] { BDF_BY_SHAPE(k_waic, p->n_modes, D, nblocks, ctx->stream, a); }))) return rc;
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
    // first pass: sum lppd and sum V into stats_out; second pass: the squares about the mean elpd those two give (read from
    // stats_out before the fixed-order sum behind it on the stream overwrites it), and the pointwise table
    const auto pass = [&] { hipLaunchKernelGGL(k_waic_read, dim3(nblocks), dim3(256), 0, ctx->stream, a); };
    a.first = nullptr; a.out = nullptr;
    int rc = launch_reduced(ctx, nblocks, a.partial, stats_out, pass);
    if (rc) return rc;
    a.first = stats_out; a.out = out_dev;
    return launch_reduced(ctx, nblocks, a.partial, stats_out, pass);
}
