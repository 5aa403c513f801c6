// k_lpd.hip -- the held-out log pointwise predictive density: for every test cell t the log-likelihood
// l_t = log p(y_t | the rows of this draw, alpha) of its kind of record, and over the posterior draws
// lpd_t = log((1 / S) sum_s exp(l_t,s)), the score that puts the Gaussian, probit, censored and interval noise models on one footing.
//
// bdf_pairs_lpd_update: in the lane that owns the pair the record's log-likelihood by its kind (record_loglik of pair_gather.h,
// bdf_lpd_record of lpd.h) behind the shared lane prologue, gather and dot product.  The running state is a streaming log-sum-exp, two doubles per pair in storage order: M the largest l so far and A = sum exp(l - M).
// The two sums over the pairs -- of l and of lpd -- go through the per-workgroup statistics and the fixed-order sum of predict.h.
//
// bdf_pairs_set_precision_scale: under the per-row noise model a cell is scored with alpha tau[its id in one
// mode]; the pairs then take k_lpd_scaled (k_lpd_scaled.hip: the same body, lpd_body.h, with SCALED set), and k_lpd is untouched.
//
// bdf_pairs_lpd: lpd_t = M + log A - log(draws) in the caller's order.
//
// No LDS beyond the statistics' reduction, no scratch, plain vector stores.
#include "lpd_body.h"

namespace {

template <int NM, int VEC, int NC>
__global__ __launch_bounds__(256, (VEC == 4 && NM * NC >= 8) ? 2 : 3) void k_lpd(LpdArgs a)
{
    lpd_body<NM, VEC, NC, false>(a);
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
    LpdArgs a = {};
    int nblocks;
    int rc = record_fill("bdf_pairs_lpd_update", ctx, p, bounds_dev, p ? p->baseline_dev : nullptr, D, factors, mean_value, alpha, alpha_dev,
                         phase, stats_out, a.rec, &nblocks);
    if (rc) return rc;
    BDF_REQUIRE(phase != 2 || p->lpd_draws >= 1.0, BDF_ERR_ARG, "bdf_pairs_lpd_update: phase 2 before a phase 1: the pairs hold no draw");
    BDF_REQUIRE(!(p->scale_dev && p->link == 1), BDF_ERR_ARG, "bdf_pairs_lpd_update: pairs with the probit link take no precision scale");
    const int64_t n = p->n;
    BDF_HIP(hipSetDevice(ctx->device));
    if (n == 0) {
        BDF_HIP(hipMemsetAsync(stats_out, 0, 4 * sizeof(double), ctx->stream));
    } else {
        if (phase >= 1 && !p->lpd_dev) {
            if (int rc = p->lpd_dev.alloc((size_t)n * 2)) return rc;
            BDF_HIP(hipMemsetAsync(p->lpd_dev, 0, (size_t)n * 2 * sizeof(double), ctx->stream));
        }
        a.M = p->lpd_dev; a.A = p->lpd_dev ? p->lpd_dev + n : nullptr;
        a.log_draws = phase == 2 ? log(p->lpd_draws + 1.0) : 0.0;
        a.scale = p->scale_dev; a.scale_mode = p->scale_mode;
        if (a.scale) rc = bdf_lpd_launch_scaled(ctx, p->n_modes, D, nblocks, &a, sizeof(a), stats_out);
        else rc = launch_reduced(ctx, nblocks, a.rec.partial, stats_out, [&] { BDF_BY_SHAPE(k_lpd, p->n_modes, D, nblocks, ctx->stream, a); });
        if (rc) return rc;
    }
    if (phase == 1) p->lpd_draws = 1.0;
    else if (phase == 2) p->lpd_draws += 1.0;
    return BDF_OK;
}

extern "C" int bdf_pairs_set_precision_scale(bdf_pairs *p, const double *tau_dev, int mode)
{
    BDF_REQUIRE(p != nullptr, BDF_ERR_ARG, "bdf_pairs_set_precision_scale: NULL argument");
    if (!tau_dev) { p->scale_dev = nullptr; p->scale_mode = 0; return BDF_OK; }
    BDF_REQUIRE(mode >= 0 && mode < p->n_modes, BDF_ERR_ARG, "bdf_pairs_set_precision_scale: mode=%d must be in 0..%d", mode, p->n_modes - 1);
    BDF_REQUIRE(p->link != 1, BDF_ERR_ARG, "bdf_pairs_set_precision_scale: pairs with the probit link take no precision scale");
    p->scale_dev = tau_dev; p->scale_mode = mode;
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
