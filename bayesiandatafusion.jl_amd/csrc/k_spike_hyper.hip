// k_spike_hyper.hip -- the hyper step of the spike-and-slab prior (spike.h), the running sums of its
// result, and diag(tau) as the matrix the row launch's prior image is built from.
//
//   n_d = #{i : u_id != 0},  q_d = sum_i u_id^2
//   G1 ~ Gamma(incl_a + n_d),  G2 ~ Gamma(incl_b + N - n_d),  G3 ~ Gamma(shape + n_d / 2)
//   pi_d = G1 / (G1 + G2),  logit pi_d = log G1 - log G2,  tau_d = G3 / (rate + q_d / 2)
//
// Two launches: k_spike_partial, one workgroup per BDF_SPIKE_ROWS_PER_BLOCK rows -- thread d walks its component down the block's
// rows, so a partial is a sum in row order whatever the grid --, then k_spike_draw, one workgroup: thread d adds the partials in
// block order and draws.  Nothing goes to the host.
#include "spike.h"

namespace {

__global__ __launch_bounds__(64) void k_spike_partial(int D, int64_t N, const double *__restrict__ sample, double *__restrict__ part)
{
    const int d = threadIdx.x;
    if (d >= D) return;
    const int64_t r0 = (int64_t)blockIdx.x * BDF_SPIKE_ROWS_PER_BLOCK;
    const int64_t r1 = r0 + BDF_SPIKE_ROWS_PER_BLOCK < N ? r0 + BDF_SPIKE_ROWS_PER_BLOCK : N;
    double n = 0.0, q = 0.0;
    for (int64_t i = r0; i < r1; i++) {
        const double u = sample[i * D + d];
        n += (u != 0.0) ? 1.0 : 0.0;
        q = fma(u, u, q);
    }
    part[((int64_t)blockIdx.x * 2) * D + d] = n;
    part[((int64_t)blockIdx.x * 2 + 1) * D + d] = q;
}

__global__ __launch_bounds__(64) void k_spike_draw(int D, int64_t N, int64_t nblocks, const double *__restrict__ part, double incl_a,
                                                   double incl_b, double shape, double rate, uint64_t seed, uint32_t sweep,
                                                   uint32_t entity_tag, double *__restrict__ state)
{
    const int d = threadIdx.x;
    if (d >= D) return;
    double n = 0.0, q = 0.0;
    for (int64_t b = 0; b < nblocks; b++) {
        n += part[(b * 2) * D + d];
        q += part[(b * 2 + 1) * D + d];
    }
    const double g1 = bdf_gamma_on(BDF_P_SPIKE_N, BDF_P_SPIKE_U, seed, sweep, entity_tag, (uint64_t)(3 * d), incl_a + n);
    const double g2 = bdf_gamma_on(BDF_P_SPIKE_N, BDF_P_SPIKE_U, seed, sweep, entity_tag, (uint64_t)(3 * d + 1), incl_b + ((double)N - n));
    const double g3 = bdf_gamma_on(BDF_P_SPIKE_N, BDF_P_SPIKE_U, seed, sweep, entity_tag, (uint64_t)(3 * d + 2), shape + 0.5 * n);
    const double tau = g3 / (rate + 0.5 * q);
    state[BDF_SPIKE_PI(D, d)] = g1 / (g1 + g2);
    state[BDF_SPIKE_TAU(D, d)] = tau;
    state[BDF_SPIKE_LOGIT(D, d)] = log(g1) - log(g2);       // never formed from pi: no clipping
    state[BDF_SPIKE_LOGTAU(D, d)] = log(tau);
}

// row_sum += [u != 0]; the draw's counts into hyper_sum[2 D + d] (integers: exact whatever the order of the atomics); workgroup 0
// adds pi and tau
__global__ __launch_bounds__(64) void k_spike_accumulate(int D, int64_t N, const double *__restrict__ sample, const double *__restrict__ state,
                                                         double *__restrict__ row_sum, double *__restrict__ hyper_sum)
{
    const int d = threadIdx.x;
    if (d >= D) return;
    const int64_t r0 = (int64_t)blockIdx.x * BDF_SPIKE_ROWS_PER_BLOCK;
    const int64_t r1 = r0 + BDF_SPIKE_ROWS_PER_BLOCK < N ? r0 + BDF_SPIKE_ROWS_PER_BLOCK : N;
    double n = 0.0;
    for (int64_t i = r0; i < r1; i++) {
        const double s = (sample[i * D + d] != 0.0) ? 1.0 : 0.0;
        row_sum[i * D + d] += s;
        n += s;
    }
    atomicAdd(hyper_sum + 2 * D + d, n);
    if (blockIdx.x == 0) {
        hyper_sum[d] += state[BDF_SPIKE_PI(D, d)];
        hyper_sum[D + d] += state[BDF_SPIKE_TAU(D, d)];
    }
}

__global__ __launch_bounds__(256) void k_spike_lambda(int D, const double *__restrict__ state, double *__restrict__ out)
{
    for (int t = threadIdx.x; t < D * D + D; t += blockDim.x) {
        double v = 0.0;
        if (t < D * D && t / D == t % D) v = state[BDF_SPIKE_TAU(D, t / D)];
        out[t] = v;
    }
}

bool ok_param(double x, double lo) { return x >= lo && x < __builtin_inf(); }

}  // namespace

int bdf_spike_lambda_launch(bdf_ctx *ctx, int D, const double *spike_state, double *Lambda_mu_out)
{
    hipLaunchKernelGGL(k_spike_lambda, dim3(1), dim3(256), 0, ctx->stream, D, spike_state, Lambda_mu_out);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}

extern "C" int bdf_spike_hyper(bdf_ctx *ctx, int D, int64_t N, const double *sample, double incl_a, double incl_b, double shape, double rate,
                               uint32_t entity_tag, double *spike_state)
{
    BDF_REQUIRE(ctx && sample && spike_state, BDF_ERR_ARG, "bdf_spike_hyper: NULL argument");
    BDF_REQUIRE(D >= 1 && D <= BDF_MAX_D, BDF_ERR_ARG, "bdf_spike_hyper: num_latent=%d must be in 1..%d", D, BDF_MAX_D);
    BDF_REQUIRE(N >= 1, BDF_ERR_ARG, "bdf_spike_hyper: N=%lld must be positive", (long long)N);
    BDF_REQUIRE(ok_param(incl_a, 0.5) && ok_param(incl_b, 0.5) && ok_param(shape, 0.5), BDF_ERR_ARG,
                "bdf_spike_hyper: incl_a=%g, incl_b=%g and shape=%g must be >= 0.5 and finite", incl_a, incl_b, shape);
    BDF_REQUIRE(rate > 0.0 && ok_param(rate, 0.0), BDF_ERR_ARG, "bdf_spike_hyper: rate=%g must be positive and finite", rate);
    const int64_t nblocks = (N + BDF_SPIKE_ROWS_PER_BLOCK - 1) / BDF_SPIKE_ROWS_PER_BLOCK;
    BDF_REQUIRE(nblocks <= BDF_SPIKE_MAX_BLOCKS, BDF_ERR_ARG, "bdf_spike_hyper: N=%lld is more rows than one grid takes", (long long)N);
    void *part;
    int rc = bdf_scratch(ctx, (size_t)nblocks * 2 * (size_t)D * sizeof(double), &part);
    if (rc) return rc;
    hipLaunchKernelGGL(k_spike_partial, dim3((unsigned)nblocks), dim3(64), 0, ctx->stream, D, N, sample, (double *)part);
    BDF_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_spike_draw, dim3(1), dim3(64), 0, ctx->stream, D, N, nblocks, (const double *)part, incl_a, incl_b, shape, rate,
                       ctx->seed, ctx->sweep_host, entity_tag, spike_state);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}

extern "C" int bdf_spike_accumulate(bdf_ctx *ctx, int D, int64_t N, const double *sample, const double *spike_state, double *row_sum,
                                    double *hyper_sum)
{
    BDF_REQUIRE(ctx && sample && spike_state && row_sum && hyper_sum, BDF_ERR_ARG, "bdf_spike_accumulate: NULL argument");
    BDF_REQUIRE(D >= 1 && D <= BDF_MAX_D, BDF_ERR_ARG, "bdf_spike_accumulate: num_latent=%d must be in 1..%d", D, BDF_MAX_D);
    BDF_REQUIRE(N >= 1, BDF_ERR_ARG, "bdf_spike_accumulate: N=%lld must be positive", (long long)N);
    const int64_t nblocks = (N + BDF_SPIKE_ROWS_PER_BLOCK - 1) / BDF_SPIKE_ROWS_PER_BLOCK;
    BDF_REQUIRE(nblocks <= BDF_SPIKE_MAX_BLOCKS, BDF_ERR_ARG, "bdf_spike_accumulate: N=%lld is more rows than one grid takes", (long long)N);
    hipLaunchKernelGGL(k_spike_accumulate, dim3((unsigned)nblocks), dim3(64), 0, ctx->stream, D, N, sample, spike_state, row_sum, hyper_sum);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}
