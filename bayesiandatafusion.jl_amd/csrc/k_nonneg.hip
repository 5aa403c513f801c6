// k_nonneg.hip -- the non-negative prior of an entity's rows (nonneg.h): the coordinate sweep of the rows'
// systems, the hyper step, the running sums of the result, and diag(tau) as the matrix the row launch's prior image is built from.
//
// The rows' systems P_i = diag(tau) + sum alpha sum omega w w' and c_i are left in the context's scratch by K1's dump launch
// (rows_plan.hip), a chunk of rows at a time.  k_nonneg_sweep then gives every LANE one row: 64 rows advance through step d
// together, and every lane's evaluation of the map (an erfc, a log / sqrt, two degree-7 rationals) is a draw that is needed -- a
// wave per row, as k_rows_ss finishes its rows, would evaluate it in 64 lanes for the one that holds component d.
//   u      the wave's LDS as [k][lane]: a runtime d indexes it without private memory, and lanes read consecutive doubles
//   P      step d reads row d of the lane's own P, D contiguous doubles, by 16-byte loads where D is even: every line a lane
//          fetches is consumed within the step (the other form, the wave's 64 segments staged through a padded LDS tile, was not
//          built: DESIGN.md section 26 says what the probe showed)
//   d      a real loop: the map's code appears once; divergence is confined to its branches
// No cross-lane operation.  A lane past the chunk's end loads and stores nothing but stays in the loop.
//
// Hyper step: k_nonneg_partial, one workgroup per BDF_SPIKE_ROWS_PER_BLOCK rows -- thread d walks its component down the block's
// rows, so a partial is a sum in row order whatever the grid --, then k_nonneg_draw, one workgroup: thread d adds the partials in
// block order and draws.  Nothing goes to the host.
#include "rows.h"
#include "spike.h"
#include "nonneg.h"

#define BDF_NONNEG_SCRATCH_CAP ((size_t)1 << 30)      // bytes of systems per chunk by default

namespace {

typedef double nn_d2 __attribute__((ext_vector_type(2)));

// The map as a function of its own, not inlined: inside the d loop the compiler moves its ~120 double literals (three degree-7
// rationals, erfc, log) in front of the loop and holds them in registers across it -- 197 VGPRs and three spilled SGPRs, against
// 57 VGPRs and none with the call, which leaves the occupancy to the LDS (5 / 3 / 2 waves per SIMD at DP = 16 / 32 / 64).
__device__ __attribute__((noinline)) double nonneg_map(double m, double lambda, double U) { return bdf_nonneg(m, lambda, U); }

template <int DP>
__global__ __launch_bounds__(64) void k_nonneg_sweep(NonnegSweepArgs a)
{
    __shared__ double u[DP * 64];
    const int lane = threadIdx.x, D = a.D;
    const int64_t i = (int64_t)blockIdx.x * 64 + lane;
    const bool live = i < a.n;
    int64_t row = 0, io = 0;          // the row's random stream; its place in u_current and out
    if (live) {
        row = a.rows ? (int64_t)a.rows[a.pos0 + i * a.stride] : a.row_begin + i;
        io = a.rows ? row : i;
    }
    const double *P = a.P + i * D * D, *c = a.c + i * D;
    for (int k = 0; k < D; k++) u[k * 64 + lane] = live ? a.u_current[io * D + k] : 0.0;
    for (int d = 0; d < D; d++) {
        double lam = 1.0, dot = 0.0, cd = 0.0, U = 0.5;
        if (live) {
            const double *Pd = P + d * D;
            if (a.wide) {
                for (int k = 0; k < D; k += 2) {
                    const nn_d2 p = *reinterpret_cast<const nn_d2 *>(Pd + k);
                    dot += (k == d) ? 0.0 : p.x * u[k * 64 + lane];
                    dot += (k + 1 == d) ? 0.0 : p.y * u[(k + 1) * 64 + lane];
                    lam = (k == d) ? p.x : ((k + 1 == d) ? p.y : lam);
                }
            } else {
                for (int k = 0; k < D; k++) {
                    const double p = Pd[k];
                    dot += (k == d) ? 0.0 : p * u[k * 64 + lane];
                    lam = (k == d) ? p : lam;
                }
            }
            cd = c[d];
            U = bdf_uniform(a.seed, a.sweep, BDF_P_NONNEG, a.entity_tag, (uint64_t)row, (uint32_t)d);
            if (!(lam > 0.0 && lam < __builtin_inf())) atomicOr_system(a.flag, 1);
        }
        u[d * 64 + lane] = nonneg_map((cd - dot) / lam, lam, U);
    }
    if (live)
        for (int k = 0; k < D; k++) a.out[io * D + k] = u[k * 64 + lane];
}

__global__ __launch_bounds__(64) void k_nonneg_partial(int D, int64_t N, const double *__restrict__ sample, double *__restrict__ part)
{
    const int d = threadIdx.x;
    if (d >= D) return;
    const int64_t r0 = (int64_t)blockIdx.x * BDF_SPIKE_ROWS_PER_BLOCK;
    const int64_t r1 = r0 + BDF_SPIKE_ROWS_PER_BLOCK < N ? r0 + BDF_SPIKE_ROWS_PER_BLOCK : N;
    double q = 0.0;
    for (int64_t i = r0; i < r1; i++) {
        const double v = sample[i * D + d];
        q = fma(v, v, q);
    }
    part[(int64_t)blockIdx.x * D + d] = q;
}

__global__ __launch_bounds__(64) void k_nonneg_draw(int D, int64_t N, int64_t nblocks, const double *__restrict__ part, double shape, double rate,
                                                    uint64_t seed, uint32_t sweep, uint32_t entity_tag, double *__restrict__ tau)
{
    const int d = threadIdx.x;
    if (d >= D) return;
    double q = 0.0;
    for (int64_t b = 0; b < nblocks; b++) q += part[b * D + d];
    const double g = bdf_gamma_on(BDF_P_NONNEG_N, BDF_P_NONNEG_U, seed, sweep, entity_tag, (uint64_t)d, shape + 0.5 * (double)N);
    tau[d] = g / (rate + 0.5 * q);
}

// row_sum += u; workgroup 0 adds tau
__global__ __launch_bounds__(64) void k_nonneg_accumulate(int D, int64_t N, const double *__restrict__ sample, const double *__restrict__ tau,
                                                          double *__restrict__ row_sum, double *__restrict__ hyper_sum)
{
    const int d = threadIdx.x;
    if (d >= D) return;
    const int64_t r0 = (int64_t)blockIdx.x * BDF_SPIKE_ROWS_PER_BLOCK;
    const int64_t r1 = r0 + BDF_SPIKE_ROWS_PER_BLOCK < N ? r0 + BDF_SPIKE_ROWS_PER_BLOCK : N;
    for (int64_t i = r0; i < r1; i++) row_sum[i * D + d] += sample[i * D + d];
    if (blockIdx.x == 0) hyper_sum[d] += tau[d];
}

__global__ __launch_bounds__(256) void k_nonneg_lambda(int D, const double *__restrict__ tau, double *__restrict__ out)
{
    for (int t = threadIdx.x; t < D * D + D; t += blockDim.x) {
        double v = 0.0;
        if (t < D * D && t / D == t % D) v = tau[t / D];
        out[t] = v;
    }
}

bool ok_param(double x, double lo) { return x >= lo && x < __builtin_inf(); }

}  // namespace

int bdf_nonneg_lambda_launch(bdf_ctx *ctx, int D, const double *tau, double *Lambda_mu_out)
{
    hipLaunchKernelGGL(k_nonneg_lambda, dim3(1), dim3(256), 0, ctx->stream, D, tau, Lambda_mu_out);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}

int64_t bdf_nonneg_chunk_rows(const bdf_ctx *ctx, int D)
{
    if (ctx->nonneg_chunk > 0) return ctx->nonneg_chunk;
    const int64_t rows = (int64_t)(BDF_NONNEG_SCRATCH_CAP / (((size_t)D * D + D) * sizeof(double)));
    return rows / 64 * 64;            // (whole waves; at least 32,000 rows: D <= BDF_MAX_D)
}

int bdf_nonneg_sweep_launch(bdf_ctx *ctx, const NonnegSweepArgs &a)
{
    if (a.n <= 0) return BDF_OK;
    const dim3 grid((unsigned)((a.n + 63) / 64)), block(64);
    const int DP = bdf_rows_dp(a.D);
    if (DP == 16) hipLaunchKernelGGL(k_nonneg_sweep<16>, grid, block, 0, ctx->stream, a);
    else if (DP == 32) hipLaunchKernelGGL(k_nonneg_sweep<32>, grid, block, 0, ctx->stream, a);
    else hipLaunchKernelGGL(k_nonneg_sweep<64>, grid, block, 0, ctx->stream, a);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}

extern "C" int bdf_ctx_set_nonneg_chunk(bdf_ctx *ctx, int64_t rows)
{
    BDF_REQUIRE(ctx && rows >= 0 && rows <= ((int64_t)1 << 31) - 64, BDF_ERR_ARG, "bdf_ctx_set_nonneg_chunk: 0 (the default) or a positive number of rows below 2^31");
    ctx->nonneg_chunk = rows;
    return BDF_OK;
}

extern "C" int bdf_nonneg_sweep(bdf_ctx *ctx, int D, int64_t n_rows, const double *P, const double *c, const double *u_current,
                                uint32_t entity_tag, int64_t row_begin, double *out)
{
    BDF_REQUIRE(ctx && P && c && u_current && out, BDF_ERR_ARG, "bdf_nonneg_sweep: NULL argument");
    BDF_REQUIRE(D >= 1 && D <= BDF_MAX_D, BDF_ERR_ARG, "bdf_nonneg_sweep: num_latent=%d must be in 1..%d", D, BDF_MAX_D);
    BDF_REQUIRE(n_rows >= 1 && row_begin >= 0, BDF_ERR_ARG, "bdf_nonneg_sweep: n_rows=%lld must be positive, row_begin=%lld not negative",
                (long long)n_rows, (long long)row_begin);
    BDF_REQUIRE(out != u_current, BDF_ERR_ARG, "bdf_nonneg_sweep: out aliases u_current");
    const int64_t chunk = bdf_nonneg_chunk_rows(ctx, D);
    for (int64_t r0 = 0; r0 < n_rows; r0 += chunk) {
        NonnegSweepArgs a{};
        a.P = P + r0 * D * D; a.c = c + r0 * D; a.u_current = u_current + r0 * D; a.out = out + r0 * D;
        a.rows = nullptr; a.row_begin = row_begin + r0; a.n = std::min(chunk, n_rows - r0);
        a.seed = ctx->seed; a.sweep = ctx->sweep_host; a.entity_tag = entity_tag; a.D = D;
        a.wide = D % 2 == 0 && ((uintptr_t)a.P & 15) == 0;
        a.flag = ctx->flag_dev;
        int rc = bdf_nonneg_sweep_launch(ctx, a);
        if (rc) return rc;
    }
    return BDF_OK;
}

extern "C" int bdf_nonneg_hyper(bdf_ctx *ctx, int D, int64_t N, const double *sample, double shape, double rate, uint32_t entity_tag,
                                double *tau)
{
    BDF_REQUIRE(ctx && sample && tau, BDF_ERR_ARG, "bdf_nonneg_hyper: NULL argument");
    BDF_REQUIRE(D >= 1 && D <= BDF_MAX_D, BDF_ERR_ARG, "bdf_nonneg_hyper: num_latent=%d must be in 1..%d", D, BDF_MAX_D);
    BDF_REQUIRE(N >= 1, BDF_ERR_ARG, "bdf_nonneg_hyper: N=%lld must be positive", (long long)N);
    BDF_REQUIRE(ok_param(shape, 0.5), BDF_ERR_ARG, "bdf_nonneg_hyper: shape=%g must be >= 0.5 and finite", shape);
    BDF_REQUIRE(rate > 0.0 && ok_param(rate, 0.0), BDF_ERR_ARG, "bdf_nonneg_hyper: rate=%g must be positive and finite", rate);
    const int64_t nblocks = (N + BDF_SPIKE_ROWS_PER_BLOCK - 1) / BDF_SPIKE_ROWS_PER_BLOCK;
    BDF_REQUIRE(nblocks <= BDF_SPIKE_MAX_BLOCKS, BDF_ERR_ARG, "bdf_nonneg_hyper: N=%lld is more rows than one grid takes", (long long)N);
    void *part;
    int rc = bdf_scratch(ctx, (size_t)nblocks * (size_t)D * sizeof(double), &part);
    if (rc) return rc;
    hipLaunchKernelGGL(k_nonneg_partial, dim3((unsigned)nblocks), dim3(64), 0, ctx->stream, D, N, sample, (double *)part);
    BDF_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_nonneg_draw, dim3(1), dim3(64), 0, ctx->stream, D, N, nblocks, (const double *)part, shape, rate, ctx->seed,
                       ctx->sweep_host, entity_tag, tau);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}

extern "C" int bdf_nonneg_accumulate(bdf_ctx *ctx, int D, int64_t N, const double *sample, const double *tau, double *row_sum,
                                     double *hyper_sum)
{
    BDF_REQUIRE(ctx && sample && tau && row_sum && hyper_sum, BDF_ERR_ARG, "bdf_nonneg_accumulate: NULL argument");
    BDF_REQUIRE(D >= 1 && D <= BDF_MAX_D, BDF_ERR_ARG, "bdf_nonneg_accumulate: num_latent=%d must be in 1..%d", D, BDF_MAX_D);
    BDF_REQUIRE(N >= 1, BDF_ERR_ARG, "bdf_nonneg_accumulate: N=%lld must be positive", (long long)N);
    const int64_t nblocks = (N + BDF_SPIKE_ROWS_PER_BLOCK - 1) / BDF_SPIKE_ROWS_PER_BLOCK;
    BDF_REQUIRE(nblocks <= BDF_SPIKE_MAX_BLOCKS, BDF_ERR_ARG, "bdf_nonneg_accumulate: N=%lld is more rows than one grid takes", (long long)N);
    hipLaunchKernelGGL(k_nonneg_accumulate, dim3((unsigned)nblocks), dim3(64), 0, ctx->stream, D, N, sample, tau, row_sum, hyper_sum);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}
