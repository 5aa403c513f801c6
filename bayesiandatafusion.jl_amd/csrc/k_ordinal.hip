// k_ordinal.hip -- the ordinal probit noise model: a relation whose training values are levels 1 .. K of a
// latent z ~ N(udot + mean_value, 1 / alpha) cut at e_1 < ... < e_{K-1}, of which the two outer edges are fixed and the K - 3
// between them are sampled.  Given the edges the model IS the interval model (k_interval.hip) with every row's bounds
// (e_{y-1}, e_y); what this unit adds is the edges' own update, one Metropolis step per iteration with z integrated out
// (Cowles 1996), in four launches on one stream and without a word to the host:
//
// k_ordinal_propose (one wave): the K - 3 normals of the step's stream, the proposed edge table and the log Jacobian (ordinal.h).
// k_ordinal_mass: the lane prologue, gather and dot product of pair_gather.h and, in the lane that owns the pair, the difference of the
//   log masses (lpd.h, bdf_lpd_mass) of its level's interval under the proposed and the current edges; both tables (17 doubles each)
//   sit in LDS.  A pair whose level kept both its edges -- levels 1 and K always -- contributes an exact 0 and evaluates nothing;
//   a group of 8 lanes with no other pair gathers nothing.  Per-workgroup sums through the statistics' reduction of predict.h.
// k_ordinal_accept (one workgroup): the fixed-order sum, the decision against the step's uniform, the published edges, the step
//   size, the counters and the trace row.
// k_ordinal_bounds: every row's (lower, upper) from its code and the edges, one 16-byte store per row; as the step's last launch
//   it returns at once when the proposal was refused, the bounds being what they were.
//
// No scratch, no LDS beyond the reduction's 128 bytes and the tables, plain vector stores.
#include "bdf_common.h"
#include "ordinal.h"
#include "predict.h"
#include "pair_gather.h"

namespace {

struct OrdMassArgs {
    PairArgs pair;
    int K;
    const int8_t *codes;           // the caller's order: the level 1 .. K of every pair
    const double *st;              // the object's state (BDF_ORD_*)
    double *partial;               // per-block statistics
};

__device__ __forceinline__ int level_of(const int8_t *codes, int64_t i, int K)
{
    const int c = codes[i];
    return c < 1 ? 1 : (c > K ? K : c);          // (the host refuses other codes; never an index outside the table)
}

// No grid-stride loop, as k_lpd and for its reason.  Every lane of a launch whose proposal
// stands reaches the statistics' barrier; a launch whose proposal fell to the gap guard leaves at once, all of it.
template <int NM, int VEC, int NC>
__global__ __launch_bounds__(256, (VEC == 4 && NM * NC >= 8) ? 2 : 3) void k_ordinal_mass(OrdMassArgs a)
{
    __shared__ double tab[2 * BDF_ORD_TABLE];                  // the current table, then the proposed one
    const int tid = threadIdx.x;
    if (a.st[BDF_ORD_VALID] == 0.0) return;
    if (tid < 2 * BDF_ORD_TABLE) tab[tid] = a.st[BDF_ORD_CUR + tid];
    __syncthreads();
    const double alpha = pair_alpha(a.pair);
    const int64_t trip = pair_trip();
    double st[4] = {0.0, 0.0, 0.0, 0.0};
    if (trip * 8 < a.pair.n) {
        PairLane<NM> l;
        pair_lane(a.pair, trip, l);
        const int c = level_of(a.codes, l.po, a.K);
        const double lo0 = tab[c - 1], hi0 = tab[c], lo1 = tab[BDF_ORD_TABLE + c - 1], hi1 = tab[BDF_ORD_TABLE + c];
        const bool moved = l.ok && c > 1 && c < a.K && (lo0 != lo1 || hi0 != hi1);
        if (group_any(moved)) {
            const double m = pair_dot<NM, VEC, NC>(a.pair, l) + a.pair.mean;
            if (moved) st[0] = bdf_lpd_mass(m, lo1, hi1, alpha) - bdf_lpd_mass(m, lo0, hi0, alpha);
        }
    }
    block_stats(a.partial, st);
}

struct OrdStepArgs {
    int K, adapt;                  // adapt: 0 frozen, 1 adapt, -1: adapt while fewer than adapt_steps steps have been taken
    double *st;
    uint64_t seed;
    uint32_t sweep, entity;        // pair_entity(rel_tag)
    int nblocks;
    const double *partial;
    int64_t adapt_steps, capacity;
};

__global__ __launch_bounds__(64) void k_ordinal_propose(OrdStepArgs a)
{
    __shared__ double eps[BDF_ORD_MAX_K];
    const int lane = threadIdx.x;
    if (lane < a.K - 3) eps[lane] = bdf_normal(a.seed, a.sweep, BDF_P_ORDINAL, a.entity, 0, lane);
    __syncthreads();
    if (lane == 0) {
        double jac;
        const bool ok = bdf_ordinal_propose(a.K, a.st + BDF_ORD_CUR, a.st[BDF_ORD_SIGMA], eps, a.st + BDF_ORD_PROP, &jac);
        a.st[BDF_ORD_JAC] = jac;
        a.st[BDF_ORD_VALID] = ok ? 1.0 : 0.0;
    }
}

__global__ __launch_bounds__(256) void k_ordinal_accept(OrdStepArgs a)
{
    __shared__ double red[4];
    const int tid = threadIdx.x;
    const bool valid = a.st[BDF_ORD_VALID] != 0.0;
    double v = 0.0;
    if (valid)
        for (int b = tid; b < a.nblocks; b += 256) v += a.partial[b * 4];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    if (tid != 0) return;
    const double S = valid ? ((red[0] + red[1]) + (red[2] + red[3])) + a.st[BDF_ORD_JAC] : -INFINITY;
    const double lu = log(bdf_uniform(a.seed, a.sweep, BDF_P_ORDINAL, a.entity, 1, 0));
    const bool acc = valid && lu < S;
    if (acc)
        for (int k = 0; k <= a.K; k++) a.st[BDF_ORD_CUR + k] = a.st[BDF_ORD_PROP + k];
    const double before = a.st[BDF_ORD_PROPOSALS], i = before + 1.0;
    if (a.adapt > 0 || (a.adapt < 0 && before < (double)a.adapt_steps))
        a.st[BDF_ORD_SIGMA] = bdf_ordinal_adapt(a.st[BDF_ORD_SIGMA], acc, i);
    a.st[BDF_ORD_PROPOSALS] = i;
    if (acc) a.st[BDF_ORD_ACCEPTS] += 1.0;
    a.st[BDF_ORD_LAST_S] = S;
    a.st[BDF_ORD_ACCEPTED] = acc ? 1.0 : 0.0;
    a.st[BDF_ORD_LOGU] = lu;
    const int64_t row = (int64_t)before;
    if (row < a.capacity)
        for (int k = 1; k <= a.K - 1; k++) a.st[BDF_ORD_TRACE + row * (a.K - 1) + (k - 1)] = a.st[BDF_ORD_CUR + k];
}

struct OrdBoundsArgs {
    int K, only_accepted;
    int64_t n;
    const double *st;
    const int8_t *codes;
    double2 *out;
};

__global__ __launch_bounds__(256) void k_ordinal_bounds(OrdBoundsArgs a)
{
    if (a.only_accepted && a.st[BDF_ORD_ACCEPTED] == 0.0) return;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const int c = level_of(a.codes, i, a.K);
    a.out[i] = double2{a.st[BDF_ORD_CUR + c - 1], a.st[BDF_ORD_CUR + c]};
}

int enqueue_bounds(const char *who, bdf_ctx *ctx, const bdf_ordinal *ord, const int8_t *codes_dev, int64_t n, double *bounds_out, int only_accepted)
{
    BDF_REQUIRE(((uintptr_t)bounds_out & 15) == 0, BDF_ERR_ARG, "%s: the bounds must be aligned to 16 bytes", who);
    BDF_REQUIRE(n >= 0 && (n + 255) / 256 <= INT32_MAX, BDF_ERR_ARG, "%s: %lld rows are more than one launch covers", who, (long long)n);
    if (n == 0) return BDF_OK;
    OrdBoundsArgs b;
    b.K = ord->K; b.only_accepted = only_accepted; b.n = n; b.st = ord->state_dev; b.codes = codes_dev; b.out = (double2 *)bounds_out;
    hipLaunchKernelGGL(k_ordinal_bounds, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, b);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}

}  // namespace

extern "C" int bdf_ordinal_create(bdf_ctx *ctx, int K, double step, int64_t trace_capacity, bdf_ordinal **out)
{
    BDF_REQUIRE(ctx && out, BDF_ERR_ARG, "bdf_ordinal_create: NULL argument");
    BDF_REQUIRE(K >= BDF_ORD_MIN_K && K <= BDF_ORD_MAX_K, BDF_ERR_ARG, "bdf_ordinal_create: %d levels; must be in %d..%d", K, BDF_ORD_MIN_K, BDF_ORD_MAX_K);
    BDF_REQUIRE(step >= 1e-8 && step <= 10.0, BDF_ERR_ARG, "bdf_ordinal_create: step=%g must be in [1e-8, 10]", step);
    BDF_REQUIRE(trace_capacity >= 0 && trace_capacity <= BDF_ORD_MAX_TRACE, BDF_ERR_ARG, "bdf_ordinal_create: trace_capacity=%lld must be in 0..%lld",
                (long long)trace_capacity, (long long)BDF_ORD_MAX_TRACE);
    // the head of the buffer from the host (48 doubles); the trace is filled on the device: bytes of all ones are a NaN
    double h[BDF_ORD_TRACE];
    for (int k = 0; k < BDF_ORD_TRACE; k++) h[k] = 0.0;
    for (int t = 0; t < 2; t++) {
        double *e = h + (t ? BDF_ORD_PROP : BDF_ORD_CUR);
        for (int k = 0; k < BDF_ORD_TABLE; k++) e[k] = k == 0 ? -INFINITY : (k < K ? (double)k + 0.5 : INFINITY);
    }
    h[BDF_ORD_SIGMA] = step;
    const size_t trace_doubles = (size_t)trace_capacity * (size_t)(K - 1);
    BDF_HIP(hipSetDevice(ctx->device));
    std::unique_ptr<bdf_ordinal> o(new bdf_ordinal());
    o->ctx = ctx; o->K = K; o->capacity = trace_capacity; o->state_doubles = BDF_ORD_TRACE + trace_doubles;
    o->stream = ctx->stream;
    if (int rc = o->state_dev.alloc(o->state_doubles)) return rc;
    double *dev = o->state_dev;
    hipError_t e = hipMemcpy(dev, h, sizeof(h), hipMemcpyHostToDevice);
    if (e == hipSuccess && trace_doubles) e = hipMemset(dev + BDF_ORD_TRACE, 0xff, trace_doubles * sizeof(double));
    if (e != hipSuccess) {
        bdf_set_error("bdf_ordinal_create: filling the state failed: %s", hipGetErrorString(e));
        return BDF_ERR_HIP;
    }
    *out = o.release();
    return BDF_OK;
}

extern "C" int bdf_ordinal_destroy(bdf_ordinal *ord)
{
    if (ord) delete ord;
    return BDF_OK;
}

extern "C" int bdf_ordinal_set_adapt(bdf_ordinal *ord, int64_t steps)
{
    BDF_REQUIRE(ord && steps >= 0, BDF_ERR_ARG, "bdf_ordinal_set_adapt: bad argument");
    ord->adapt_steps = steps;
    return BDF_OK;
}

extern "C" int bdf_ordinal_step(bdf_ctx *ctx, bdf_ordinal *ord, const bdf_pairs *train, const int8_t *codes_dev, int D, const double *const *factors,
                                double mean_value, double alpha, const double *alpha_dev, uint32_t rel_tag, int adapt, double *bounds_dev)
{
    BDF_REQUIRE(ord && codes_dev && bounds_dev, BDF_ERR_ARG, "bdf_ordinal_step: NULL argument");
    BDF_REQUIRE(((uintptr_t)bounds_dev & 15) == 0, BDF_ERR_ARG, "bdf_ordinal_step: bounds_dev must be aligned to 16 bytes");
    BDF_REQUIRE(adapt >= -1 && adapt <= 1, BDF_ERR_ARG, "bdf_ordinal_step: adapt must be -1, 0 or 1");
    OrdMassArgs m = {};
    int rc = pair_fill("bdf_ordinal_step", ctx, train, D, factors, mean_value, true, alpha, alpha_dev, m.pair);
    if (rc) return rc;
    BDF_REQUIRE(ctx->device == ord->ctx->device, BDF_ERR_ARG, "bdf_ordinal_step: the context and the object are on different devices");
    m.K = ord->K; m.codes = codes_dev; m.st = ord->state_dev;
    int nblocks;
    if ((rc = pair_blocks("bdf_ordinal_step", "observations", train->n, &nblocks, INT32_MAX / 4))) return rc;
    BDF_HIP(hipSetDevice(ctx->device));
    // (the sum behind the launch is k_ordinal_accept's own, with the decision: no launch_reduced here)
    void *sc;
    if ((rc = bdf_scratch(ctx, (size_t)std::max(nblocks, 1) * 4 * sizeof(double), &sc))) return rc;
    m.partial = (double *)sc;
    OrdStepArgs s;
    memset(&s, 0, sizeof(s));
    s.K = ord->K; s.adapt = adapt; s.st = ord->state_dev; s.seed = ctx->seed; s.sweep = ctx->sweep_host; s.entity = pair_entity(rel_tag);
    s.nblocks = nblocks; s.partial = m.partial; s.adapt_steps = ord->adapt_steps; s.capacity = ord->capacity;
    ord->stream = ctx->stream;
    hipLaunchKernelGGL(k_ordinal_propose, dim3(1), dim3(64), 0, ctx->stream, s);
    if (nblocks > 0) BDF_BY_SHAPE(k_ordinal_mass, train->n_modes, D, nblocks, ctx->stream, m);
    hipLaunchKernelGGL(k_ordinal_accept, dim3(1), dim3(256), 0, ctx->stream, s);
    BDF_HIP(hipGetLastError());
    return enqueue_bounds("bdf_ordinal_step", ctx, ord, codes_dev, train->n, bounds_dev, 1);
}

extern "C" int bdf_ordinal_bounds(bdf_ctx *ctx, const bdf_ordinal *ord, const int8_t *codes_dev, int64_t n, double *bounds_out)
{
    BDF_REQUIRE(ctx && ord && (n == 0 || (codes_dev && bounds_out)), BDF_ERR_ARG, "bdf_ordinal_bounds: NULL argument");
    BDF_REQUIRE(ctx->device == ord->ctx->device, BDF_ERR_ARG, "bdf_ordinal_bounds: the context and the object are on different devices");
    BDF_HIP(hipSetDevice(ctx->device));
    return enqueue_bounds("bdf_ordinal_bounds", ctx, ord, codes_dev, n, bounds_out, 0);
}

extern "C" int bdf_ordinal_read(bdf_ordinal *ord, double *edges, double *sigma, int64_t *proposals, int64_t *accepts, double *last_S,
                                double *trace, int64_t trace_rows)
{
    BDF_REQUIRE(ord, BDF_ERR_ARG, "bdf_ordinal_read: NULL argument");
    BDF_REQUIRE(trace_rows >= 0 && trace_rows <= ord->capacity, BDF_ERR_ARG, "bdf_ordinal_read: %lld trace rows asked for, the object keeps %lld",
                (long long)trace_rows, (long long)ord->capacity);
    BDF_REQUIRE(trace_rows == 0 || trace, BDF_ERR_ARG, "bdf_ordinal_read: trace is NULL");
    BDF_HIP(hipSetDevice(ord->ctx->device));
    BDF_HIP(hipStreamSynchronize(ord->stream));
    double h[BDF_ORD_TRACE];
    BDF_HIP(hipMemcpy(h, ord->state_dev, sizeof(h), hipMemcpyDeviceToHost));
    if (edges) for (int k = 1; k <= ord->K - 1; k++) edges[k - 1] = h[BDF_ORD_CUR + k];
    if (sigma) *sigma = h[BDF_ORD_SIGMA];
    if (proposals) *proposals = (int64_t)h[BDF_ORD_PROPOSALS];
    if (accepts) *accepts = (int64_t)h[BDF_ORD_ACCEPTS];
    if (last_S) *last_S = h[BDF_ORD_LAST_S];
    if (trace_rows) BDF_HIP(hipMemcpy(trace, ord->state_dev + BDF_ORD_TRACE, (size_t)trace_rows * (size_t)(ord->K - 1) * sizeof(double), hipMemcpyDeviceToHost));
    return BDF_OK;
}

extern "C" int bdf_ordinal_proposal(bdf_ordinal *ord, double *edges, double *jacobian, int *accepted, double *log_u)
{
    BDF_REQUIRE(ord, BDF_ERR_ARG, "bdf_ordinal_proposal: NULL argument");
    BDF_HIP(hipSetDevice(ord->ctx->device));
    BDF_HIP(hipStreamSynchronize(ord->stream));
    double h[BDF_ORD_TRACE];
    BDF_HIP(hipMemcpy(h, ord->state_dev, sizeof(h), hipMemcpyDeviceToHost));
    if (edges) for (int k = 1; k <= ord->K - 1; k++) edges[k - 1] = h[BDF_ORD_PROP + k];
    if (jacobian) *jacobian = h[BDF_ORD_JAC];
    if (accepted) *accepted = h[BDF_ORD_ACCEPTED] != 0.0;
    if (log_u) *log_u = h[BDF_ORD_LOGU];
    return BDF_OK;
}
