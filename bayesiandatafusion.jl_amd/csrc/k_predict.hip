// k_predict.hip -- K7: test-set prediction and the running posterior mean of macau.jl:142-203.
//
// pred(r, test_vec) = udot(r, test_vec) + mean_value (src/sampling.jl:9-14); udot is the sum over the latent
// dimension of the product of the modes' factor rows (src/sampling.jl:30-45).  8 lanes share one test pair and read
// 32 bytes each, so that a gathered factor row is read as whole 128-byte segments.
#include "bdf_common.h"
#include "predict.h"
#include <algorithm>
#include <cstdlib>

namespace {

// General kernel: NM modes, any order of the pairs.  VEC = 4: D a multiple of 4, NC 32-byte pieces of a row per lane
// (D <= 32: one, D <= 64: two); VEC = 1: any D, a lane takes elements sub, sub + 8, ...  A trip is 8 consecutive pairs, their
// rows gathered BATCH pairs at a time.
template <int NM, int VEC, int NC>
__global__ __launch_bounds__(256) void k_predict(PredArgs a)
{
    const int tid = threadIdx.x, sub = tid & 7;
    double st[4] = {0.0, 0.0, 0.0, 0.0};
    const int64_t ngroups = (int64_t)gridDim.x * 32, ntrips = (a.n + 7) / 8;
    constexpr int BATCH = (VEC == 1) ? 2 : (NC * NM <= 3 ? 4 : 2);
    for (int64_t trip = (int64_t)blockIdx.x * 32 + tid / 8; trip < ntrips; trip += ngroups) {
        const int64_t p0 = trip * 8;
        PairState ps;
        pair_load(a, p0 + sub, ps);
        int32_t my[NM];
#pragma unroll
        for (int k = 0; k < NM; k++) my[k] = a.ids[(int64_t)k * a.n + ps.pm];
        double keep = 0.0;
#pragma unroll
        for (int u0 = 0; u0 < 8; u0 += BATCH) {
            if (p0 + u0 >= a.n) break;                     // group-uniform
            double s[BATCH];
            if constexpr (VEC == 4) {
                double4 f[BATCH][NM][NC];
#pragma unroll
                for (int u = 0; u < BATCH; u++)
#pragma unroll
                    for (int k = 0; k < NM; k++) {
                        const double *row = a.fac[k] + (int64_t)__shfl(my[k], u0 + u, 8) * a.D;
#pragma unroll
                        for (int c = 0; c < NC; c++) {
                            const int e = sub * 4 + 32 * c;
                            f[u][k][c] = e < a.D ? *(const double4 *)(row + e) : double4{0.0, 0.0, 0.0, 0.0};
                        }
                    }
#pragma unroll
                for (int u = 0; u < BATCH; u++) {
                    double acc = 0.0;
#pragma unroll
                    for (int c = 0; c < NC; c++) {
                        double4 p = f[u][0][c];
#pragma unroll
                        for (int k = 1; k < NM; k++) { p.x *= f[u][k][c].x; p.y *= f[u][k][c].y; p.z *= f[u][k][c].z; p.w *= f[u][k][c].w; }
                        if (sub * 4 + 32 * c < a.D) acc += (p.x + p.y) + (p.z + p.w);
                    }
                    s[u] = acc;
                }
            } else {
#pragma unroll
                for (int u = 0; u < BATCH; u++) {
                    const double *row[NM];
#pragma unroll
                    for (int k = 0; k < NM; k++) row[k] = a.fac[k] + (int64_t)__shfl(my[k], u0 + u, 8) * a.D;
                    double acc = 0.0;
                    for (int e = sub; e < a.D; e += 8) {
                        double p = 1.0;
#pragma unroll
                        for (int k = 0; k < NM; k++) p *= row[k][e];
                        acc += p;
                    }
                    s[u] = acc;
                }
            }
#pragma unroll
            for (int u = 0; u < BATCH; u++) {
                double v = s[u];
                v += __shfl_xor(v, 4); v += __shfl_xor(v, 2); v += __shfl_xor(v, 1);
                if (sub == u0 + u) keep = v;
            }
        }
        pair_finish(a, ps, keep, st);
    }
    if (a.phase >= 0) block_stats(a, st);
}

// Pairs stored sorted by one mode (bdf_pairs_sort), two-mode relation, D a multiple of 4 up to 32: a group of 8 lanes walks RUN
// consecutive pairs and keeps the factor row of the sorted mode in registers while its id does not change -- the update then
// gathers one row per pair instead of two (MovieLens test set sorted by movie: 126 pairs per row; 136 MB instead of 256 MB
// of L2 gathers per update, which is what the update and the row kernel running beside it compete for).  A lane owns two
// pairs of the run (p0 + sub, p0 + 8 + sub), see PairState.
constexpr int RUN = 16;
__global__ __launch_bounds__(256) void k_predict_runs(PredArgs a)
{
    const int tid = threadIdx.x, sub = tid & 7;
    double st[4] = {0.0, 0.0, 0.0, 0.0};
    const int ks = a.sorted_mode, ko = 1 - ks;
    const int32_t *ids_s = a.ids + (int64_t)ks * a.n, *ids_o = a.ids + (int64_t)ko * a.n;
    const double *fs = a.fac[ks], *fo = a.fac[ko];
    const bool live = sub * 4 < a.D;                      // lanes beyond D / 4 hold zeros
    const int eoff = live ? sub * 4 : 0;
    const int64_t p0 = ((int64_t)blockIdx.x * 32 + tid / 8) * RUN;
    PairState ps[2];
    int32_t my_s[2], my_o[2];
#pragma unroll
    for (int q = 0; q < 2; q++) {
        pair_load(a, p0 + 8 * q + sub, ps[q]);
        my_s[q] = ids_s[ps[q].pm]; my_o[q] = ids_o[ps[q].pm];
    }
    int32_t cur = -1;
    double4 srow = {0.0, 0.0, 0.0, 0.0};
    double keep[2] = {0.0, 0.0};
#pragma unroll
    for (int q = 0; q < 2; q++) {
        if (p0 + 8 * q >= a.n) break;                      // group-uniform
        int32_t is[8], io[8];
        double4 orow[8];
#pragma unroll
        for (int u = 0; u < 8; u++) { is[u] = __shfl(my_s[q], u, 8); io[u] = __shfl(my_o[q], u, 8); }
#pragma unroll
        for (int u = 0; u < 8; u++) orow[u] = *(const double4 *)(fo + (int64_t)io[u] * a.D + eoff);
#pragma unroll
        for (int u = 0; u < 8; u++) {
            if (is[u] != cur) { srow = *(const double4 *)(fs + (int64_t)is[u] * a.D + eoff); cur = is[u]; }
            double s = live ? (srow.x * orow[u].x + srow.y * orow[u].y) + (srow.z * orow[u].z + srow.w * orow[u].w) : 0.0;
            s += __shfl_xor(s, 4); s += __shfl_xor(s, 2); s += __shfl_xor(s, 1);
            if (sub == u) keep[q] = s;
        }
    }
#pragma unroll
    for (int q = 0; q < 2; q++) pair_finish(a, ps[q], keep[q], st);
    if (a.phase >= 0) block_stats(a, st);
}

int launch_predict(bdf_ctx *ctx, PredArgs &a)
{
    if (a.n == 0) return BDF_OK;
    if (a.sorted_mode >= 0 && a.n_modes == 2 && (a.D & 3) == 0 && a.D <= 32) {
        const int nblocks = (int)((a.n + 32 * RUN - 1) / (32 * RUN));
        if (a.phase >= 0) {
            void *sc;
            int rc = bdf_scratch(ctx, (size_t)nblocks * 4 * sizeof(double), &sc);
            if (rc) return rc;
            a.partial = (double *)sc;
        }
        hipLaunchKernelGGL(k_predict_runs, dim3(nblocks), dim3(256), 0, ctx->stream, a);
        if (a.phase >= 0) hipLaunchKernelGGL(k_predict_final, dim3(1), dim3(256), 0, ctx->stream, nblocks, (const double *)a.partial, a.stats);
        BDF_HIP(hipGetLastError());
        return BDF_OK;
    }
    const int64_t ntrips = (a.n + 7) / 8;
    const int nblocks = (int)std::min<int64_t>((ntrips + 31) / 32, 8192);
    if (a.phase >= 0) {
        void *sc;
        int rc = bdf_scratch(ctx, (size_t)nblocks * 4 * sizeof(double), &sc);
        if (rc) return rc;
        a.partial = (double *)sc;
    }
#define PRED(NM, VEC, NC) hipLaunchKernelGGL((k_predict<NM, VEC, NC>), dim3(nblocks), dim3(256), 0, ctx->stream, a)
#define PRED_NM(VEC, NC) do { if (a.n_modes == 2) PRED(2, VEC, NC); else if (a.n_modes == 3) PRED(3, VEC, NC); else PRED(4, VEC, NC); } while (0)
    if ((a.D & 3) != 0 || a.n_modes < 2) {
        if (a.n_modes == 1) PRED(1, 1, 1); else PRED_NM(1, 1);
    } else if (a.D <= 32) PRED_NM(4, 1);
    else PRED_NM(4, 2);
#undef PRED_NM
#undef PRED
    if (a.phase >= 0) hipLaunchKernelGGL(k_predict_final, dim3(1), dim3(256), 0, ctx->stream, nblocks, (const double *)a.partial, a.stats);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}

}  // namespace

// ---- pred_all (sampling.jl:91-97): every cell of the relation.  A workgroup takes a TILE of 16 rows of the first mode x 16 cells of
// the others (their flattened index): the first mode's rows sit in LDS, every thread owns one cell and walks the latent dimension
// in order.  (A reporting path -- predictions_full of macau.jl:145-147 -- not the sweep: plain fp64, no matrix cores.)
namespace {
struct PredAllArgs {
    int D, n_modes;
    int64_t dims[BDF_MAX_MODES];
    const double *fac[BDF_MAX_MODES];
    double mean;
    double *out;
    int64_t rest;                  // cells of the modes behind the first: dims[1] * ... * dims[n - 1]
};
__global__ __launch_bounds__(256) void k_predict_all(PredAllArgs a)
{
    __shared__ double u[16][BDF_MAX_D + 1];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int64_t i0 = (int64_t)blockIdx.y * 16, c = (int64_t)blockIdx.x * 16 + tx;
    for (int e = threadIdx.x; e < 16 * a.D; e += 256) {
        const int r = e / a.D, d = e - r * a.D;
        u[r][d] = i0 + r < a.dims[0] ? a.fac[0][(i0 + r) * a.D + d] : 0.0;
    }
    __syncthreads();
    if (c >= a.rest || i0 + ty >= a.dims[0]) return;
    // the cell's indices in the modes behind the first (the last one fastest)
    const double *row[BDF_MAX_MODES];
    int64_t q = c;
#pragma unroll
    for (int k = BDF_MAX_MODES - 1; k >= 1; k--)
        if (k < a.n_modes) { row[k] = a.fac[k] + (q % a.dims[k]) * a.D; q /= a.dims[k]; }
    double s = 0.0;
    for (int d = 0; d < a.D; d++) {
        double pr = u[ty][d];
#pragma unroll
        for (int k = 1; k < BDF_MAX_MODES; k++)
            if (k < a.n_modes) pr *= row[k][d];
        s += pr;
    }
    a.out[(i0 + ty) * a.rest + c] = s + a.mean;
}
}  // namespace

extern "C" int bdf_predict_all(bdf_ctx *ctx, int n_modes, const int64_t *dims, int D, const double *const *factors,
                               double mean_value, double *out)
{
    BDF_REQUIRE(ctx && dims && factors && out, BDF_ERR_ARG, "bdf_predict_all: NULL argument");
    BDF_REQUIRE(n_modes >= 2 && n_modes <= BDF_MAX_MODES, BDF_ERR_ARG, "bdf_predict_all: n_modes=%d must be in 2..%d", n_modes, BDF_MAX_MODES);
    BDF_REQUIRE(D >= 1 && D <= BDF_MAX_D, BDF_ERR_ARG, "bdf_predict_all: num_latent=%d must be in 1..%d", D, BDF_MAX_D);
    PredAllArgs a;
    memset(&a, 0, sizeof(a));
    a.D = D; a.n_modes = n_modes; a.mean = mean_value; a.out = out; a.rest = 1;
    for (int k = 0; k < n_modes; k++) {
        BDF_REQUIRE(dims[k] >= 0 && factors[k] != nullptr, BDF_ERR_ARG, "bdf_predict_all: dims[%d] < 0 or factors[%d] NULL", k, k);
        a.dims[k] = dims[k]; a.fac[k] = factors[k];
        if (k >= 1) a.rest *= dims[k];
    }
    if (a.dims[0] == 0 || a.rest == 0) return BDF_OK;
    const int64_t gx = (a.rest + 15) / 16, gy = (a.dims[0] + 15) / 16;
    BDF_REQUIRE(gx < (int64_t)0x7fffffff && gy <= 65535 * (int64_t)1024, BDF_ERR_BOUNDS, "bdf_predict_all: %lld x %lld cells are too many for one launch",
                (long long)a.dims[0], (long long)a.rest);
    BDF_HIP(hipSetDevice(ctx->device));
    // (grid.y is limited to 65,535 blocks: the first mode in slabs of that many tiles)
    for (int64_t y0 = 0; y0 < gy; y0 += 65535) {
        PredAllArgs b = a;
        const int64_t ny = std::min<int64_t>(65535, gy - y0);
        b.fac[0] = a.fac[0] + y0 * 16 * D;
        b.dims[0] = std::min<int64_t>(a.dims[0] - y0 * 16, ny * 16);
        b.out = a.out + y0 * 16 * a.rest;
        hipLaunchKernelGGL(k_predict_all, dim3((unsigned)gx, (unsigned)ny), dim3(256), 0, ctx->stream, b);
    }
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}

extern "C" int bdf_pairs_create(bdf_ctx *ctx, int n_modes, int64_t n, const void *ids, int id_bytes,
                                const double *values, bdf_pairs **out)
{
    BDF_REQUIRE(ctx && out, BDF_ERR_ARG, "bdf_pairs_create: NULL argument");
    BDF_REQUIRE(n_modes >= 2 && n_modes <= BDF_MAX_MODES, BDF_ERR_ARG, "bdf_pairs_create: n_modes=%d must be in 2..%d", n_modes, BDF_MAX_MODES);
    BDF_REQUIRE(id_bytes == 4 || id_bytes == 8, BDF_ERR_ARG, "bdf_pairs_create: id_bytes must be 4 or 8");
    BDF_REQUIRE(n >= 0 && (n == 0 || (ids && values)), BDF_ERR_ARG, "bdf_pairs_create: ids/values NULL");
    BDF_HIP(hipSetDevice(ctx->device));
    std::vector<int32_t> h((size_t)n * n_modes);
    for (size_t q = 0; q < h.size(); q++) {
        int64_t v = id_bytes == 8 ? ((const int64_t *)ids)[q] : (int64_t)((const int32_t *)ids)[q];
        BDF_REQUIRE(v >= 1 && v < (int64_t)0x7fffffff, BDF_ERR_BOUNDS, "bdf_pairs_create: id %lld out of range", (long long)v);
        h[q] = (int32_t)(v - 1);
    }
    std::unique_ptr<bdf_pairs> p(new bdf_pairs());       // error paths free what was allocated
    p->ctx = ctx; p->n_modes = n_modes; p->n = n;
    p->ids_host = h;
    p->values_host.assign(values, values + (n ? n : 0));
    size_t nb = std::max<size_t>((size_t)n * sizeof(double), 8);
    int rc;
    if ((rc = p->ids_dev.alloc_bytes(std::max<size_t>(h.size() * sizeof(int32_t), 8))) || (rc = p->values_dev.alloc_bytes(nb)) ||
        (rc = p->avg_dev.alloc_bytes(nb)) || (rc = p->sq_dev.alloc_bytes(nb)))
        return rc;
    if (n) {
        BDF_HIP(hipMemcpy(p->ids_dev, h.data(), h.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        BDF_HIP(hipMemcpy(p->values_dev, values, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    }
    // (on the context's stream and waited for: the pairs may be updated on another stream next, and a plain hipMemset may still
    // be pending on the NULL stream when it returns)
    BDF_HIP(hipMemsetAsync(p->avg_dev, 0, nb, ctx->stream));
    BDF_HIP(hipMemsetAsync(p->sq_dev, 0, nb, ctx->stream));
    BDF_HIP(hipStreamSynchronize(ctx->stream));
    *out = p.release();
    return BDF_OK;
}

bdf_pairs::~bdf_pairs()
{
    if (!ctx) return;
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
}

extern "C" int bdf_pairs_destroy(bdf_pairs *p)
{
    if (p) delete p;
    return BDF_OK;
}

extern "C" int bdf_predict(bdf_ctx *ctx, const bdf_pairs *p, int D, const double *const *factors,
                           double mean_value, double *out)
{
    PredArgs a;
    int rc = fill("bdf_predict", ctx, p, D, factors, a);
    if (rc) return rc;
    BDF_REQUIRE(out != nullptr, BDF_ERR_ARG, "bdf_predict: out is NULL");
    a.mean = mean_value; a.out = out;
    return p->link ? bdf_predict_link(ctx, p, D, factors, mean_value, nullptr, out, -1, 0.0, 1.0, 0.0, 0.0, nullptr) : launch_predict(ctx, a);
}

// udot + mean_value, whatever baseline the pairs carry (sample_beta_rel needs the residual against the plain mean)
int bdf_predict_plain(bdf_ctx *ctx, const bdf_pairs *p, int D, const double *const *factors, double mean_value, double *out)
{
    PredArgs a;
    int rc = fill("bdf_predict", ctx, p, D, factors, a);
    if (rc) return rc;
    a.mean = mean_value; a.linear = nullptr; a.out = out;
    return launch_predict(ctx, a);
}

extern "C" int bdf_predict_update(bdf_ctx *ctx, bdf_pairs *p, int D, const double *const *factors,
                                  double mean_value, int phase, double clamp_lo, double clamp_hi,
                                  double class_cut, double *stats_out)
{
    PredArgs a;
    int rc = fill("bdf_predict_update", ctx, p, D, factors, a);
    if (rc) return rc;
    BDF_REQUIRE(stats_out != nullptr, BDF_ERR_ARG, "bdf_predict_update: stats_out is NULL");
    BDF_REQUIRE(phase >= 0 && phase <= 2, BDF_ERR_ARG, "bdf_predict_update: phase must be 0, 1 or 2");
    a.mean = mean_value; a.avg = p->avg_dev; a.sq = p->sq_dev; a.phase = phase; a.count = p->count;
    a.clamp_lo = clamp_lo; a.clamp_hi = clamp_hi; a.cut = class_cut; a.stats = stats_out;
    // (sorted pairs of a two-mode relation without a per-pair baseline -- the sweep's test set: the kernel that fits beside the row
    // kernel's waves, k_update_runs.hip; the same values as k_predict_runs, which keeps the predictions and the baselines)
    const bool runs = a.sorted_mode >= 0 && a.n_modes == 2 && (a.D & 3) == 0 && a.D <= 32 && a.linear == nullptr;
    rc = p->link ? bdf_predict_link(ctx, p, D, factors, mean_value, nullptr, nullptr, phase, p->count, clamp_lo, clamp_hi, class_cut, stats_out)
         : runs  ? bdf_update_runs(ctx, p, D, factors, mean_value, phase, p->count, clamp_lo, clamp_hi, class_cut, stats_out)
                 : launch_predict(ctx, a);
    if (rc) return rc;
    if (phase == 1) p->count = 1.0;
    else if (phase == 2) p->count += 1.0;
    return BDF_OK;
}

extern "C" int bdf_predict_sse(bdf_ctx *ctx, const bdf_pairs *p, int D, const double *const *factors, double mean_value,
                               const double *linear_values, double *stats_out)
{
    // sum over the pairs of (value - pred)^2 with pred = udot + (linear_values[pair] | mean_value): the err' err of
    // sample_alpha (macau.jl:86-87); stats_out as bdf_predict_update's, [1] is the sum of squares
    PredArgs a;
    int rc = fill("bdf_predict_sse", ctx, p, D, factors, a);
    if (rc) return rc;
    BDF_REQUIRE(stats_out != nullptr, BDF_ERR_ARG, "bdf_predict_sse: stats_out is NULL");
    a.mean = mean_value; if (linear_values) a.linear = linear_values; a.phase = 3; a.count = 0.0;
    a.clamp_lo = 1.0; a.clamp_hi = 0.0; a.cut = 0.0; a.stats = stats_out;
    if (p->link) return bdf_predict_link(ctx, p, D, factors, mean_value, linear_values, nullptr, 3, 0.0, 1.0, 0.0, 0.0, stats_out);
    return launch_predict(ctx, a);
}

extern "C" int bdf_pairs_sort(bdf_pairs *p, int mode)
{
    // Store the pairs sorted by their id in `mode` (stable): consecutive pairs then share that mode's factor row, which
    // the 8 lanes of the next pair find in cache -- half the gather traffic of a prediction update.  The caller's order
    // is kept in every interface: bdf_predict's out and the baseline are indexed through the permutation, bdf_pairs_order
    // returns it for the running state (bdf_pairs_state stays in storage order).  Only before the first update.
    BDF_REQUIRE(p != nullptr, BDF_ERR_ARG, "bdf_pairs_sort: NULL argument");
    BDF_REQUIRE(mode >= 0 && mode < p->n_modes, BDF_ERR_ARG, "bdf_pairs_sort: mode %d out of range", mode);
    BDF_REQUIRE(p->count == 0.0 && p->orig_dev == nullptr, BDF_ERR_ARG, "bdf_pairs_sort: the pairs already hold prediction state or are sorted");
    const int64_t n = p->n;
    if (n == 0) return BDF_OK;
    BDF_HIP(hipSetDevice(p->ctx->device));
    std::vector<int32_t> perm((size_t)n);
    for (int64_t i = 0; i < n; i++) perm[(size_t)i] = (int32_t)i;
    const int32_t *key = p->ids_host.data() + (size_t)mode * n;
    std::stable_sort(perm.begin(), perm.end(), [key](int32_t x, int32_t y) { return key[x] < key[y]; });
    std::vector<int32_t> ids((size_t)n * p->n_modes);
    std::vector<double> vals((size_t)n);
    for (int k = 0; k < p->n_modes; k++)
        for (int64_t i = 0; i < n; i++) ids[(size_t)k * n + i] = p->ids_host[(size_t)k * n + perm[(size_t)i]];
    for (int64_t i = 0; i < n; i++) vals[(size_t)i] = p->values_host[(size_t)perm[(size_t)i]];
    BDF_HIP(hipStreamSynchronize(p->ctx->stream));
    BDF_HIP(hipMemcpy(p->ids_dev, ids.data(), ids.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    BDF_HIP(hipMemcpy(p->values_dev, vals.data(), vals.size() * sizeof(double), hipMemcpyHostToDevice));
    if (int rc = p->orig_dev.alloc((size_t)n)) return rc;
    BDF_HIP(hipMemcpy(p->orig_dev, perm.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
    p->orig_host = perm;
    p->sorted_mode = mode;
    return BDF_OK;
}

extern "C" int bdf_pairs_order(const bdf_pairs *p, int64_t *orig_host)
{
    // orig_host[i] = the caller's index of the pair stored at position i (identity unless bdf_pairs_sort was called)
    BDF_REQUIRE(p && orig_host, BDF_ERR_ARG, "bdf_pairs_order: NULL argument");
    for (int64_t i = 0; i < p->n; i++) orig_host[i] = p->orig_host.empty() ? i : (int64_t)p->orig_host[(size_t)i];
    return BDF_OK;
}

extern "C" int bdf_pairs_set_baseline(bdf_pairs *p, const double *baseline)
{
    BDF_REQUIRE(p != nullptr, BDF_ERR_ARG, "bdf_pairs_set_baseline: NULL argument");
    p->baseline_dev = baseline;
    return BDF_OK;
}

extern "C" int bdf_pairs_set_link(bdf_pairs *p, int link)
{
    BDF_REQUIRE(p != nullptr, BDF_ERR_ARG, "bdf_pairs_set_link: NULL argument");
    BDF_REQUIRE(link == 0 || link == 1, BDF_ERR_ARG, "bdf_pairs_set_link: link=%d must be 0 (identity) or 1 (probit)", link);
    p->link = link;
    return BDF_OK;
}

extern "C" int bdf_pairs_set_logistic_link(bdf_pairs *p)
{
    BDF_REQUIRE(p != nullptr, BDF_ERR_ARG, "bdf_pairs_set_logistic_link: NULL argument");
    p->link = 2;
    return BDF_OK;
}

extern "C" int bdf_pairs_set_count_link(bdf_pairs *p, double r)
{
    BDF_REQUIRE(p != nullptr, BDF_ERR_ARG, "bdf_pairs_set_count_link: NULL argument");
    BDF_REQUIRE(r >= 1.0 && r <= 2147483648.0 && r == std::floor(r), BDF_ERR_ARG, "bdf_pairs_set_count_link: r=%g must be an integer, at least 1", r);
    p->link = 3;
    p->link_r = r;
    return BDF_OK;
}

extern "C" int bdf_pairs_state(const bdf_pairs *p, double **avg, double **sq, int64_t *n)
{
    BDF_REQUIRE(p && avg && sq && n, BDF_ERR_ARG, "bdf_pairs_state: NULL argument");
    *avg = p->avg_dev; *sq = p->sq_dev; *n = p->n;
    return BDF_OK;
}
