// k_diag.hip -- convergence diagnostics of held-out predictions (setDiagnostics): every posterior draw of the
// test cells' predictions is kept on the device, and at the end of the run every cell's series -- and one or two traced scalars'
// -- gives its split R-hat, its effective sample size and the Monte Carlo standard error of its mean.
//
// The plane: capacity rows (draws) of n_cells + n_scalars doubles, draw-major.  A row holds the cells in the pairs' STORAGE order,
// then the scalars: [0] this draw's sum over the cells of (value - p)^2, [1] its alpha.
//
// bdf_diag_push: k_diag_push, one more of pair_gather.h's kernels (8 lanes to 8 consecutive pairs, no loop): the owning lane forms p
// as k_predict's does (pair_finish of predict.h: dot + base, then the pairs' link) and stores it at its storage position in the
// next row -- coalesced.  (value - p)^2 leaves through the workgroup's statistics and their fixed-order sum; alpha rides in the
// second statistic of one lane (a sum of one alpha and zeros is that alpha), so both scalars come out of one final kernel.
//
// bdf_diag_compute: k_diag, one lane per series, a workgroup of one wave per 64 consecutive series.  The wave's tile (all draws
// x 64 series, rows of 512 bytes) sits in LDS while it fits the 160 KB of a workgroup (draws <= BDF_DIAG_LDS_DRAWS); beyond that the
// same code reads the plane itself, where a wave's load is the same 512-byte row.  The autocovariances are taken two lags at a
// time, as Geyer's pairs need them, until the lane's pair sum is not positive; a lane that has stopped idles until its wave's last
// one has (series of one wave are neighbours, not alike: nothing is rebalanced).  The summary -- max, min and three exact
// counts per workgroup, combined by k_diag_final -- does not depend on the grid or on any order.
//
// f64 throughout, no scratch, plain vector stores.
#include "bdf_common.h"
#include "predict.h"
#include "pair_gather.h"
#include <cmath>

#define BDF_DIAG_LDS_DRAWS 320     // 64 series x 320 draws x 8 bytes = 160 KB
#define BDF_DIAG_STATS 6           // max R-hat, min ESS, R-hat > cut, ESS < cut, constant series, draws; then 3 per scalar

struct bdf_diag {
    bdf_ctx *ctx = nullptr;        // borrowed
    int64_t n_cells = 0, capacity = 0, draws = 0;
    int n_scalars = 0;
    DevBuf<double> plane_dev;      // capacity x (n_cells + n_scalars), draw-major
    DevBuf<double> stage_dev;      // a push's four statistics, of which the row takes the first n_scalars
    ~bdf_diag()
    {
        if (!ctx) return;
        hipSetDevice(ctx->device);
        hipStreamSynchronize(ctx->stream);
    }
};

namespace {

struct DiagPushArgs {
    PairArgs pair;
    const double *baseline;        // nullable: per-pair baseline instead of mean (the caller's order)
    int link;                      // the pairs' (bdf_pairs_set_link and its kin)
    double link_r;
    int with_alpha;                // the row has a second scalar
    double *row;                   // this draw's row of the plane
    double *partial;               // per-block statistics
};

// No grid-stride loop, as the other kernels of pair_gather.h.  Every lane reaches the statistics' barrier.
template <int NM, int VEC, int NC>
__global__ __launch_bounds__(256) void k_diag_push(DiagPushArgs a)
{
    double st[4] = {0.0, 0.0, 0.0, 0.0};
    const int64_t trip = pair_trip();
    if (trip * 8 < a.pair.n) {                     // (group-uniform)
        PairLane<NM> l;
        pair_lane(a.pair, trip, l);
        const double y = a.pair.values[l.pm];
        const double base = a.baseline ? a.baseline[l.po] : a.pair.mean;
        const double dot = pair_dot<NM, VEC, NC>(a.pair, l);
        if (l.ok) {
            double p = dot + base;
            if (a.link == 1) p = bdf_phi(p);
            else if (a.link == 2) p = bdf_pg_logistic(p);
            else if (a.link == 3) p = bdf_pg_count_mean(p, a.link_r);
            a.row[l.pm] = p;
            const double e = y - p;
            st[0] = e * e;
        }
    }
    if (a.with_alpha && blockIdx.x == 0 && threadIdx.x == 0) st[1] = pair_alpha(a.pair);
    block_stats(a.partial, st);
}

struct DiagArgs {
    const double *plane;
    int64_t stride, n_cells, total;    // doubles per row; series that are cells; all series (cells, then scalars)
    int n, h, off2;                    // draws; h = n / 2; the second chain starts at n - h
    double cap;                        // 2 h log10(2 h)
    double rhat_cut, ess_cut;
    const int32_t *orig;               // nullable: storage position -> the caller's index
    double *out;                       // nullable: n_cells x 3 in the caller's order
    double *scalars;                   // 3 per scalar
    double *partial;                   // 5 per workgroup: max R-hat, min ESS, three counts
};

// the statistic of DESIGN.md section 32 for the series that this lane owns; x(i): its value of draw i
template <bool IN_LDS>
__global__ __launch_bounds__(64) void k_diag(DiagArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double tile[];      // IN_LDS: [draw][64]
    const int lane = threadIdx.x;
    const int64_t s = (int64_t)blockIdx.x * 64 + lane;
    const bool mine = s < a.total;
    const double *col = a.plane + (mine ? s : a.total - 1);           // a lane past the end reads the last series, and keeps nothing
    const int n = a.n, h = a.h, off2 = a.off2;
    if constexpr (IN_LDS) {
        for (int i = 0; i < n; i++) tile[i * 64 + lane] = col[(int64_t)i * a.stride];
        __syncthreads();
    }
    auto x = [&](int i) -> double {
        if constexpr (IN_LDS) return tile[i * 64 + lane];
        else return col[(int64_t)i * a.stride];
    };

    bool finite = true;
    double m1 = 0.0, m2 = 0.0;
    for (int i = 0; i < h; i++) {
        const double u = x(i), v = x(off2 + i);
        finite = finite && isfinite(u) && isfinite(v);
        m1 += u; m2 += v;
    }
    m1 /= (double)h; m2 /= (double)h;
    double q1 = 0.0, q2 = 0.0;
    for (int i = 0; i < h; i++) {
        const double u = x(i) - m1, v = x(off2 + i) - m2;
        q1 += u * u; q2 += v * v;
    }
    const double W = (q1 / (double)(h - 1) + q2 / (double)(h - 1)) / 2.0;
    const double dm = m1 - m2;
    const double varp = W * (double)(h - 1) / (double)h + dm * dm / 2.0;
    const bool bad = !(finite && W > 0.0 && isfinite(W));

    // Geyer's initial monotone sequence: P_k = rho_2k + rho_2k+1 while 2k + 1 <= h - 1, up to the first P_k <= 0
    bool done = bad || !mine;
    double sumP = 0.0, prevP = INFINITY;
    for (int k = 0; 2 * k + 1 <= h - 1; k++) {
        if (__ballot(!done) == 0) break;           // (wave-uniform)
        const int t0 = 2 * k, t1 = t0 + 1;
        double e1 = 0.0, e2 = 0.0, o1 = 0.0, o2 = 0.0;
        int i = 0;
        for (; i + t1 < h; i++) {
            const double u = x(i) - m1, v = x(off2 + i) - m2;
            e1 += u * (x(i + t0) - m1); o1 += u * (x(i + t1) - m1);
            e2 += v * (x(off2 + i + t0) - m2); o2 += v * (x(off2 + i + t1) - m2);
        }
        e1 += (x(i) - m1) * (x(i + t0) - m1);      // the even lag's last term, i = h - 1 - t0
        e2 += (x(off2 + i) - m2) * (x(off2 + i + t0) - m2);
        const double re = k == 0 ? 1.0 : 1.0 - (W - (e1 / (double)h + e2 / (double)h) / 2.0) / varp;
        const double ro = 1.0 - (W - (o1 / (double)h + o2 / (double)h) / 2.0) / varp;
        double P = re + ro;
        if (!done) {
            if (P <= 0.0) done = true;
            else { P = fmin(P, prevP); sumP += P; prevP = P; }
        }
    }
    const double tau = -1.0 + 2.0 * sumP;
    double rhat = NAN, ess = NAN, mcse = NAN;
    if (!bad) {
        rhat = sqrt(varp / W);
        ess = tau <= 0.0 ? a.cap : fmin((double)(2 * h) / tau, a.cap);
        mcse = sqrt(varp / ess);
    }
    const bool cell = mine && s < a.n_cells;
    if (cell && a.out) {
        double *o = a.out + 3 * (a.orig ? (int64_t)a.orig[s] : s);
        o[0] = rhat; o[1] = ess; o[2] = mcse;
    }
    if (mine && !cell) {
        double *o = a.scalars + 3 * (s - a.n_cells);
        o[0] = rhat; o[1] = ess; o[2] = mcse;
    }
    // the workgroup's summary over its cells: a constant series is counted and is in no other figure
    const bool ok = cell && !bad;
    double mx = ok ? rhat : -INFINITY, mn = ok ? ess : INFINITY;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { mx = fmax(mx, __shfl_xor(mx, off)); mn = fmin(mn, __shfl_xor(mn, off)); }
    const double high = (double)__popcll(__ballot(ok && rhat > a.rhat_cut)), low = (double)__popcll(__ballot(ok && ess < a.ess_cut));
    const double constant = (double)__popcll(__ballot(cell && bad));
    if (lane == 0) {
        double *p = a.partial + (int64_t)blockIdx.x * 5;
        p[0] = mx; p[1] = mn; p[2] = high; p[3] = low; p[4] = constant;
    }
}

// max, min and the counts (whole numbers in doubles: exact in any order) over the workgroups; NaN where no cell has a figure
__global__ __launch_bounds__(256) void k_diag_final(int nblocks, const double *partial, double draws, double *stats)
{
    __shared__ double red[5][4];
    const int tid = threadIdx.x;
    double v[5] = {-INFINITY, INFINITY, 0.0, 0.0, 0.0};
    for (int b = tid; b < nblocks; b += 256) {
        const double *p = partial + (int64_t)b * 5;
        v[0] = fmax(v[0], p[0]); v[1] = fmin(v[1], p[1]);
        v[2] += p[2]; v[3] += p[3]; v[4] += p[4];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        v[0] = fmax(v[0], __shfl_xor(v[0], off)); v[1] = fmin(v[1], __shfl_xor(v[1], off));
        v[2] += __shfl_xor(v[2], off); v[3] += __shfl_xor(v[3], off); v[4] += __shfl_xor(v[4], off);
    }
    if ((tid & 63) == 0)
#pragma unroll
        for (int q = 0; q < 5; q++) red[q][tid >> 6] = v[q];
    __syncthreads();
    if (tid == 0) {
        const double mx = fmax(fmax(red[0][0], red[0][1]), fmax(red[0][2], red[0][3]));
        const double mn = fmin(fmin(red[1][0], red[1][1]), fmin(red[1][2], red[1][3]));
        stats[0] = mx == -INFINITY ? NAN : mx;
        stats[1] = mn == INFINITY ? NAN : mn;
#pragma unroll
        for (int q = 2; q < 5; q++) stats[q] = (red[q][0] + red[q][1]) + (red[q][2] + red[q][3]);
        stats[5] = draws;
    }
}

}  // namespace

extern "C" int bdf_diag_create(bdf_ctx *ctx, int64_t n_cells, int n_scalars, int64_t capacity, bdf_diag **out)
{
    BDF_REQUIRE(ctx && out, BDF_ERR_ARG, "bdf_diag_create: NULL argument");
    BDF_REQUIRE(n_cells >= 1 && n_cells < (int64_t)0x7fffffff, BDF_ERR_ARG, "bdf_diag_create: n_cells=%lld must be in 1..2^31 - 2", (long long)n_cells);
    BDF_REQUIRE(n_scalars >= 0 && n_scalars <= 2, BDF_ERR_ARG, "bdf_diag_create: n_scalars=%d must be 0, 1 (sse) or 2 (sse, alpha)", n_scalars);
    BDF_REQUIRE(capacity >= 1 && capacity <= (int64_t)1 << 20, BDF_ERR_ARG, "bdf_diag_create: capacity=%lld must be in 1..2^20", (long long)capacity);
    BDF_HIP(hipSetDevice(ctx->device));
    std::unique_ptr<bdf_diag> d(new bdf_diag());
    d->n_cells = n_cells; d->n_scalars = n_scalars; d->capacity = capacity;
    const size_t doubles = (size_t)capacity * (size_t)(n_cells + n_scalars);
    if (d->plane_dev.alloc(doubles) != BDF_OK) {
        bdf_set_error("bdf_diag_create: no device memory for %lld draws of %lld cells and %d scalars (%zu bytes)", (long long)capacity,
                      (long long)n_cells, n_scalars, doubles * sizeof(double));
        return BDF_ERR_HIP;
    }
    if (int rc = d->stage_dev.alloc(4)) return rc;
    d->ctx = ctx;
    *out = d.release();
    return BDF_OK;
}

extern "C" int bdf_diag_destroy(bdf_diag *d)
{
    if (d) delete d;
    return BDF_OK;
}

extern "C" int bdf_diag_push(bdf_ctx *ctx, bdf_diag *d, const bdf_pairs *p, int D, const double *const *factors, double mean_value,
                             double alpha, const double *alpha_dev)
{
    BDF_REQUIRE(d != nullptr, BDF_ERR_ARG, "bdf_diag_push: NULL argument");
    DiagPushArgs a = {};
    const bool with_alpha = d->n_scalars == 2;
    int rc = pair_fill("bdf_diag_push", ctx, p, D, factors, mean_value, with_alpha, alpha, alpha_dev, a.pair);
    if (rc) return rc;
    BDF_REQUIRE(p->n == d->n_cells, BDF_ERR_ARG, "bdf_diag_push: the pairs hold %lld cells, the plane's rows %lld", (long long)p->n, (long long)d->n_cells);
    BDF_REQUIRE(d->draws < d->capacity, BDF_ERR_ARG, "bdf_diag_push: the plane is full (%lld draws)", (long long)d->capacity);
    int nblocks;
    if ((rc = pair_blocks("bdf_diag_push", "cells", p->n, &nblocks))) return rc;
    a.baseline = p->baseline_dev; a.link = p->link; a.link_r = p->link_r; a.with_alpha = with_alpha ? 1 : 0;
    a.row = d->plane_dev + (size_t)d->draws * (size_t)(d->n_cells + d->n_scalars);
    BDF_HIP(hipSetDevice(ctx->device));
    rc = launch_reduced(ctx, nblocks, a.partial, d->stage_dev.get(), [&] { BDF_BY_SHAPE(k_diag_push, p->n_modes, D, nblocks, ctx->stream, a); });
    if (rc) return rc;
    if (d->n_scalars)
        BDF_HIP(hipMemcpyAsync(a.row + d->n_cells, d->stage_dev.get(), (size_t)d->n_scalars * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    d->draws += 1;
    return BDF_OK;
}

extern "C" int bdf_diag_write(bdf_diag *d, int64_t draw, const double *values_dev)
{
    BDF_REQUIRE(d && values_dev, BDF_ERR_ARG, "bdf_diag_write: NULL argument");
    BDF_REQUIRE(draw >= 0 && draw < d->capacity, BDF_ERR_ARG, "bdf_diag_write: draw=%lld must be in 0..%lld", (long long)draw, (long long)d->capacity - 1);
    const size_t stride = (size_t)(d->n_cells + d->n_scalars);
    BDF_HIP(hipSetDevice(d->ctx->device));
    BDF_HIP(hipMemcpyAsync(d->plane_dev + (size_t)draw * stride, values_dev, stride * sizeof(double), hipMemcpyDeviceToDevice, d->ctx->stream));
    d->draws = std::max(d->draws, draw + 1);
    return BDF_OK;
}

extern "C" int bdf_diag_plane(const bdf_diag *d, double **dev_ptr, int64_t *draws)
{
    BDF_REQUIRE(d && dev_ptr && draws, BDF_ERR_ARG, "bdf_diag_plane: NULL argument");
    *dev_ptr = d->plane_dev; *draws = d->draws;
    return BDF_OK;
}

extern "C" int bdf_diag_compute(bdf_ctx *ctx, const bdf_diag *d, const int32_t *orig_dev, double rhat_cut, double ess_cut, double *out_dev,
                                double *stats_out)
{
    BDF_REQUIRE(ctx && d && stats_out, BDF_ERR_ARG, "bdf_diag_compute: NULL argument");
    BDF_REQUIRE(d->draws >= 4, BDF_ERR_ARG, "bdf_diag_compute: %lld draws: a split chain needs at least 4", (long long)d->draws);
    BDF_REQUIRE(rhat_cut == rhat_cut && ess_cut == ess_cut, BDF_ERR_ARG, "bdf_diag_compute: a cut is NaN");
    DiagArgs a = {};
    a.plane = d->plane_dev; a.stride = d->n_cells + d->n_scalars; a.n_cells = d->n_cells; a.total = a.stride;
    a.n = (int)d->draws; a.h = a.n / 2; a.off2 = a.n - a.h;
    a.cap = (double)(2 * a.h) * std::log10((double)(2 * a.h));
    a.rhat_cut = rhat_cut; a.ess_cut = ess_cut; a.orig = orig_dev; a.out = out_dev; a.scalars = stats_out + BDF_DIAG_STATS;
    const int nblocks = (int)((a.total + 63) / 64);
    void *sc;
    if (int rc = bdf_scratch(ctx, (size_t)nblocks * 5 * sizeof(double), &sc)) return rc;
    a.partial = (double *)sc;
    BDF_HIP(hipSetDevice(ctx->device));
    if (a.n <= BDF_DIAG_LDS_DRAWS) {
        const size_t lds = (size_t)a.n * 64 * sizeof(double);
        BDF_HIP(hipFuncSetAttribute((const void *)k_diag<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_diag<true>, dim3(nblocks), dim3(64), lds, ctx->stream, a);
    } else {
        hipLaunchKernelGGL(k_diag<false>, dim3(nblocks), dim3(64), 0, ctx->stream, a);
    }
    hipLaunchKernelGGL(k_diag_final, dim3(1), dim3(256), 0, ctx->stream, nblocks, (const double *)a.partial, (double)a.n, stats_out);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}
