// predict.h -- what the prediction kernels of k_predict.hip and the probit-link kernels of k_probit.hip share: the launch
// arguments, what a lane does for the pair it owns (everything of macau.jl:142-184 that is not the gather), the
// per-workgroup statistics and their fixed-order sum, which the kernels of k_lpd.hip, k_waic.hip and k_ordinal.hip leave their
// sums through as well.  File-local in every unit that includes it.
#pragma once
#include "bdf_common.h"
#include "probit.h"
#include "pg.h"

namespace {


struct PredArgs {
    int D, n_modes;
    int64_t n;
    const int32_t *ids;            // n_modes planes of n, 0-based
    const double *fac[BDF_MAX_MODES];
    double mean;
    const double *linear;          // nullable: per-pair baseline instead of mean (relation features: linear_values)
    const int32_t *orig;           // nullable: the pairs are stored sorted; orig[pair] = the caller's index (out, linear)
    int sorted_mode;               // the mode they are sorted by (-1: none)
    const double *values;
    double *out;                   // nullable: raw predictions
    double *avg, *sq;              // running state (update mode)
    int phase;                     // -1: predict only
    double count, clamp_lo, clamp_hi, cut;
    double *stats;
    double *partial;               // per-block statistics
    double link_r;                 // the count link's dispersion r (k_pg.hip)
};

__device__ inline double clampv(double x, double lo, double hi)
{
    if (lo > hi) return x;
    return x < lo ? lo : (x > hi ? hi : x);
}

// ---- what a lane does for the pair it owns: everything of macau.jl:142-184 that is not the gather -----------------------
// A group of 8 lanes computes the dot products of 8 consecutive pairs together (32 bytes of a factor row per lane) and then
// lane `sub` owns pair p0 + sub: ids, value and running state are read 8 consecutive pairs per group and instruction before
// the first gather is issued, and written back the same way.  (One lane per group doing the updates one after the other
// issued six times as many memory instructions as the gather itself, each with 8 active lanes 128 B apart.)
struct PairState {
    int64_t pm, po;                // storage position; the caller's index (out, linear)
    bool ok;
    double y, av, sv, base;
};

__device__ inline void pair_load(const PredArgs &a, int64_t p, PairState &s)
{
    s.ok = p < a.n;
    s.pm = s.ok ? p : a.n - 1;
    s.po = a.orig ? (int64_t)a.orig[s.pm] : s.pm;
    s.base = a.linear ? a.linear[s.po] : a.mean;
    s.y = a.phase >= 0 ? a.values[s.pm] : 0.0;
    s.av = 0.0; s.sv = 0.0;
    if (a.phase == 2) { s.av = a.avg[s.pm]; s.sv = a.sq[s.pm]; }
}

// LINK 1 (k_probit.hip): the prediction is the probability Phi(dot + base), before the clamp, the running state and the statistics;
// LINK 2 / 3 (k_pg.hip): the logistic probability / the count's mean r e^(dot + base)
template <int LINK = 0>
__device__ inline void pair_finish(const PredArgs &a, const PairState &s, double dot, double (&st)[4])
{
    if (!s.ok) return;
    double p = dot + s.base;
    if constexpr (LINK == 1) p = bdf_phi(p);
    if constexpr (LINK == 2) p = bdf_pg_logistic(p);
    if constexpr (LINK == 3) p = bdf_pg_count_mean(p, a.link_r);
    if (a.out) a.out[s.po] = p;
    if (a.phase >= 0) {
        double avg;
        if (a.phase == 0 || a.phase == 3) { avg = p; }
        else if (a.phase == 1) { avg = p; a.sq[s.pm] = p * p; }
        else { avg = (a.count * s.av + p) / (a.count + 1.0); a.sq[s.pm] = s.sv + p * p; }
        if (a.phase != 3) a.avg[s.pm] = avg;           // phase 3: statistics of this sample only, no running state
        const double ea = s.y - clampv(avg, a.clamp_lo, a.clamp_hi), ep = s.y - clampv(p, a.clamp_lo, a.clamp_hi);
        const bool label = s.y < a.cut;
        st[0] += ea * ea; st[1] += ep * ep;
        st[2] += (label == (avg < a.cut)) ? 1.0 : 0.0;
        st[3] += (label == (p < a.cut)) ? 1.0 : 0.0;
    }
}

// the workgroup's four sums, in fixed order, to partial[4 * block]; every lane of the workgroup calls it
__device__ inline void block_stats(double *partial, const double (&st)[4])
{
    __shared__ double red[4][256 / 64];
    const int tid = threadIdx.x;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        double v = st[q];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
        if ((tid & 63) == 0) red[q][tid >> 6] = v;
    }
    __syncthreads();
    if (tid < 4) partial[blockIdx.x * 4 + tid] = red[tid][0] + red[tid][1] + red[tid][2] + red[tid][3];
}

__device__ inline void block_stats(const PredArgs &a, const double (&st)[4]) { block_stats(a.partial, st); }

// fixed-order sum of the per-block statistics
__global__ __launch_bounds__(256) void k_predict_final(int nblocks, const double *partial, double *stats)
{
    __shared__ double red[4][4];
    const int tid = threadIdx.x;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int b = tid; b < nblocks; b += 256)
#pragma unroll
        for (int q = 0; q < 4; q++) v[q] += partial[b * 4 + q];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        double x = v[q];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off);
        if ((tid & 63) == 0) red[q][tid >> 6] = x;
    }
    __syncthreads();
    if (tid < 4) stats[tid] = red[tid][0] + red[tid][1] + red[tid][2] + red[tid][3];
}

// a launch of nblocks workgroups that leave their statistics through block_stats, and the fixed-order sum behind it: `partial`
// gets the context's scratch for them before launch() runs
template <class Launch>
int launch_reduced(bdf_ctx *ctx, int nblocks, double *&partial, double *stats, Launch launch)
{
    void *sc;
    int rc = bdf_scratch(ctx, (size_t)nblocks * 4 * sizeof(double), &sc);
    if (rc) return rc;
    partial = (double *)sc;
    launch();
    hipLaunchKernelGGL(k_predict_final, dim3(1), dim3(256), 0, ctx->stream, nblocks, (const double *)partial, stats);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}

int fill(const char *who, bdf_ctx *ctx, const bdf_pairs *p, int D, const double *const *factors, PredArgs &a)
{
    BDF_REQUIRE(ctx && p && factors, BDF_ERR_ARG, "%s: NULL argument", who);
    BDF_REQUIRE(D >= 1 && D <= BDF_MAX_D, BDF_ERR_ARG, "%s: num_latent=%d must be in 1..%d", who, D, BDF_MAX_D);
    memset(&a, 0, sizeof(a));
    a.D = D; a.n_modes = p->n_modes; a.n = p->n; a.ids = p->ids_dev; a.values = p->values_dev;
    for (int k = 0; k < p->n_modes; k++) {
        BDF_REQUIRE(factors[k] != nullptr, BDF_ERR_ARG, "%s: factors[%d] is NULL", who, k);
        a.fac[k] = factors[k];
    }
    a.phase = -1;
    a.linear = p->baseline_dev;
    a.orig = p->orig_dev;
    a.sorted_mode = p->orig_dev ? p->sorted_mode : -1;
    return BDF_OK;
}

}  // namespace
