// pair_gather.h -- what the kernels that walk a set of pairs 8 lanes to 8 consecutive pairs share (k_probit_draw, k_censored_draw,
// k_interval_draw, k_ordinal_mass, k_lpd, k_waic; DESIGN.md section 12 describes the shape once): the head of their launch
// arguments and its host-side fill, the lane prologue, the dot products of the 8 pairs as k_predict.hip's general kernel forms
// them, the group test, the latent draws' tail, the two launch geometries, the choice of a kernel variant by the shape and, for
// the two kernels that score a record by its kind, the record's arguments and log-likelihood.  File-local in every unit that
// includes it.
#pragma once
#include "bdf_common.h"
#include "lpd.h"
#include <algorithm>
#include <cmath>

namespace {

// ---- the launch arguments' head -----------------------------------------------------------------------------------------------
struct PairArgs {
    int D;
    int64_t n;
    const int32_t *ids;            // n_modes planes of n, 0-based
    const double *fac[BDF_MAX_MODES];
    const double *values;
    const int32_t *orig;           // nullable: the pairs are stored sorted; orig[pair] = the caller's index
    double mean, alpha;
    const double *alpha_dev;       // nullable: wins over alpha (read on the device when alpha was sampled there)
};

// the shared checks and fields, under the caller's name; with_alpha: the probit draw has none
int pair_fill(const char *who, bdf_ctx *ctx, const bdf_pairs *p, int D, const double *const *factors, double mean_value, bool with_alpha,
              double alpha, const double *alpha_dev, PairArgs &a)
{
    BDF_REQUIRE(ctx && p && factors, BDF_ERR_ARG, "%s: NULL argument", who);
    BDF_REQUIRE(D >= 1 && D <= BDF_MAX_D, BDF_ERR_ARG, "%s: num_latent=%d must be in 1..%d", who, D, BDF_MAX_D);
    BDF_REQUIRE(!with_alpha || alpha_dev || (alpha > 0.0 && std::isfinite(alpha)), BDF_ERR_ARG, "%s: alpha=%g must be positive and finite", who, alpha);
    a = {};
    a.D = D; a.n = p->n; a.ids = p->ids_dev; a.values = p->values_dev; a.orig = p->orig_dev;
    for (int k = 0; k < p->n_modes; k++) {
        BDF_REQUIRE(factors[k] != nullptr, BDF_ERR_ARG, "%s: factors[%d] is NULL", who, k);
        a.fac[k] = factors[k];
    }
    a.mean = mean_value; a.alpha = alpha; a.alpha_dev = alpha_dev;
    return BDF_OK;
}

// the entity of a relation's own random streams
inline uint32_t pair_entity(uint32_t rel_tag) { return 0x800000u | rel_tag; }

// ---- the two launch geometries: a workgroup is 32 groups of 8 lanes, a trip is 8 consecutive pairs ----------------------------
// the grid-stride form (k_probit_draw, k_censored_draw)
inline int pair_blocks_strided(int64_t n) { return (int)std::min<int64_t>(((n + 7) / 8 + 31) / 32, 8192); }

// one group per 8 pairs and no loop (the other four: around a loop the compiler spills, k_interval.hip)
int pair_blocks(const char *who, const char *what, int64_t n, int *nblocks, int64_t most = INT32_MAX)
{
    const int64_t nb = ((n + 7) / 8 + 31) / 32;
    BDF_REQUIRE(nb <= most, BDF_ERR_ARG, "%s: %lld %s are more than one launch covers", who, (long long)n, what);
    *nblocks = (int)nb;
    return BDF_OK;
}

__device__ __forceinline__ int64_t pair_trip() { return (int64_t)blockIdx.x * 32 + threadIdx.x / 8; }

// ---- the lane prologue --------------------------------------------------------------------------------------------------------
// Lane `sub` of the group that takes trip `trip` owns pair p0 + sub: pm is where it is stored, po the caller's index (what the
// random streams and the per-observation arrays in the caller's order are keyed by), my[k] its id in mode k.  A lane past the
// end (!ok) reads the last pair in its place, never past the arrays, and still takes part in the gather's shuffles.
template <int NM>
struct PairLane {
    int64_t p0, pm, po;
    int sub;
    bool ok;
    int32_t my[NM];
};

template <int NM>
__device__ __forceinline__ void pair_lane(const PairArgs &a, int64_t trip, PairLane<NM> &l)
{
    l.sub = threadIdx.x & 7;
    l.p0 = trip * 8;
    const int64_t p = l.p0 + l.sub;
    l.ok = p < a.n;
    l.pm = l.ok ? p : a.n - 1;
    l.po = a.orig ? (int64_t)a.orig[l.pm] : l.pm;
#pragma unroll
    for (int k = 0; k < NM; k++) l.my[k] = a.ids[(int64_t)k * a.n + l.pm];
}

__device__ __forceinline__ double pair_alpha(const PairArgs &a) { return a.alpha_dev ? *a.alpha_dev : a.alpha; }

// does any pair of this lane's group say x?  (Its 8 lanes are 8 neighbours of one wave, so the answer is the same in all of them.)
__device__ __forceinline__ unsigned group_any(bool x) { return (unsigned)(__ballot(x) >> (threadIdx.x & 56)) & 0xffu; }

// the tail of a latent draw: what the row kernels read as the observation's base, mean + (y - z), and the latent itself
__device__ __forceinline__ void latent_store(double *linear, double *z_out, int64_t po, double mean, double y, double z)
{
    linear[po] = mean + (y - z);
    if (z_out) z_out[po] = z;
}

// the dot products of the 8 consecutive pairs p0 .. p0 + 7 of a group of 8 lanes; my[k]: the id in mode k of pair p0 + sub.
// Returns, in lane sub, the dot product of pair p0 + sub.  VEC = 4: D a multiple of 4, NC 32-byte pieces of a row per lane
// (D <= 32: one, D <= 64: two); VEC = 1: any D, a lane takes elements sub, sub + 8, ...
template <int NM, int VEC, int NC>
__device__ __forceinline__ double group_dots(const double *const (&fac)[BDF_MAX_MODES], int D, int64_t n, int64_t p0, int sub,
                                             const int32_t (&my)[NM])
{
    constexpr int BATCH = (VEC == 1) ? 2 : (NC * NM <= 3 ? 4 : 2);
    double keep = 0.0;
#pragma unroll
    for (int u0 = 0; u0 < 8; u0 += BATCH) {
        if (p0 + u0 >= n) break;                       // group-uniform
        double s[BATCH];
        if constexpr (VEC == 4) {
            double4 f[BATCH][NM][NC];
#pragma unroll
            for (int u = 0; u < BATCH; u++)
#pragma unroll
                for (int k = 0; k < NM; k++) {
                    const double *row = fac[k] + (int64_t)__shfl(my[k], u0 + u, 8) * D;
#pragma unroll
                    for (int c = 0; c < NC; c++) {
                        const int e = sub * 4 + 32 * c;
                        f[u][k][c] = e < D ? *(const double4 *)(row + e) : double4{0.0, 0.0, 0.0, 0.0};
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
                    if (sub * 4 + 32 * c < D) acc += (p.x + p.y) + (p.z + p.w);
                }
                s[u] = acc;
            }
        } else {
#pragma unroll
            for (int u = 0; u < BATCH; u++) {
                const double *row[NM];
#pragma unroll
                for (int k = 0; k < NM; k++) row[k] = fac[k] + (int64_t)__shfl(my[k], u0 + u, 8) * D;
                double acc = 0.0;
                for (int e = sub; e < D; e += 8) {
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
    return keep;
}

template <int NM, int VEC, int NC>
__device__ __forceinline__ double pair_dot(const PairArgs &a, const PairLane<NM> &l)
{
    return group_dots<NM, VEC, NC>(a.fac, a.D, a.n, l.p0, l.sub, l.my);
}

// ---- records scored by their log-likelihood (k_lpd, k_waic) ---------------------------------------------------------------------
struct RecordArgs {
    PairArgs pair;
    const double *baseline;        // nullable: per-pair baseline instead of mean (the caller's order)
    const double2 *bounds;         // nullable; the caller's order: (lo, hi) per pair, lo == hi a measurement
    int link, phase;
    double *partial;               // per-block statistics
};

// One group of 8 lanes per 8 pairs.  The log-likelihood l of the record that this lane owns (lpd.h: the owning lane fetches its
// (lo, hi) with one 16-byte load) and pm, where its running state is stored; false in a lane that owns none.  SCALED (k_lpd under
// the per-row noise model, bdf_pairs_set_precision_scale): the record's precision is alpha scale[its id in mode scale_mode].
template <int NM, int VEC, int NC, bool SCALED = false>
__device__ __forceinline__ bool record_loglik(const RecordArgs &r, int64_t &pm, double &l, const double *scale = nullptr, int scale_mode = 0)
{
    double alpha = pair_alpha(r.pair);
    const int64_t trip = pair_trip();
    if (trip * 8 >= r.pair.n) return false;
    PairLane<NM> ln;
    pair_lane(r.pair, trip, ln);
    const double y = r.pair.values[ln.pm];
    const double base = r.baseline ? r.baseline[ln.po] : r.pair.mean;
    double lo = y, hi = y;
    if (r.bounds) { const double2 bd = r.bounds[ln.po]; lo = bd.x; hi = bd.y; }
    const double m = pair_dot<NM, VEC, NC>(r.pair, ln) + base;
    if (!ln.ok) return false;
    pm = ln.pm;
    if constexpr (SCALED) {
        int32_t id = ln.my[0];
#pragma unroll
        for (int k = 1; k < NM; k++)
            if (scale_mode == k) id = ln.my[k];
        alpha *= scale[id];
    }
    l = bdf_lpd_record(r.link, y, m, lo, hi, alpha);
    return true;
}

// the checks and fields of an update over such records (phase 0: statistics only, 1: start the running state, 2: fold into it)
int record_fill(const char *who, bdf_ctx *ctx, const bdf_pairs *p, const double *bounds_dev, const double *baseline, int D,
                const double *const *factors, double mean_value, double alpha, const double *alpha_dev, int phase, const double *stats_out,
                RecordArgs &r, int *nblocks)
{
    BDF_REQUIRE(ctx && p && factors && stats_out, BDF_ERR_ARG, "%s: NULL argument", who);
    BDF_REQUIRE(p->link <= 1, BDF_ERR_ARG, "%s: pairs with the logistic or the count link are not scored yet", who);
    BDF_REQUIRE(!(bounds_dev && p->link == 1), BDF_ERR_ARG, "%s: pairs with the probit link take no bounds", who);
    BDF_REQUIRE(((uintptr_t)bounds_dev & 15) == 0, BDF_ERR_ARG, "%s: bounds_dev must be aligned to 16 bytes", who);
    BDF_REQUIRE(phase >= 0 && phase <= 2, BDF_ERR_ARG, "%s: phase must be 0, 1 or 2", who);
    int rc = pair_fill(who, ctx, p, D, factors, mean_value, true, alpha, alpha_dev, r.pair);
    if (rc) return rc;
    r.baseline = baseline; r.bounds = (const double2 *)bounds_dev; r.link = p->link; r.phase = phase;
    return pair_blocks(who, "pairs", p->n, nblocks);
}

// the kernel variant by the number of modes, D % 4 and D <= 32, as launch_predict of k_predict.hip chooses it
#define BDF_BY_SHAPE(KERNEL, n_modes, D, nblocks, stream, args)                                                             \
    do {                                                                                                                     \
        const bool vec__ = ((D) & 3) == 0;                                                                                   \
        const int nc__ = (D) <= 32 ? 1 : 2;                                                                                  \
        if ((n_modes) == 2) {                                                                                                \
            if (!vec__) hipLaunchKernelGGL((KERNEL<2, 1, 1>), dim3(nblocks), dim3(256), 0, stream, args);                    \
            else if (nc__ == 1) hipLaunchKernelGGL((KERNEL<2, 4, 1>), dim3(nblocks), dim3(256), 0, stream, args);            \
            else hipLaunchKernelGGL((KERNEL<2, 4, 2>), dim3(nblocks), dim3(256), 0, stream, args);                           \
        } else if ((n_modes) == 3) {                                                                                         \
            if (!vec__) hipLaunchKernelGGL((KERNEL<3, 1, 1>), dim3(nblocks), dim3(256), 0, stream, args);                    \
            else if (nc__ == 1) hipLaunchKernelGGL((KERNEL<3, 4, 1>), dim3(nblocks), dim3(256), 0, stream, args);            \
            else hipLaunchKernelGGL((KERNEL<3, 4, 2>), dim3(nblocks), dim3(256), 0, stream, args);                           \
        } else {                                                                                                             \
            if (!vec__) hipLaunchKernelGGL((KERNEL<4, 1, 1>), dim3(nblocks), dim3(256), 0, stream, args);                    \
            else if (nc__ == 1) hipLaunchKernelGGL((KERNEL<4, 4, 1>), dim3(nblocks), dim3(256), 0, stream, args);            \
            else hipLaunchKernelGGL((KERNEL<4, 4, 2>), dim3(nblocks), dim3(256), 0, stream, args);                           \
        }                                                                                                                    \
    } while (0)

}  // namespace
