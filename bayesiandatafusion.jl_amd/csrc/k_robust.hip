// k_robust.hip -- the robust (Student-t) noise model and observation weights: an observation counts with
// precision alpha omega_k.  With known weights omega is the caller's; under the Student-t model it is the scale mixture's latent,
// omega_k ~ Gamma(nu / 2, rate nu / 2), drawn here given the rows: omega_k = 2 G_k / (nu + alpha e_k^2), e_k = y_k - mean - udot_k.
//
// bdf_robust_draw: the lane prologue, gather and dot product of pair_gather.h and, in the lane that owns the pair, one gamma variate
// by Marsaglia-Tsang on the observation's own two streams (BDF_P_ROBUST_N / BDF_P_ROBUST_U: bdf_gamma's streams are sample_alpha's
// at variate 0).  It writes omega in the caller's order -- what the row kernels read as TermDev::weight -- and, when asked, leaves
// sum omega e^2 for sample_alpha: per-workgroup sums to the context's scratch and a one-workgroup pass over them, both in a fixed
// order.  bdf_pairs_weighted_sse: the same kernel without the draw, on the caller's weights.
//
// One group of 8 lanes per 8 pairs and no grid-stride loop (every lane reaches the sum's barrier).  No scratch memory, 32 bytes of
// LDS, plain vector stores, no floating-point atomics.
#include "bdf_common.h"
#include "robust.h"
#include "pair_gather.h"

namespace {

struct RobustArgs {
    PairArgs pair;
    const double *weights;         // bdf_pairs_weighted_sse: the caller's order
    double nu;
    uint64_t seed;
    uint32_t sweep, entity;        // pair_entity(rel_tag)
    double *precision;             // bdf_robust_draw: omega, the caller's order
    double *partial;               // nullable: one sum per workgroup
};

template <int NM, int VEC, int NC, bool DRAW>
__device__ __forceinline__ void robust_body(const RobustArgs &a)
{
    __shared__ double red[4];
    const int tid = threadIdx.x;
    const int64_t trip = pair_trip();
    double term = 0.0;
    if (trip * 8 < a.pair.n) {
        PairLane<NM> l;
        pair_lane(a.pair, trip, l);
        const double y = a.pair.values[l.pm];
        const double e = (y - a.pair.mean) - pair_dot<NM, VEC, NC>(a.pair, l);
        if (l.ok) {
            double w;
            if constexpr (DRAW) {
                // the observation's own gamma variate: the streams are keyed by the caller's index, not by where the pair is stored
                const double G = bdf_gamma_on(BDF_P_ROBUST_N, BDF_P_ROBUST_U, a.seed, a.sweep, a.entity, (uint64_t)l.po, 0.5 * (a.nu + 1.0));
                w = bdf_robust_omega(G, a.nu, pair_alpha(a.pair), e);
                a.precision[l.po] = w;
            } else {
                w = a.weights[l.po];
            }
            term = bdf_robust_term(w, e);
        }
    }
    if (a.partial == nullptr) return;          // (the same in every lane of the launch)
    double v = term;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) a.partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// (Registers: the gather's BATCH x NM x NC double4 beside the owner's Philox / Box-Muller / log arithmetic; k_censored_draw's
// bounds hold it free of scratch: DESIGN.md section 18 has the listing.)
template <int NM, int VEC, int NC>
__global__ __launch_bounds__(256, (VEC == 4 && NM * NC >= 8) ? 2 : 3) void k_robust_draw(RobustArgs a)
{
    robust_body<NM, VEC, NC, true>(a);
}

template <int NM, int VEC, int NC>
__global__ __launch_bounds__(256, (VEC == 4 && NM * NC >= 8) ? 2 : 3) void k_weighted_sse(RobustArgs a)
{
    robust_body<NM, VEC, NC, false>(a);
}

// the workgroups' sums added in a fixed order
__global__ __launch_bounds__(256) void k_robust_final(int nblocks, const double *partial, double *out)
{
    __shared__ double red[4];
    const int tid = threadIdx.x;
    double v = 0.0;
    for (int b = tid; b < nblocks; b += 256) v += partial[b];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) *out = (red[0] + red[1]) + (red[2] + red[3]);
}

int launch_robust(const char *who, bdf_ctx *ctx, const bdf_pairs *p, int D, RobustArgs &a, bool draw, double *sum_out)
{
    int nblocks, rc;
    if ((rc = pair_blocks(who, "observations", p->n, &nblocks))) return rc;
    BDF_HIP(hipSetDevice(ctx->device));
    if (sum_out) {
        void *sc;
        if ((rc = bdf_scratch(ctx, (size_t)std::max(nblocks, 1) * sizeof(double), &sc))) return rc;
        a.partial = (double *)sc;
    }
    if (nblocks > 0) {
        if (draw) BDF_BY_SHAPE(k_robust_draw, p->n_modes, D, nblocks, ctx->stream, a);
        else BDF_BY_SHAPE(k_weighted_sse, p->n_modes, D, nblocks, ctx->stream, a);
    }
    if (sum_out) hipLaunchKernelGGL(k_robust_final, dim3(1), dim3(256), 0, ctx->stream, nblocks, (const double *)a.partial, sum_out);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}

}  // namespace

extern "C" int bdf_robust_draw(bdf_ctx *ctx, const bdf_pairs *train, int D, const double *const *factors, double mean_value, double alpha,
                               const double *alpha_dev, double nu, uint32_t rel_tag, double *precision_out, double *wsse_out)
{
    BDF_REQUIRE(precision_out, BDF_ERR_ARG, "bdf_robust_draw: NULL argument");
    BDF_REQUIRE(nu >= 1.0 && std::isfinite(nu), BDF_ERR_ARG, "bdf_robust_draw: nu=%g must be at least 1 and finite", nu);
    RobustArgs a = {};
    int rc = pair_fill("bdf_robust_draw", ctx, train, D, factors, mean_value, true, alpha, alpha_dev, a.pair);
    if (rc) return rc;
    a.nu = nu;
    a.seed = ctx->seed; a.sweep = ctx->sweep_host; a.entity = pair_entity(rel_tag);
    a.precision = precision_out;
    return launch_robust("bdf_robust_draw", ctx, train, D, a, true, wsse_out);
}

extern "C" int bdf_pairs_weighted_sse(bdf_ctx *ctx, const bdf_pairs *pairs, int D, const double *const *factors, double mean_value,
                                      const double *weights, double *out)
{
    BDF_REQUIRE(weights && out, BDF_ERR_ARG, "bdf_pairs_weighted_sse: NULL argument");
    RobustArgs a = {};
    int rc = pair_fill("bdf_pairs_weighted_sse", ctx, pairs, D, factors, mean_value, false, 0.0, nullptr, a.pair);
    if (rc) return rc;
    a.weights = weights;
    return launch_robust("bdf_pairs_weighted_sse", ctx, pairs, D, a, false, out);
}
