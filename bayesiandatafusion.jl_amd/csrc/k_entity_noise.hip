// k_entity_noise.hip -- a noise precision per row of one entity of a relation: a cell whose id in that
// entity's mode is j counts with precision alpha tau_j, tau_j ~ Gamma(shape, rate) a priori, and given the rows
//   tau_j ~ Gamma(shape + n_j / 2, rate + alpha S_j / 2),  S_j = sum of e_k^2 over the n_j cells of row j, e_k = y_k - (udot_k + mean).
//
// bdf_entity_noise_draw makes two launches on the context's stream.
//   1. k_noise_resid: the lane prologue, gather and dot product of pair_gather.h (8 lanes per pair, no grid-stride loop, as
//      k_robust.hip); the lane that owns the pair writes e^2 to precision_out at the caller's index.
//   2. k_noise_rows<W>: one group of W lanes per row of the mode's CSR (rowptr, perm), rows taken in the relation's degree order.  The
//      group reads precision_out[perm[entry]] -- a streaming read of perm, a gather of 8 bytes per cell -- and sums it in the order
//      entity_noise.h writes down; its first lane draws G by Marsaglia-Tsang on the row's own two streams (BDF_P_NOISE_N /
//      BDF_P_NOISE_U, entity 0x800000 | rel_tag, row j) and forms tau_j; the group writes tau_j to tau_out[j] and over the e^2 of its
//      own entries, which is what the row kernels read as TermDev::weight.  Every entry belongs to one row: nothing races.
//      W = 8 when nnz / N <= 32, else 64, from the shape alone.  With wsse_out: sum_j tau_j S_j through per-workgroup sums in the
//      context's scratch and a one-workgroup pass over them, both in a fixed order.
//
// No scratch memory, 32 bytes of LDS, plain vector stores, no floating-point atomics.
#include "bdf_common.h"
#include "entity_noise.h"
#include "pair_gather.h"

namespace {

struct NoiseResidArgs {
    PairArgs pair;
    double *sq;                    // e^2, the caller's order
};

// (Registers: the gather's BATCH x NM x NC double4 and one subtraction; k_robust_draw's bounds.)
template <int NM, int VEC, int NC>
__global__ __launch_bounds__(256, (VEC == 4 && NM * NC >= 8) ? 2 : 3) void k_noise_resid(NoiseResidArgs a)
{
    const int64_t trip = pair_trip();
    if (trip * 8 >= a.pair.n) return;              // (group-uniform; no barrier follows)
    PairLane<NM> l;
    pair_lane(a.pair, trip, l);
    const double y = a.pair.values[l.pm];
    // the prediction as bdf_predict forms it, udot + mean, then the residual: the same bits as y - bdf_predict's output
    const double e = y - (pair_dot<NM, VEC, NC>(a.pair, l) + a.pair.mean);
    if (l.ok) a.sq[l.po] = e * e;
}

struct NoiseRowsArgs {
    int64_t N;                     // rows of the mode
    const int64_t *rowptr;         // N + 1
    const int32_t *perm;           // nnz: the caller's index of every entry, mode order
    const int32_t *order;          // N: the rows by falling degree
    double alpha;
    const double *alpha_dev;       // nullable: wins over alpha
    double shape, rate;
    uint64_t seed;
    uint32_t sweep, entity;        // pair_entity(rel_tag)
    double *tau;                   // N
    double *precision;             // in: e^2, out: tau of the entry's row; the caller's order
    double *partial;               // nullable: one sum per workgroup
};

template <int W>
__global__ __launch_bounds__(256) void k_noise_rows(NoiseRowsArgs a)
{
    __shared__ double red[4];
    const int tid = threadIdx.x, lane = tid & (W - 1);
    const int64_t g = (int64_t)blockIdx.x * (256 / W) + tid / W;
    const bool live = g < a.N;                     // (the same in every lane of a group)
    double term = 0.0;
    if (live) {
        const int64_t j = a.order[g];
        const int64_t begin = a.rowptr[j], end = a.rowptr[j + 1];
        double v = 0.0;
        for (int64_t q = begin + lane; q < end; q += W) v += a.precision[a.perm[q]];
#pragma unroll
        for (int off = W / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off);
        double tau = 0.0;
        if (lane == 0) {
            const double G = bdf_gamma_on(BDF_P_NOISE_N, BDF_P_NOISE_U, a.seed, a.sweep, a.entity, (uint64_t)j,
                                          bdf_entity_noise_shape(a.shape, (long long)(end - begin)));
            tau = bdf_entity_noise_tau(G, a.rate, a.alpha_dev ? *a.alpha_dev : a.alpha, v);
            a.tau[j] = tau;
            term = bdf_entity_noise_term(tau, v);
        }
        tau = __shfl(tau, 0, W);
        for (int64_t q = begin + lane; q < end; q += W) a.precision[a.perm[q]] = tau;
    }
    if (a.partial == nullptr) return;              // (the same in every lane of the launch)
    double s = term;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) a.partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// the workgroups' sums added in a fixed order
__global__ __launch_bounds__(256) void k_noise_final(int nblocks, const double *partial, double *out)
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

}  // namespace

extern "C" int bdf_entity_noise_draw(bdf_ctx *ctx, const bdf_rel *rel, int mode, const bdf_pairs *train, int D, const double *const *factors,
                                     double mean_value, double alpha, const double *alpha_dev, double shape, double rate, uint32_t rel_tag,
                                     double *tau_out, double *precision_out, double *wsse_out)
{
    const char *who = "bdf_entity_noise_draw";
    BDF_REQUIRE(ctx && rel && train && tau_out && precision_out, BDF_ERR_ARG, "%s: NULL argument", who);
    BDF_REQUIRE(mode >= 0 && mode < rel->n_modes, BDF_ERR_ARG, "%s: mode=%d must be in 0..%d", who, mode, rel->n_modes - 1);
    BDF_REQUIRE(!rel->sharded, BDF_ERR_ARG, "%s: a relation created with a layout holds only its own rows' cells (one rank only)", who);
    BDF_REQUIRE(train->n_modes == rel->n_modes && train->n == rel->nnz, BDF_ERR_ARG,
                "%s: train (%lld pairs, %d modes) must be the relation's own cells (%lld, %d modes), in its order", who, (long long)train->n,
                train->n_modes, (long long)rel->nnz, rel->n_modes);
    BDF_REQUIRE(shape > 0.0 && std::isfinite(shape) && rate > 0.0 && std::isfinite(rate), BDF_ERR_ARG,
                "%s: shape=%g and rate=%g must be positive and finite", who, shape, rate);
    NoiseResidArgs ra = {};
    int rc = pair_fill(who, ctx, train, D, factors, mean_value, true, alpha, alpha_dev, ra.pair);
    if (rc) return rc;
    ra.sq = precision_out;
    int nblocks;
    if ((rc = pair_blocks(who, "observations", train->n, &nblocks))) return rc;
    const bdf_mode_index &ix = rel->idx[mode];
    const int64_t N = rel->dims[mode];
    // the group width from the shape alone: a row of the mean degree is one trip of 8 lanes up to 32 cells, of 64 beyond
    const int W = (N > 0 && rel->nnz > 32 * N) ? 64 : 8;
    const int64_t nb_rows = (N + 256 / W - 1) / (256 / W);
    BDF_REQUIRE(nb_rows <= INT32_MAX, BDF_ERR_ARG, "%s: %lld rows are more than one launch covers", who, (long long)N);
    BDF_HIP(hipSetDevice(ctx->device));
    NoiseRowsArgs a = {};
    a.N = N; a.rowptr = ix.rowptr_dev; a.perm = ix.perm_dev; a.order = ix.order_dev;
    a.alpha = alpha; a.alpha_dev = alpha_dev; a.shape = shape; a.rate = rate;
    a.seed = ctx->seed; a.sweep = ctx->sweep_host; a.entity = pair_entity(rel_tag);
    a.tau = tau_out; a.precision = precision_out;
    if (wsse_out) {
        void *sc;
        if ((rc = bdf_scratch(ctx, (size_t)std::max<int64_t>(nb_rows, 1) * sizeof(double), &sc))) return rc;
        a.partial = (double *)sc;
    }
    if (nblocks > 0) BDF_BY_SHAPE(k_noise_resid, train->n_modes, D, nblocks, ctx->stream, ra);
    if (nb_rows > 0) {
        if (W == 8) hipLaunchKernelGGL(k_noise_rows<8>, dim3((unsigned)nb_rows), dim3(256), 0, ctx->stream, a);
        else hipLaunchKernelGGL(k_noise_rows<64>, dim3((unsigned)nb_rows), dim3(256), 0, ctx->stream, a);
    }
    if (wsse_out) hipLaunchKernelGGL(k_noise_final, dim3(1), dim3(256), 0, ctx->stream, (int)nb_rows, (const double *)a.partial, wsse_out);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}
