// k_bias.hip -- row and column biases of a relation's entities: a cell whose id in a biased mode m is j
// is shifted by b^m_j,
//   y_k = mean + sum over the biased modes of b^m_(id_m(k)) + udot_k + eps_k,   b^m_j ~ N(0, 1 / lambda_m),  lambda_m ~ Gamma(shape_m, rate_m).
//
// bdf_bias_draw makes, on the context's stream:
//   1. k_bias_resid: the lane prologue, gather and dot product of pair_gather.h (8 lanes per 8 pairs, no grid-stride loop, as
//      k_noise_resid); the lane that owns the pair writes e = y - (udot + mean) to the residual scratch at the caller's index.  Once
//      per relation, however many modes are biased.
//   2. per biased mode m, in rising order, k_bias_rows<W>: one group of W lanes per row of the mode's CSR (rowptr, perm, colidx),
//      rows taken in the relation's degree order.  The group reads e[perm[entry]] -- a streaming read of perm, a gather of 8 bytes
//      per cell -- takes off the current bias of every OTHER biased mode (the entry's id in that mode is in the CSR's own colidx
//      plane, read streaming; the bias vectors are small and stay in cache) and sums in the order bias.h writes down; its first
//      lane draws the row's normal and forms b^m_j.  W = 8 when nnz <= 32 N, else 64, from the shape alone.  Every workgroup
//      leaves its sum of b^2 in the context's scratch, and
//   3. k_bias_lambda, one workgroup, adds those in a fixed order and draws lambda_m on the device.
//   4. k_bias_base: linear_out[k] = mean + the biases of cell k in rising mode order, element-wise over the training pairs.
// bdf_bias_baseline is launch 4 over any pairs.
//
// No scratch memory, 32 bytes of LDS (the reductions), plain vector stores, no floating-point atomics.
#include "bdf_common.h"
#include "bias.h"
#include "pair_gather.h"

namespace {

struct BiasResidArgs {
    PairArgs pair;
    double *resid;                 // e, the caller's order
};

// (Registers: the gather's BATCH x NM x NC double4 and one subtraction; k_noise_resid's bounds.)
template <int NM, int VEC, int NC>
__global__ __launch_bounds__(256, (VEC == 4 && NM * NC >= 8) ? 2 : 3) void k_bias_resid(BiasResidArgs a)
{
    const int64_t trip = pair_trip();
    if (trip * 8 >= a.pair.n) return;              // (group-uniform; no barrier follows)
    PairLane<NM> l;
    pair_lane(a.pair, trip, l);
    const double y = a.pair.values[l.pm];
    // the prediction as bdf_predict forms it, udot + mean, then the residual: the same bits as y - bdf_predict's output
    const double e = y - (pair_dot<NM, VEC, NC>(a.pair, l) + a.pair.mean);
    if (l.ok) a.resid[l.po] = e;
}

struct BiasRowsArgs {
    int64_t N, nnz;                // rows of the mode; the plane stride of colidx
    const int64_t *rowptr;         // N + 1
    const int32_t *perm;           // nnz: the caller's index of every entry, mode order
    const int32_t *colidx;         // n_modes - 1 planes of nnz: the entry's ids in the other modes, rising
    const int32_t *order;          // N: the rows by falling degree
    const double *resid;           // e, the caller's order
    int n_other;                   // the other biased modes, rising
    int plane[BDF_MAX_MODES];      // ... their plane of colidx
    const double *other[BDF_MAX_MODES];   // ... and their bias vectors
    double alpha;
    const double *alpha_dev;       // nullable: wins over alpha
    const double *lambda;          // dev scalar: this mode's current precision
    uint64_t seed;
    uint32_t sweep, entity;        // pair_entity(rel_tag)
    int mode;                      // 0-based: which normal of the row's stream
    double *bias;                  // N
    double *partial;               // one sum of b^2 per workgroup
};

template <int W>
__global__ __launch_bounds__(256) void k_bias_rows(BiasRowsArgs a)
{
    __shared__ double red[4];
    const int tid = threadIdx.x, lane = tid & (W - 1);
    const int64_t g = (int64_t)blockIdx.x * (256 / W) + tid / W;
    double term = 0.0;
    if (g < a.N) {                                 // (the same in every lane of a group)
        const int64_t j = a.order[g];
        const int64_t begin = a.rowptr[j], end = a.rowptr[j + 1];
        double v = 0.0;
        for (int64_t q = begin + lane; q < end; q += W) {
            double r = a.resid[a.perm[q]];
            for (int o = 0; o < a.n_other; o++) r = bdf_bias_resid(r, a.other[o][a.colidx[(int64_t)a.plane[o] * a.nnz + q]]);
            v += r;
        }
#pragma unroll
        for (int off = W / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off);
        if (lane == 0) {
            const double z = bdf_normal(a.seed, a.sweep, BDF_P_BIAS, a.entity, (uint64_t)j, a.mode);
            const double b = bdf_bias_row(v, (long long)(end - begin), a.alpha_dev ? *a.alpha_dev : a.alpha, *a.lambda, z);
            a.bias[j] = b;
            term = b * b;
        }
    }
    double s = term;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) a.partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// the workgroups' sums of b^2 added in a fixed order, then lambda_m from its conditional
__global__ __launch_bounds__(256) void k_bias_lambda(int nblocks, const double *partial, int64_t N, double shape, double rate, uint64_t seed,
                                                     uint32_t sweep, uint32_t entity, int mode, double *lambda)
{
    __shared__ double red[4];
    const int tid = threadIdx.x;
    double v = 0.0;
    for (int b = tid; b < nblocks; b += 256) v += partial[b];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) {
        const double G = bdf_gamma_on(BDF_P_BIAS_N, BDF_P_BIAS_U, seed, sweep, entity, (uint64_t)mode, bdf_bias_lambda_shape(shape, (long long)N));
        *lambda = bdf_bias_lambda(G, rate, (red[0] + red[1]) + (red[2] + red[3]));
    }
}

struct BiasBaseArgs {
    int64_t n;
    const int32_t *ids;            // n_modes planes of n, 0-based, storage order
    const int32_t *orig;           // nullable: storage position -> the caller's index
    int n_bias;
    int mode[BDF_MAX_MODES];       // rising
    const double *bias[BDF_MAX_MODES];
    double mean;
    double *out;                   // the caller's order
};

__global__ __launch_bounds__(256) void k_bias_base(BiasBaseArgs a)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= a.n) return;
    double base = a.mean;
    for (int t = 0; t < a.n_bias; t++) base += a.bias[t][a.ids[(int64_t)a.mode[t] * a.n + p]];
    a.out[a.orig ? (int64_t)a.orig[p] : p] = base;
}

// the terms' checks, shared by both entry points: modes distinct and in range (the terms are then taken in rising mode order,
// whichever way they were listed), shape and rate positive and finite, the buffers there
int bias_terms(const char *who, int n_modes, int n_bias, const bdf_bias_term *terms, bool with_prior, const bdf_bias_term **sorted)
{
    BDF_REQUIRE(n_bias >= 1 && n_bias <= n_modes && terms, BDF_ERR_ARG, "%s: n_bias=%d must be in 1..%d, with its terms", who, n_bias, n_modes);
    int n = 0;
    for (int m = 0; m < n_modes; m++)
        for (int t = 0; t < n_bias; t++)
            if (terms[t].mode == m) {
                BDF_REQUIRE(n == 0 || sorted[n - 1]->mode != m, BDF_ERR_ARG, "%s: mode %d is listed twice", who, m);
                sorted[n++] = terms + t;
            }
    for (int t = 0; t < n_bias; t++) {
        BDF_REQUIRE(terms[t].mode >= 0 && terms[t].mode < n_modes, BDF_ERR_ARG, "%s: term %d: mode=%d must be in 0..%d", who, t, terms[t].mode, n_modes - 1);
        BDF_REQUIRE(terms[t].bias != nullptr, BDF_ERR_ARG, "%s: term %d has no bias buffer", who, t);
        if (!with_prior) continue;
        BDF_REQUIRE(terms[t].lambda != nullptr, BDF_ERR_ARG, "%s: term %d has no lambda buffer", who, t);
        BDF_REQUIRE(terms[t].shape > 0.0 && std::isfinite(terms[t].shape) && terms[t].rate > 0.0 && std::isfinite(terms[t].rate), BDF_ERR_ARG,
                    "%s: term %d: shape=%g and rate=%g must be positive and finite", who, t, terms[t].shape, terms[t].rate);
    }
    BDF_REQUIRE(n == n_bias, BDF_ERR_ARG, "%s: a mode is listed twice", who);
    return BDF_OK;
}

int launch_base(const char *who, bdf_ctx *ctx, const bdf_pairs *p, int n_bias, const bdf_bias_term *const *sorted, double mean, double *out)
{
    const int64_t nb = (p->n + 255) / 256;
    BDF_REQUIRE(nb <= INT32_MAX, BDF_ERR_ARG, "%s: %lld pairs are more than one launch covers", who, (long long)p->n);
    if (nb == 0) return BDF_OK;
    BiasBaseArgs a = {};
    a.n = p->n; a.ids = p->ids_dev; a.orig = p->orig_dev; a.n_bias = n_bias; a.mean = mean; a.out = out;
    for (int t = 0; t < n_bias; t++) { a.mode[t] = sorted[t]->mode; a.bias[t] = sorted[t]->bias; }
    hipLaunchKernelGGL(k_bias_base, dim3((unsigned)nb), dim3(256), 0, ctx->stream, a);
    return BDF_OK;
}

}  // namespace

extern "C" int bdf_bias_draw(bdf_ctx *ctx, const bdf_rel *rel, const bdf_pairs *train, int D, const double *const *factors, double mean_value,
                             double alpha, const double *alpha_dev, uint32_t rel_tag, int n_bias, const bdf_bias_term *terms, double *resid_scratch,
                             double *linear_out)
{
    const char *who = "bdf_bias_draw";
    BDF_REQUIRE(ctx && rel && train && terms && resid_scratch && linear_out, BDF_ERR_ARG, "%s: NULL argument", who);
    BDF_REQUIRE(!rel->sharded, BDF_ERR_ARG, "%s: a relation created with a layout holds only its own rows' cells (one rank only)", who);
    BDF_REQUIRE(train->n_modes == rel->n_modes && train->n == rel->nnz, BDF_ERR_ARG,
                "%s: train (%lld pairs, %d modes) must be the relation's own cells (%lld, %d modes), in its order", who, (long long)train->n,
                train->n_modes, (long long)rel->nnz, rel->n_modes);
    const bdf_bias_term *sorted[BDF_MAX_MODES];
    int rc = bias_terms(who, rel->n_modes, n_bias, terms, true, sorted);
    if (rc) return rc;
    BiasResidArgs ra = {};
    if ((rc = pair_fill(who, ctx, train, D, factors, mean_value, true, alpha, alpha_dev, ra.pair))) return rc;
    ra.resid = resid_scratch;
    int nblocks;
    if ((rc = pair_blocks(who, "observations", train->n, &nblocks))) return rc;
    int64_t most = 1;
    for (int t = 0; t < n_bias; t++) {
        const int64_t N = rel->dims[sorted[t]->mode];
        const int W = (N > 0 && rel->nnz > 32 * N) ? 64 : 8;
        const int64_t nb = (N + 256 / W - 1) / (256 / W);
        BDF_REQUIRE(nb <= INT32_MAX, BDF_ERR_ARG, "%s: %lld rows are more than one launch covers", who, (long long)N);
        most = std::max(most, nb);
    }
    void *sc;
    if ((rc = bdf_scratch(ctx, (size_t)most * sizeof(double), &sc))) return rc;
    BDF_HIP(hipSetDevice(ctx->device));
    if (nblocks > 0) BDF_BY_SHAPE(k_bias_resid, train->n_modes, D, nblocks, ctx->stream, ra);
    for (int t = 0; t < n_bias; t++) {
        const int mode = sorted[t]->mode;
        const bdf_mode_index &ix = rel->idx[mode];
        const int64_t N = rel->dims[mode];
        // the group width from the shape alone: a row of the mean degree is one trip of 8 lanes up to 32 cells, of 64 beyond
        const int W = (N > 0 && rel->nnz > 32 * N) ? 64 : 8;
        const int64_t nb = (N + 256 / W - 1) / (256 / W);
        BiasRowsArgs a = {};
        a.N = N; a.nnz = rel->nnz; a.rowptr = ix.rowptr_dev; a.perm = ix.perm_dev; a.colidx = ix.colidx_dev; a.order = ix.order_dev;
        a.resid = resid_scratch;
        for (int o = 0; o < n_bias; o++) {
            if (o == t) continue;
            const int om = sorted[o]->mode;
            a.plane[a.n_other] = om < mode ? om : om - 1;       // (colidx lists the other modes in rising order)
            a.other[a.n_other] = sorted[o]->bias;
            a.n_other++;
        }
        a.alpha = alpha; a.alpha_dev = alpha_dev; a.lambda = sorted[t]->lambda;
        a.seed = ctx->seed; a.sweep = ctx->sweep_host; a.entity = pair_entity(rel_tag); a.mode = mode;
        a.bias = sorted[t]->bias; a.partial = (double *)sc;
        if (nb > 0) {
            if (W == 8) hipLaunchKernelGGL(k_bias_rows<8>, dim3((unsigned)nb), dim3(256), 0, ctx->stream, a);
            else hipLaunchKernelGGL(k_bias_rows<64>, dim3((unsigned)nb), dim3(256), 0, ctx->stream, a);
        }
        // (the next mode's rows reuse the scratch: behind this launch on the same stream)
        hipLaunchKernelGGL(k_bias_lambda, dim3(1), dim3(256), 0, ctx->stream, (int)nb, (const double *)sc, N, sorted[t]->shape, sorted[t]->rate,
                           ctx->seed, ctx->sweep_host, pair_entity(rel_tag), mode, sorted[t]->lambda);
    }
    if ((rc = launch_base(who, ctx, train, n_bias, sorted, mean_value, linear_out))) return rc;
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}

extern "C" int bdf_bias_baseline(bdf_ctx *ctx, const bdf_pairs *pairs, int n_bias, const bdf_bias_term *terms, double mean_value, double *out_dev)
{
    const char *who = "bdf_bias_baseline";
    BDF_REQUIRE(ctx && pairs && terms && out_dev, BDF_ERR_ARG, "%s: NULL argument", who);
    const bdf_bias_term *sorted[BDF_MAX_MODES];
    int rc = bias_terms(who, pairs->n_modes, n_bias, terms, false, sorted);
    if (rc) return rc;
    BDF_HIP(hipSetDevice(ctx->device));
    if ((rc = launch_base(who, ctx, pairs, n_bias, sorted, mean_value, out_dev))) return rc;
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}
