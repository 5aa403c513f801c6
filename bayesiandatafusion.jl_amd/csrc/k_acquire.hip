// k_acquire.hip -- acquisition lists per row from the moments of u.v over the posterior draws (setAcquire):
//
//   bdf_acquire_push    k_scores_push (k_recommend.hip: bdf_ring_push) of this draw's factors into the next slot of a ring, in the
//                       layout of section 21, and k_acquire_alpha: one lane stores the draw's precision behind the factors, read
//                       from device memory when it was sampled there.
//   bdf_acquire_flush   k_acquire_accum<PROB>: a workgroup of four waves owns BDF_ACQ_TN x BDF_ACQ_TM cells, a wave 2 x 2 blocks of
//                       16 x 16.  The wave loads its blocks of the planes mean, M2 (and psum) into registers; per buffered draw, in
//                       push order, it forms p = u.v on v_mfma_f64_16x16x4_f64 from ZERO accumulators (d in ascending blocks of
//                       four) and folds it in with the draw's running count n (Welford: bdf_acq_fold; psum: bdf_acq_prob); the
//                       planes are stored once.  The fold is sequential and a draw's product starts from zero, so the planes' bits
//                       depend neither on `batch` nor on where the flushes fall.  Rows behind n_rows and columns behind M are
//                       zero operands and are not stored.
//   bdf_acquire_topk    k_acquire_score: the score plane from (mean, M2, psum, n) by bdf_acq_score; k_topk_rows (k_recommend.hip:
//                       bdf_topk_plane) on that plane with draws = 1 and mean_value = 0, for which bdf_rec_score is the identity;
//                       k_acquire_gather: mean + mean_value, sd and prob at the listed items.
//
// Plain vector stores, no atomics, no LDS, no scratch memory.
#include "draw_ring.h"
#include "acquire.h"

struct bdf_acquire {
    bdf_draw_ring ring;            // a slot: (n_rows + M) x 4 nblk of factors, then BDF_ACQ_TAIL doubles (the first: alpha)
    int want_prob = 0;
    double mean_value = 0.0, threshold = 0.0;
    DevBuf<double> plane_dev[4];   // BDF_ACQ_MEAN, _M2, _PSUM (empty without want_prob), _SCORE: n_rows x M row-major, then BDF_REC_GUARD
                                   // doubles of NaN that nothing writes
    ~bdf_acquire() { ring.drain(); }
};

#define BDF_ACQ_TAIL 4             // doubles behind a slot's factors (32 bytes: the next slot stays aligned as the first)

namespace {

typedef double bd4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(64) void k_acquire_alpha(double *__restrict__ dst, double alpha, const double *__restrict__ alpha_dev)
{
    if (threadIdx.x == 0) dst[0] = alpha_dev ? alpha_dev[0] : alpha;
}

template <bool PROB>
__global__ __launch_bounds__(256) void k_acquire_accum(double *__restrict__ mean_pl, double *__restrict__ m2_pl, double *__restrict__ psum_pl,
                                                       const double *__restrict__ ring, int64_t n_rows, int64_t M, int nblk, int held, int64_t slot,
                                                       double n0, double mean_value, double threshold, int64_t tiles_m, int64_t tiles)
{
    constexpr int RB = BDF_ACQ_WN / 16, CB = BDF_ACQ_WM / 16;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 15, h = lane >> 4;
    const int64_t factors = (n_rows + M) * 4 * nblk;       // doubles of a slot's factors; alpha stands behind them
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t ti = t / tiles_m, tj = t - ti * tiles_m;
        const int64_t row0 = ti * BDF_ACQ_TN + (wave >> 1) * BDF_ACQ_WN, col0 = tj * BDF_ACQ_TM + (wave & 1) * BDF_ACQ_WM;
        if (row0 >= n_rows || col0 >= M) continue;         // (wave-uniform; the kernel has no barrier)
        // C layout: lane (j, h), register r: row h + 4 r of the block, column j
        bd4 mu[RB][CB], m2[RB][CB], ps[RB][CB];
#pragma unroll
        for (int rb = 0; rb < RB; rb++)
#pragma unroll
            for (int cb = 0; cb < CB; cb++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int64_t row = row0 + 16 * rb + h + 4 * r, col = col0 + 16 * cb + j;
                    const bool in = row < n_rows && col < M;
                    mu[rb][cb][r] = in ? mean_pl[row * M + col] : 0.0;
                    m2[rb][cb][r] = in ? m2_pl[row * M + col] : 0.0;
                    ps[rb][cb][r] = (PROB && in) ? psum_pl[row * M + col] : 0.0;
                }
        for (int b = 0; b < held; b++) {
            const double *Ub = ring + b * slot, *Vb = Ub + n_rows * 4 * nblk;
            bd4 p[RB][CB];
#pragma unroll
            for (int rb = 0; rb < RB; rb++)
#pragma unroll
                for (int cb = 0; cb < CB; cb++) p[rb][cb] = bd4{0.0, 0.0, 0.0, 0.0};
            // operands: lane (j, h) holds U[row j of the block][d = 4 s + h] and V[column j of the block][d = 4 s + h]
            for (int s = 0; s < nblk; s++) {
                double av[RB], bv[CB];
#pragma unroll
                for (int rb = 0; rb < RB; rb++) {
                    const int64_t row = row0 + 16 * rb + j;
                    av[rb] = row < n_rows ? Ub[(s * n_rows + row) * 4 + h] : 0.0;
                }
#pragma unroll
                for (int cb = 0; cb < CB; cb++) {
                    const int64_t col = col0 + 16 * cb + j;
                    bv[cb] = col < M ? Vb[(s * M + col) * 4 + h] : 0.0;
                }
#pragma unroll
                for (int rb = 0; rb < RB; rb++)
#pragma unroll
                    for (int cb = 0; cb < CB; cb++) p[rb][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[rb], bv[cb], p[rb][cb], 0, 0, 0);
            }
            const double n = n0 + (double)(b + 1);
            const double root_alpha = PROB ? sqrt(Ub[factors]) : 0.0;
#pragma unroll
            for (int rb = 0; rb < RB; rb++)
#pragma unroll
                for (int cb = 0; cb < CB; cb++)
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const double pr = p[rb][cb][r];
                        double a = mu[rb][cb][r], q = m2[rb][cb][r];
                        bdf_acq_fold(pr, n, a, q);
                        mu[rb][cb][r] = a; m2[rb][cb][r] = q;
                        if (PROB) ps[rb][cb][r] += bdf_acq_prob(pr, root_alpha, mean_value, threshold);
                    }
        }
#pragma unroll
        for (int rb = 0; rb < RB; rb++)
#pragma unroll
            for (int cb = 0; cb < CB; cb++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int64_t row = row0 + 16 * rb + h + 4 * r, col = col0 + 16 * cb + j;
                    if (row < n_rows && col < M) {
                        mean_pl[row * M + col] = mu[rb][cb][r];
                        m2_pl[row * M + col] = m2[rb][cb][r];
                        if (PROB) psum_pl[row * M + col] = ps[rb][cb][r];
                    }
                }
    }
}

__global__ __launch_bounds__(256) void k_acquire_score(const double *__restrict__ mean_pl, const double *__restrict__ m2_pl,
                                                       const double *__restrict__ psum_pl, int64_t cells, int rule, double n, double kappa,
                                                       double mean_value, double *__restrict__ score_pl)
{
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < cells; e += (int64_t)gridDim.x * 256)
        score_pl[e] = bdf_acq_score(rule, mean_pl[e], m2_pl[e], rule == BDF_ACQ_PROB ? psum_pl[e] : 0.0, n, kappa, mean_value);
}

__global__ __launch_bounds__(256) void k_acquire_gather(const double *__restrict__ mean_pl, const double *__restrict__ m2_pl,
                                                        const double *__restrict__ psum_pl, const int32_t *__restrict__ items, int64_t n_rows,
                                                        int64_t M, int K, double n, double mean_value, double *__restrict__ mean_out,
                                                        double *__restrict__ sd_out, double *__restrict__ prob_out)
{
    const int64_t total = n_rows * K;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int item = items[e];
        const bool on = item > 0 && (int64_t)item <= M;
        const int64_t cell = on ? (e / K) * M + (item - 1) : 0;
        const double nan = __builtin_nan("");
        if (mean_out) mean_out[e] = on ? mean_pl[cell] + mean_value : nan;
        if (sd_out) sd_out[e] = on ? bdf_acq_sd(m2_pl[cell], n) : nan;
        if (prob_out) prob_out[e] = on ? bdf_acq_score(BDF_ACQ_PROB, 0.0, 0.0, psum_pl[cell], n, 0.0, 0.0) : nan;
    }
}

const char *const plane_name[4] = {"the mean plane", "the M2 plane", "the psum plane", "the score plane"};

}  // namespace

extern "C" int bdf_acquire_destroy(bdf_acquire *ac)
{
    if (ac) delete ac;
    return BDF_OK;
}

static int acquire_flush(void *ac) { return bdf_acquire_flush((bdf_acquire *)ac); }

extern "C" int bdf_acquire_create(bdf_ctx *ctx, int64_t n_rows, int64_t M, int D, int batch, const int32_t *rows_dev, int want_prob,
                                  double mean_value, double threshold, bdf_acquire **out)
{
    const char *who = "bdf_acquire_create";
    BDF_REQUIRE(ctx && out, BDF_ERR_ARG, "%s: NULL argument", who);
    std::unique_ptr<bdf_acquire> ac(new bdf_acquire());
    int rc = bdf_ring_init(&ac->ring, who, ctx, n_rows, M, D, batch, BDF_ACQ_TAIL, acquire_flush, ac.get());
    if (rc) return rc;
    BDF_REQUIRE(std::isfinite(mean_value), BDF_ERR_ARG, "bdf_acquire_create: mean_value must be finite");
    BDF_REQUIRE(!want_prob || std::isfinite(threshold), BDF_ERR_ARG, "bdf_acquire_create: threshold must be finite");
    BDF_HIP(hipSetDevice(ctx->device));
    ac->want_prob = want_prob ? 1 : 0; ac->mean_value = mean_value; ac->threshold = want_prob ? threshold : 0.0;
    for (int q = 0; q < 4; q++) {
        if (q == BDF_ACQ_PSUM && !want_prob) continue;
        // (the score plane holds NaN until a list is asked for)
        if ((rc = bdf_ring_plane(&ac->ring, who, plane_name[q], q == BDF_ACQ_SCORE ? 0xff : 0, ac->plane_dev[q]))) return rc;
    }
    if ((rc = bdf_ring_alloc(&ac->ring, who, rows_dev))) return rc;
    *out = ac.release();
    return BDF_OK;
}

extern "C" int bdf_acquire_flush(bdf_acquire *ac)
{
    BDF_REQUIRE(ac != nullptr, BDF_ERR_ARG, "bdf_acquire_flush: NULL argument");
    bdf_draw_ring *r = &ac->ring;
    if (r->held == 0) return BDF_OK;
    bdf_ctx *ctx = r->ctx;
    BDF_HIP(hipSetDevice(ctx->device));
    const int held = r->held;
    r->held = 0;
    if (r->n_rows == 0 || r->M == 0) return BDF_OK;
    const int64_t tiles_n = (r->n_rows + BDF_ACQ_TN - 1) / BDF_ACQ_TN, tiles_m = (r->M + BDF_ACQ_TM - 1) / BDF_ACQ_TM;
    const int64_t tiles = tiles_n * tiles_m;
    const dim3 grid((unsigned)std::min<int64_t>(tiles, (int64_t)std::max(ctx->n_cus, 1) * 8));
    const double n0 = r->draws - (double)held;            // the draws that the planes hold already
    if (ac->want_prob)
        hipLaunchKernelGGL(k_acquire_accum<true>, grid, dim3(256), 0, ctx->stream, ac->plane_dev[BDF_ACQ_MEAN], ac->plane_dev[BDF_ACQ_M2],
                           ac->plane_dev[BDF_ACQ_PSUM], (const double *)r->ring_dev, r->n_rows, r->M, r->nblk, held, r->slot, n0, ac->mean_value,
                           ac->threshold, tiles_m, tiles);
    else
        hipLaunchKernelGGL(k_acquire_accum<false>, grid, dim3(256), 0, ctx->stream, ac->plane_dev[BDF_ACQ_MEAN], ac->plane_dev[BDF_ACQ_M2],
                           (double *)nullptr, (const double *)r->ring_dev, r->n_rows, r->M, r->nblk, held, r->slot, n0, ac->mean_value,
                           ac->threshold, tiles_m, tiles);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}

extern "C" int bdf_acquire_push(bdf_acquire *ac, const double *U, const double *V, double alpha, const double *alpha_dev)
{
    BDF_REQUIRE(ac && U && V, BDF_ERR_ARG, "bdf_acquire_push: NULL argument");
    BDF_REQUIRE(alpha_dev || (alpha > 0.0 && std::isfinite(alpha)), BDF_ERR_ARG, "bdf_acquire_push: alpha=%g must be positive and finite (or alpha_dev given)", alpha);
    BDF_HIP(hipSetDevice(ac->ring.ctx->device));
    // (the slot's tail ahead of its factors, which bdf_ring_push writes before it counts the draw and flushes a full ring)
    hipLaunchKernelGGL(k_acquire_alpha, dim3(1), dim3(64), 0, ac->ring.ctx->stream, bdf_ring_slot(&ac->ring) + (ac->ring.slot - BDF_ACQ_TAIL), alpha, alpha_dev);
    BDF_HIP(hipGetLastError());
    return bdf_ring_push(&ac->ring, U, V);
}

extern "C" int bdf_acquire_copy(bdf_acquire *ac, int plane, double *buf_dev, int64_t first, int64_t count, int write)
{
    BDF_REQUIRE(ac && buf_dev, BDF_ERR_ARG, "bdf_acquire_copy: NULL argument");
    BDF_REQUIRE(plane >= 0 && plane < 4 && ac->plane_dev[plane], BDF_ERR_ARG,
                "bdf_acquire_copy: plane=%d must be 0 (mean), 1 (M2), 2 (psum, kept with want_prob only) or 3 (score)", plane);
    return bdf_ring_copy(&ac->ring, "bdf_acquire_copy", "plane", ac->plane_dev[plane], buf_dev, first, count, write);
}

extern "C" int bdf_acquire_set_draws(bdf_acquire *ac, double draws) { return bdf_ring_set_draws(ac ? &ac->ring : nullptr, "bdf_acquire", draws); }

extern "C" int bdf_acquire_topk(bdf_acquire *ac, const bdf_rel *rel, int K, int rule, double kappa, int32_t *items_out, double *scores_out,
                                double *mean_out, double *sd_out, double *prob_out)
{
    BDF_REQUIRE(ac && items_out && scores_out, BDF_ERR_ARG, "bdf_acquire_topk: NULL argument");
    BDF_REQUIRE(rule == BDF_ACQ_UCB || rule == BDF_ACQ_SD || rule == BDF_ACQ_PROB, BDF_ERR_ARG, "bdf_acquire_topk: rule=%d must be 0 (ucb), 1 (sd) or 2 (prob_above)", rule);
    BDF_REQUIRE(rule != BDF_ACQ_UCB || (kappa >= 0.0 && std::isfinite(kappa)), BDF_ERR_ARG, "bdf_acquire_topk: kappa=%g must be finite and not negative", kappa);
    BDF_REQUIRE(ac->want_prob || (rule != BDF_ACQ_PROB && !prob_out), BDF_ERR_ARG, "bdf_acquire_topk: no psum plane is kept (bdf_acquire_create with want_prob)");
    BDF_REQUIRE(K >= 1 && K <= BDF_REC_MAX_K, BDF_ERR_ARG, "bdf_acquire_topk: K=%d must be in 1..%d", K, BDF_REC_MAX_K);
    int rc = bdf_acquire_flush(ac);
    if (rc) return rc;
    bdf_ctx *ctx = ac->ring.ctx;
    BDF_HIP(hipSetDevice(ctx->device));
    const int64_t cells = ac->ring.n_rows * ac->ring.M;
    if (cells > 0) {
        const dim3 grid((unsigned)std::min<int64_t>((cells + 255) / 256, 65536));
        hipLaunchKernelGGL(k_acquire_score, grid, dim3(256), 0, ctx->stream, (const double *)ac->plane_dev[BDF_ACQ_MEAN], (const double *)ac->plane_dev[BDF_ACQ_M2],
                           (const double *)ac->plane_dev[BDF_ACQ_PSUM], cells, rule, ac->ring.draws, kappa, ac->mean_value, ac->plane_dev[BDF_ACQ_SCORE]);
        BDF_HIP(hipGetLastError());
    }
    // bdf_rec_score(score, 1, 0) is the score itself
    rc = bdf_topk_plane(&ac->ring, "bdf_acquire_topk", ac->plane_dev[BDF_ACQ_SCORE], rel, K, 1.0, 0.0, items_out, scores_out);
    if (rc) return rc;
    if (ac->ring.n_rows > 0 && (mean_out || sd_out || prob_out)) {
        const int64_t total = ac->ring.n_rows * K;
        const dim3 grid((unsigned)std::min<int64_t>((total + 255) / 256, 65536));
        hipLaunchKernelGGL(k_acquire_gather, grid, dim3(256), 0, ctx->stream, (const double *)ac->plane_dev[BDF_ACQ_MEAN], (const double *)ac->plane_dev[BDF_ACQ_M2],
                           (const double *)ac->plane_dev[BDF_ACQ_PSUM], (const int32_t *)items_out, ac->ring.n_rows, ac->ring.M, K, ac->ring.draws, ac->mean_value, mean_out,
                           sd_out, prob_out);
        BDF_HIP(hipGetLastError());
    }
    return BDF_OK;
}
