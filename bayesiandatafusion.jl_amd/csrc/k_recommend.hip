// k_recommend.hip -- top-K lists per row from the posterior mean score (setRecommend):
//
//   bdf_scores_push     k_scores_push: this draw's factors into the next slot of a ring, U gathered through the scored rows, in blocks
//                       of four d (slot[(s rows + row) 4 + k] = F[row][4 s + k], zero behind D), so that a matrix operand of 16 rows
//                       is 512 consecutive bytes.
//   bdf_scores_flush    k_scores_accum<DP>: sum[i, j] += sum_b sum_d U_b[i, d] V_b[j, d] on v_mfma_f64_16x16x4_f64.  A workgroup of
//                       four waves owns BDF_REC_TN x BDF_REC_TM cells, a wave 2 x 4 blocks of 16 x 16: the blocks are loaded INTO the
//                       accumulators, one chain of matrix instructions runs over the buffered draws (push order, d in ascending blocks
//                       of four) and the blocks are stored once -- the bits do not depend on where the flushes fall.  Rows behind
//                       n_rows and columns behind M are zero operands and are not stored.
//   bdf_scores_topk     k_topk_rows: one wave per row, one pass over its M sums.  The list lives in the wave, sorted, one entry per
//                       lane; 64 columns at a time are scored, filtered against the K-th entry by a ballot and the survivors inserted
//                       in column order.  The row's listed columns are marked in LDS first (a window of BDF_REC_WINDOW columns).
//   bdf_scores_metrics  k_rec_metrics: one wave per scored row, every list item looked up in the row's relevant test items (sorted on
//                       the host once); k_rec_metrics_final: one workgroup adds the rows' recall, NDCG and hit in a fixed order.
//
// Plain vector stores, no floating-point atomics, no scratch memory.
#include "draw_ring.h"

struct bdf_scores {
    bdf_draw_ring ring;
    DevBuf<double> sum_dev;        // n_rows x M, row-major, then BDF_REC_GUARD doubles of NaN that nothing writes
    // bdf_scores_metrics: the relevant test items of every scored row, built at the first call for (pairs, class_cut)
    const bdf_pairs *rel_pairs = nullptr;      // borrowed
    double rel_cut = 0.0;
    DevBuf<int64_t> rel_ptr_dev;   // n_rows + 1
    DevBuf<int32_t> rel_items_dev; // 1-based item ids, ascending within a row
    DevBuf<double> row_metrics_dev;    // 4 planes of n_rows: recall, ndcg, hit, scored
    ~bdf_scores() { ring.drain(); }
};

namespace {

typedef double bd4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void k_scores_push(const double *__restrict__ U, const double *__restrict__ V, const int32_t *__restrict__ rows,
                                                     int64_t n_rows, int64_t M, int D, int nblk, double *__restrict__ slot)
{
    const int64_t nu = n_rows * nblk, total = nu + M * nblk;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const bool isU = e < nu;
        const int64_t q = isU ? e : e - nu, n = isU ? n_rows : M;
        const int64_t s = q / n, row = q - s * n;
        const int64_t src = (isU && rows) ? (int64_t)rows[row] : row;
        const double *f = (isU ? U : V) + src * D;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int d = (int)s * 4 + k;
            slot[e * 4 + k] = d < D ? f[d] : 0.0;
        }
    }
}

template <int DP>
__global__ __launch_bounds__(256) void k_scores_accum(double *__restrict__ sum, const double *__restrict__ ring, int64_t n_rows, int64_t M, int nblk,
                                                      int held, int64_t tiles_m, int64_t tiles)
{
    constexpr int KQ = DP / 4, RB = BDF_REC_WN / 16, CB = BDF_REC_WM / 16;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 15, h = lane >> 4;
    const int64_t slot = (n_rows + M) * 4 * nblk;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t ti = t / tiles_m, tj = t - ti * tiles_m;
        const int64_t row0 = ti * BDF_REC_TN + (wave >> 1) * BDF_REC_WN, col0 = tj * BDF_REC_TM + (wave & 1) * BDF_REC_WM;
        if (row0 >= n_rows || col0 >= M) continue;         // (wave-uniform; the kernel has no barrier)
        // C layout: lane (j, h), register r: row h + 4 r of the block, column j
        bd4 acc[RB][CB];
#pragma unroll
        for (int rb = 0; rb < RB; rb++)
#pragma unroll
            for (int cb = 0; cb < CB; cb++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int64_t row = row0 + 16 * rb + h + 4 * r, col = col0 + 16 * cb + j;
                    acc[rb][cb][r] = (row < n_rows && col < M) ? sum[row * M + col] : 0.0;
                }
        // operands: lane (j, h) holds U[row j of the block][d = 4 s + h] and V[column j of the block][d = 4 s + h]
        for (int b = 0; b < held; b++) {
            const double *Ub = ring + b * slot, *Vb = Ub + n_rows * 4 * nblk;
#pragma unroll
            for (int s = 0; s < KQ; s++) {
                if (s < nblk) {
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
                        for (int cb = 0; cb < CB; cb++) acc[rb][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[rb], bv[cb], acc[rb][cb], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int rb = 0; rb < RB; rb++)
#pragma unroll
            for (int cb = 0; cb < CB; cb++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int64_t row = row0 + 16 * rb + h + 4 * r, col = col0 + 16 * cb + j;
                    if (row < n_rows && col < M) sum[row * M + col] = acc[rb][cb][r];
                }
    }
}

__global__ __launch_bounds__(64) void k_topk_rows(const double *__restrict__ sum, int64_t n_rows, int64_t M, const int32_t *__restrict__ rows,
                                                  const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx, int K, double draws,
                                                  double mean_value, int32_t *__restrict__ items, double *__restrict__ scores)
{
    __shared__ uint32_t listed[BDF_REC_WINDOW / 32];
    const int lane = threadIdx.x;
    for (int64_t r = blockIdx.x; r < n_rows; r += gridDim.x) {
        double ls = 0.0;                                   // this lane's entry of the list: lanes 0 .. count - 1, best first
        int li = 0, count = 0;
        int64_t e0 = 0, e1 = 0;
        if (rowptr) {
            const int64_t id = rows ? (int64_t)rows[r] : r;
            e0 = rowptr[id]; e1 = rowptr[id + 1];
        }
        for (int64_t w0 = 0; w0 < M; w0 += BDF_REC_WINDOW) {
            const int64_t w1 = w0 + BDF_REC_WINDOW < M ? w0 + BDF_REC_WINDOW : M;
            if (e1 > e0) {
                __syncthreads();                           // (the previous window has been read)
                for (int q = lane; q < BDF_REC_WINDOW / 32; q += 64) listed[q] = 0u;
                __syncthreads();
                for (int64_t e = e0 + lane; e < e1; e += 64) {
                    const int64_t c = (int64_t)colidx[e] - w0;
                    if (c >= 0 && c < BDF_REC_WINDOW) atomicOr(&listed[c >> 5], 1u << (c & 31));
                }
                __syncthreads();
            }
            for (int64_t c0 = w0; c0 < w1; c0 += 64) {
                const int64_t c = c0 + lane;
                bool ok = c < w1;
                double s = 0.0;
                if (ok) {
                    s = bdf_rec_score(sum[r * M + c], draws, mean_value);
                    ok = s == s;                           // (no draws: no candidates)
                    if (e1 > e0) ok = ok && !((listed[(c - w0) >> 5] >> ((c - w0) & 31)) & 1u);
                }
                const int item = (int)(c + 1);
                if (count == K) ok = ok && bdf_rec_before(s, item, readlane_f64(ls, K - 1), __builtin_amdgcn_readlane(li, K - 1));
                uint64_t live = __ballot(ok);
                while (live) {
                    const int src = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)live) - 1);
                    live &= live - 1;
                    const double cs = readlane_f64(s, src);
                    const int ci = __builtin_amdgcn_readlane(item, src);
                    if (count == K && !bdf_rec_before(cs, ci, readlane_f64(ls, K - 1), __builtin_amdgcn_readlane(li, K - 1))) continue;
                    // the entries that stay in front of the candidate are a prefix of the sorted list
                    const int pos = __popcll(__ballot(lane < count && bdf_rec_before(ls, li, cs, ci)));
                    const double us = __shfl_up(ls, 1);
                    const int ui = __shfl_up(li, 1);
                    if (lane == pos) { ls = cs; li = ci; }
                    else if (lane > pos) { ls = us; li = ui; }
                    if (count < K) count++;
                }
            }
        }
        if (lane < K) {
            items[r * K + lane] = lane < count ? li : 0;
            scores[r * K + lane] = lane < count ? ls : __builtin_nan("");
        }
    }
}

__global__ __launch_bounds__(64) void k_rec_metrics(const int32_t *__restrict__ items, int K, int64_t n_rows, const int64_t *__restrict__ rel_ptr,
                                                    const int32_t *__restrict__ rel_items, double *__restrict__ per_row)
{
    const int lane = threadIdx.x;
    for (int64_t r = blockIdx.x; r < n_rows; r += gridDim.x) {
        const int64_t q0 = rel_ptr[r], n = rel_ptr[r + 1] - q0;
        bool hit = false;
        if (lane < K && n > 0) {
            const int it = items[r * K + lane];
            int64_t lo = 0, hi = n;                        // (padding, item 0, is below every id)
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (rel_items[q0 + mid] < it) lo = mid + 1; else hi = mid;
            }
            hit = it > 0 && lo < n && rel_items[q0 + lo] == it;
        }
        const uint64_t hm = __ballot(hit);
        if (lane == 0) {
            double dcg = 0.0, idcg = 0.0;
            for (int p = 0; p < K; p++)
                if ((hm >> p) & 1) dcg += bdf_rec_discount(p + 1);
            const int top = n < K ? (int)n : K;
            for (int p = 1; p <= top; p++) idcg += bdf_rec_discount(p);
            const int hits = __popcll(hm);
            per_row[r] = n > 0 ? (double)hits / (double)n : 0.0;
            per_row[n_rows + r] = n > 0 ? dcg / idcg : 0.0;
            per_row[2 * n_rows + r] = hits > 0 ? 1.0 : 0.0;
            per_row[3 * n_rows + r] = n > 0 ? 1.0 : 0.0;
        }
    }
}

// the rows' figures added in row order: thread t its block of consecutive rows, then thread 0 the 256 partial sums
__global__ __launch_bounds__(256) void k_rec_metrics_final(const double *__restrict__ per_row, int64_t n_rows, double draws, double *__restrict__ out)
{
    __shared__ double part[4][256];
    const int tid = threadIdx.x;
    const int64_t chunk = (n_rows + 255) / 256;
    const int64_t r0 = tid * chunk, r1 = r0 + chunk < n_rows ? r0 + chunk : n_rows;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t r = r0; r < r1; r++)
#pragma unroll
        for (int q = 0; q < 4; q++) s[q] += per_row[q * n_rows + r];
#pragma unroll
    for (int q = 0; q < 4; q++) part[q][tid] = s[q];
    __syncthreads();
    if (tid < 4) {
        double v = 0.0;
        for (int p = 0; p < 256; p++) v += part[tid][p];
        part[tid][0] = v;
    }
    __syncthreads();
    if (tid < 4) {
        const double scored = part[3][0];
        out[tid] = tid == 3 ? scored : (draws > 0.0 ? part[tid][0] / scored : __builtin_nan(""));
    }
}

template <typename T>
int ring_alloc(DevBuf<T> &p, size_t bytes, const char *who, const char *what, int64_t n_rows, int64_t M)
{
    if (p.alloc_bytes(std::max<size_t>(bytes, 16))) {
        const hipError_t e = hipGetLastError();         // (the allocation's error, which this also clears)
        bdf_set_error("%s: no device memory for %s of N = %lld rows and M = %lld columns (%zu bytes): %s", who, what, (long long)n_rows, (long long)M,
                      bytes, hipGetErrorString(e));
        return BDF_ERR_HIP;
    }
    return BDF_OK;
}

}  // namespace

// ---- the ring of draws (draw_ring.h), then bdf_scores
int bdf_ring_init(bdf_draw_ring *r, const char *who, bdf_ctx *ctx, int64_t n_rows, int64_t M, int D, int batch, int tail, int (*flush)(void *), void *owner)
{
    BDF_REQUIRE(n_rows >= 0 && M >= 0 && n_rows < (int64_t)0x7fffffff && M < (int64_t)0x7fffffff, BDF_ERR_ARG,
                "%s: n_rows=%lld and M=%lld must be in 0..2^31-2", who, (long long)n_rows, (long long)M);
    BDF_REQUIRE(D >= 1 && D <= BDF_MAX_D, BDF_ERR_ARG, "%s: num_latent=%d must be in 1..%d", who, D, BDF_MAX_D);
    BDF_REQUIRE(batch >= 1 && batch <= BDF_REC_MAX_BATCH, BDF_ERR_ARG, "%s: batch=%d must be in 1..%d", who, batch, BDF_REC_MAX_BATCH);
    r->ctx = ctx; r->n_rows = n_rows; r->M = M; r->D = D; r->nblk = (D + 3) / 4; r->batch = batch;
    r->slot = (n_rows + M) * 4 * r->nblk + tail; r->flush = flush; r->owner = owner;
    return BDF_OK;
}

int bdf_ring_plane(const bdf_draw_ring *r, const char *who, const char *what, int fill, DevBuf<double> &plane)
{
    const size_t cells = (size_t)r->n_rows * (size_t)r->M, bytes = cells * sizeof(double);
    const int rc = ring_alloc(plane, bytes + BDF_REC_GUARD * sizeof(double), who, what, r->n_rows, r->M);
    if (rc) return rc;
    if (bytes) BDF_HIP(hipMemsetAsync(plane, fill, bytes, r->ctx->stream));
    BDF_HIP(hipMemsetAsync(plane + cells, 0xff, BDF_REC_GUARD * sizeof(double), r->ctx->stream));      // (NaN)
    return BDF_OK;
}

int bdf_ring_alloc(bdf_draw_ring *r, const char *who, const int32_t *rows_dev)
{
    const int64_t n_rows = r->n_rows;
    int rc;
    if ((rc = ring_alloc(r->ring_dev, (size_t)r->batch * (size_t)r->slot * sizeof(double), who, "the ring of draws", n_rows, r->M))) return rc;
    if (rows_dev && n_rows) {
        if ((rc = ring_alloc(r->rows_dev, (size_t)n_rows * sizeof(int32_t), who, "the scored rows", n_rows, r->M))) return rc;
        r->rows_host.resize((size_t)n_rows);
        BDF_HIP(hipStreamSynchronize(r->ctx->stream));
        BDF_HIP(hipMemcpy(r->rows_host.data(), rows_dev, (size_t)n_rows * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (int64_t q = 0; q < n_rows; q++)
            BDF_REQUIRE(r->rows_host[(size_t)q] >= 0, BDF_ERR_BOUNDS, "%s: rows[%lld] = %d is negative (0-based rows of U)", who, (long long)q,
                        r->rows_host[(size_t)q]);
        BDF_HIP(hipMemcpy(r->rows_dev, r->rows_host.data(), (size_t)n_rows * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    BDF_HIP(hipStreamSynchronize(r->ctx->stream));
    return BDF_OK;
}

int bdf_ring_push(bdf_draw_ring *r, const double *U, const double *V)
{
    BDF_HIP(hipSetDevice(r->ctx->device));
    const int64_t quads = (r->n_rows + r->M) * r->nblk;
    if (quads > 0) {
        const dim3 grid((unsigned)std::min<int64_t>((quads + 255) / 256, 65536));
        hipLaunchKernelGGL(k_scores_push, grid, dim3(256), 0, r->ctx->stream, U, V, (const int32_t *)r->rows_dev, r->n_rows, r->M, r->D, r->nblk, bdf_ring_slot(r));
        BDF_HIP(hipGetLastError());
    }
    r->held++;
    r->draws += 1.0;
    return r->held == r->batch ? r->flush(r->owner) : BDF_OK;
}

int bdf_ring_copy(bdf_draw_ring *r, const char *who, const char *what, double *plane, double *buf_dev, int64_t first, int64_t count, int write)
{
    const int64_t cells = r->n_rows * r->M + BDF_REC_GUARD;
    BDF_REQUIRE(first >= 0 && count >= 0 && first <= cells && count <= cells - first, BDF_ERR_BOUNDS,
                "%s: cells %lld .. %lld are outside the %s and its guard (%lld doubles)", who, (long long)first, (long long)(first + count), what, (long long)cells);
    if (const int rc = r->flush(r->owner)) return rc;
    BDF_HIP(hipSetDevice(r->ctx->device));
    if (count) BDF_HIP(hipMemcpyAsync(write ? plane + first : buf_dev, write ? buf_dev : plane + first, (size_t)count * sizeof(double),
                                      hipMemcpyDeviceToDevice, r->ctx->stream));
    return BDF_OK;
}

int bdf_ring_set_draws(bdf_draw_ring *r, const char *who, double draws)
{
    BDF_REQUIRE(r != nullptr && draws >= 0.0, BDF_ERR_ARG, "%s_set_draws: NULL argument or a negative count", who);
    BDF_REQUIRE(r->held == 0, BDF_ERR_ARG, "%s_set_draws: %d draws are buffered (%s_flush first)", who, r->held, who);
    r->draws = draws;
    return BDF_OK;
}

int bdf_topk_plane(const bdf_draw_ring *r, const char *who, const double *plane, const bdf_rel *rel, int K, double draws, double mean_value,
                   int32_t *items_out, double *scores_out)
{
    const int64_t n_rows = r->n_rows, M = r->M;
    BDF_REQUIRE(K >= 1 && K <= BDF_REC_MAX_K, BDF_ERR_ARG, "%s: K=%d must be in 1..%d", who, K, BDF_REC_MAX_K);
    const int64_t *rowptr = nullptr;
    const int32_t *colidx = nullptr;
    if (rel) {
        BDF_REQUIRE(rel->n_modes == 2 && !rel->sharded, BDF_ERR_ARG, "%s: the listed cells come from a two-mode relation on one rank", who);
        BDF_REQUIRE(rel->dims[1] == M, BDF_ERR_ARG, "%s: the relation has %lld columns, the scores %lld", who, (long long)rel->dims[1], (long long)M);
        const int64_t N = rel->dims[0];
        if (r->rows_dev) {
            for (int64_t q = 0; q < n_rows; q++)
                BDF_REQUIRE(r->rows_host[(size_t)q] < N, BDF_ERR_BOUNDS, "%s: rows[%lld] = %d is outside the relation's %lld rows", who, (long long)q,
                            r->rows_host[(size_t)q], (long long)N);
        } else {
            BDF_REQUIRE(n_rows <= N, BDF_ERR_ARG, "%s: %lld scored rows, the relation has %lld", who, (long long)n_rows, (long long)N);
        }
        rowptr = rel->idx[0].rowptr_dev; colidx = rel->idx[0].colidx_dev;
    }
    if (n_rows == 0) return BDF_OK;
    BDF_HIP(hipSetDevice(r->ctx->device));
    const dim3 grid((unsigned)std::min<int64_t>(n_rows, 1 << 20));
    hipLaunchKernelGGL(k_topk_rows, grid, dim3(64), 0, r->ctx->stream, plane, n_rows, M, (const int32_t *)r->rows_dev, rowptr, colidx, K, draws, mean_value,
                       items_out, scores_out);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}

extern "C" int bdf_scores_destroy(bdf_scores *sc)
{
    if (sc) delete sc;
    return BDF_OK;
}

static int scores_flush(void *sc) { return bdf_scores_flush((bdf_scores *)sc); }

extern "C" int bdf_scores_create(bdf_ctx *ctx, int64_t n_rows, int64_t M, int D, int batch, const int32_t *rows_dev, bdf_scores **out)
{
    const char *who = "bdf_scores_create";
    BDF_REQUIRE(ctx && out, BDF_ERR_ARG, "%s: NULL argument", who);
    std::unique_ptr<bdf_scores> sc(new bdf_scores());
    int rc = bdf_ring_init(&sc->ring, who, ctx, n_rows, M, D, batch, 0, scores_flush, sc.get());
    if (rc) return rc;
    BDF_HIP(hipSetDevice(ctx->device));
    if ((rc = bdf_ring_plane(&sc->ring, who, "the score sum", 0, sc->sum_dev))) return rc;
    if ((rc = bdf_ring_alloc(&sc->ring, who, rows_dev))) return rc;
    *out = sc.release();
    return BDF_OK;
}

extern "C" int bdf_scores_flush(bdf_scores *sc)
{
    BDF_REQUIRE(sc != nullptr, BDF_ERR_ARG, "bdf_scores_flush: NULL argument");
    bdf_draw_ring *r = &sc->ring;
    if (r->held == 0) return BDF_OK;
    bdf_ctx *ctx = r->ctx;
    BDF_HIP(hipSetDevice(ctx->device));
    const int held = r->held;
    r->held = 0;
    if (r->n_rows == 0 || r->M == 0) return BDF_OK;
    const int64_t tiles_n = (r->n_rows + BDF_REC_TN - 1) / BDF_REC_TN, tiles_m = (r->M + BDF_REC_TM - 1) / BDF_REC_TM;
    const int64_t tiles = tiles_n * tiles_m;
    const dim3 grid((unsigned)std::min<int64_t>(tiles, (int64_t)std::max(ctx->n_cus, 1) * 8));
    const int DP = r->D <= 16 ? 16 : (r->D <= 32 ? 32 : 64);
    if (DP == 16) hipLaunchKernelGGL(k_scores_accum<16>, grid, dim3(256), 0, ctx->stream, sc->sum_dev, (const double *)r->ring_dev, r->n_rows, r->M, r->nblk, held, tiles_m, tiles);
    else if (DP == 32) hipLaunchKernelGGL(k_scores_accum<32>, grid, dim3(256), 0, ctx->stream, sc->sum_dev, (const double *)r->ring_dev, r->n_rows, r->M, r->nblk, held, tiles_m, tiles);
    else hipLaunchKernelGGL(k_scores_accum<64>, grid, dim3(256), 0, ctx->stream, sc->sum_dev, (const double *)r->ring_dev, r->n_rows, r->M, r->nblk, held, tiles_m, tiles);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}

extern "C" int bdf_scores_push(bdf_scores *sc, const double *U, const double *V)
{
    BDF_REQUIRE(sc && U && V, BDF_ERR_ARG, "bdf_scores_push: NULL argument");
    return bdf_ring_push(&sc->ring, U, V);
}

extern "C" int bdf_scores_copy(bdf_scores *sc, double *buf_dev, int64_t first, int64_t count, int write)
{
    BDF_REQUIRE(sc && buf_dev, BDF_ERR_ARG, "bdf_scores_copy: NULL argument");
    return bdf_ring_copy(&sc->ring, "bdf_scores_copy", "sum", sc->sum_dev, buf_dev, first, count, write);
}

extern "C" int bdf_scores_set_draws(bdf_scores *sc, double draws) { return bdf_ring_set_draws(sc ? &sc->ring : nullptr, "bdf_scores", draws); }

extern "C" int bdf_scores_topk(bdf_scores *sc, const bdf_rel *rel, int K, double mean_value, int32_t *items_out, double *scores_out)
{
    BDF_REQUIRE(sc && items_out && scores_out, BDF_ERR_ARG, "bdf_scores_topk: NULL argument");
    BDF_REQUIRE(K >= 1 && K <= BDF_REC_MAX_K, BDF_ERR_ARG, "bdf_scores_topk: K=%d must be in 1..%d", K, BDF_REC_MAX_K);
    if (const int rc = bdf_scores_flush(sc)) return rc;
    return bdf_topk_plane(&sc->ring, "bdf_scores_topk", sc->sum_dev, rel, K, sc->ring.draws, mean_value, items_out, scores_out);
}

extern "C" int bdf_scores_metrics(bdf_scores *sc, const int32_t *items, int K, const bdf_pairs *test, double class_cut, double *out)
{
    BDF_REQUIRE(sc && items && test && out, BDF_ERR_ARG, "bdf_scores_metrics: NULL argument");
    BDF_REQUIRE(K >= 1 && K <= BDF_REC_MAX_K, BDF_ERR_ARG, "bdf_scores_metrics: K=%d must be in 1..%d", K, BDF_REC_MAX_K);
    BDF_REQUIRE(test->n_modes == 2, BDF_ERR_ARG, "bdf_scores_metrics: the test cells belong to a two-mode relation, not %d modes", test->n_modes);
    bdf_ctx *ctx = sc->ring.ctx;
    BDF_HIP(hipSetDevice(ctx->device));
    const int64_t n_rows = sc->ring.n_rows;
    if (sc->rel_pairs != test || sc->rel_cut != class_cut || !sc->rel_ptr_dev) {
        // the relevant test cells (value > class_cut) by scored row, each row's items ascending and distinct
        const int64_t n = test->n;
        const int32_t *ti = test->ids_host.data(), *tj = ti + n;
        std::map<int32_t, int32_t> slot_of;
        if (sc->ring.rows_dev)
            for (int64_t r = 0; r < n_rows; r++) slot_of[sc->ring.rows_host[(size_t)r]] = (int32_t)r;
        std::vector<std::pair<int32_t, int32_t>> cells;
        for (int64_t k = 0; k < n; k++) {
            if (!(test->values_host[(size_t)k] > class_cut) || tj[k] >= sc->ring.M) continue;
            int32_t r;
            if (sc->ring.rows_dev) {
                const auto it = slot_of.find(ti[k]);
                if (it == slot_of.end()) continue;
                r = it->second;
            } else {
                if (ti[k] >= n_rows) continue;
                r = ti[k];
            }
            cells.emplace_back(r, tj[k] + 1);
        }
        std::sort(cells.begin(), cells.end());
        cells.erase(std::unique(cells.begin(), cells.end()), cells.end());
        std::vector<int64_t> ptr((size_t)n_rows + 1, 0);
        std::vector<int32_t> its(cells.size());
        for (size_t q = 0; q < cells.size(); q++) { ptr[(size_t)cells[q].first + 1]++; its[q] = cells[q].second; }
        for (int64_t r = 0; r < n_rows; r++) ptr[(size_t)r + 1] += ptr[(size_t)r];
        BDF_HIP(hipStreamSynchronize(ctx->stream));
        int rc;
        if ((rc = sc->rel_ptr_dev.upload(ptr)) || (rc = sc->rel_items_dev.upload(its))) return rc;
        if (!sc->row_metrics_dev && (rc = sc->row_metrics_dev.alloc_bytes(std::max<size_t>((size_t)n_rows * 4 * sizeof(double), 16)))) return rc;
        sc->rel_pairs = test; sc->rel_cut = class_cut;
    }
    if (n_rows > 0) {
        const dim3 grid((unsigned)std::min<int64_t>(n_rows, 1 << 20));
        hipLaunchKernelGGL(k_rec_metrics, grid, dim3(64), 0, ctx->stream, items, K, n_rows, (const int64_t *)sc->rel_ptr_dev, (const int32_t *)sc->rel_items_dev,
                           sc->row_metrics_dev);
    }
    hipLaunchKernelGGL(k_rec_metrics_final, dim3(1), dim3(256), 0, ctx->stream, (const double *)sc->row_metrics_dev, n_rows, sc->ring.draws, out);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}
