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
#include "bdf_common.h"
#include "recommend.h"

struct bdf_scores {
    bdf_ctx *ctx;
    int64_t n_rows, M;
    int D, nblk;                   // nblk: blocks of four d, ceil(D / 4)
    int batch, held;               // the ring's slots, and how many hold a draw that is not in the sum yet
    double draws;                  // draws pushed
    double *sum_dev;               // n_rows x M, row-major, then BDF_REC_GUARD doubles of NaN that nothing writes
    double *ring_dev;              // batch slots of (n_rows + M) x 4 nblk doubles
    int32_t *rows_dev;             // nullable: 0-based row of U per scored row
    std::vector<int32_t> rows_host;
    // bdf_scores_metrics: the relevant test items of every scored row, built at the first call for (pairs, class_cut)
    const bdf_pairs *rel_pairs;
    double rel_cut;
    int64_t *rel_ptr_dev;          // n_rows + 1
    int32_t *rel_items_dev;        // 1-based item ids, ascending within a row
    double *row_metrics_dev;       // 4 planes of n_rows: recall, ndcg, hit, scored
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

int scores_alloc(void **p, size_t bytes, const char *what, int64_t n_rows, int64_t M)
{
    const hipError_t e = hipMalloc(p, std::max<size_t>(bytes, 16));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        bdf_set_error("bdf_scores_create: no device memory for %s of N = %lld rows and M = %lld columns (%zu bytes): %s", what,
                      (long long)n_rows, (long long)M, bytes, hipGetErrorString(e));
        return BDF_ERR_HIP;
    }
    return BDF_OK;
}

}  // namespace

extern "C" int bdf_scores_destroy(bdf_scores *sc)
{
    if (!sc) return BDF_OK;
    hipSetDevice(sc->ctx->device);
    hipStreamSynchronize(sc->ctx->stream);
    hipFree(sc->sum_dev); hipFree(sc->ring_dev);
    if (sc->rows_dev) hipFree(sc->rows_dev);
    if (sc->rel_ptr_dev) hipFree(sc->rel_ptr_dev);
    if (sc->rel_items_dev) hipFree(sc->rel_items_dev);
    if (sc->row_metrics_dev) hipFree(sc->row_metrics_dev);
    delete sc;
    return BDF_OK;
}

extern "C" int bdf_scores_create(bdf_ctx *ctx, int64_t n_rows, int64_t M, int D, int batch, const int32_t *rows_dev, bdf_scores **out)
{
    BDF_REQUIRE(ctx && out, BDF_ERR_ARG, "bdf_scores_create: NULL argument");
    BDF_REQUIRE(n_rows >= 0 && M >= 0 && n_rows < (int64_t)0x7fffffff && M < (int64_t)0x7fffffff, BDF_ERR_ARG,
                "bdf_scores_create: n_rows=%lld and M=%lld must be in 0..2^31-2", (long long)n_rows, (long long)M);
    BDF_REQUIRE(D >= 1 && D <= BDF_MAX_D, BDF_ERR_ARG, "bdf_scores_create: num_latent=%d must be in 1..%d", D, BDF_MAX_D);
    BDF_REQUIRE(batch >= 1 && batch <= BDF_REC_MAX_BATCH, BDF_ERR_ARG, "bdf_scores_create: batch=%d must be in 1..%d", batch, BDF_REC_MAX_BATCH);
    BDF_HIP(hipSetDevice(ctx->device));
    bdf_scores *sc = new bdf_scores();
    sc->ctx = ctx; sc->n_rows = n_rows; sc->M = M; sc->D = D; sc->nblk = (D + 3) / 4; sc->batch = batch; sc->held = 0; sc->draws = 0.0;
    sc->sum_dev = sc->ring_dev = nullptr; sc->rows_dev = nullptr;
    sc->rel_pairs = nullptr; sc->rel_cut = 0.0; sc->rel_ptr_dev = nullptr; sc->rel_items_dev = nullptr; sc->row_metrics_dev = nullptr;
    struct Guard { bdf_scores *p; ~Guard() { if (p) bdf_scores_destroy(p); } } guard{sc};
    const size_t sum_bytes = (size_t)n_rows * (size_t)M * sizeof(double);
    const size_t ring_bytes = (size_t)batch * (size_t)(n_rows + M) * 4 * sc->nblk * sizeof(double);
    int rc;
    if ((rc = scores_alloc((void **)&sc->sum_dev, sum_bytes + BDF_REC_GUARD * sizeof(double), "the score sum", n_rows, M))) return rc;
    if ((rc = scores_alloc((void **)&sc->ring_dev, ring_bytes, "the ring of draws", n_rows, M))) return rc;
    if (rows_dev && n_rows) {
        if ((rc = scores_alloc((void **)&sc->rows_dev, (size_t)n_rows * sizeof(int32_t), "the scored rows", n_rows, M))) return rc;
        sc->rows_host.resize((size_t)n_rows);
        BDF_HIP(hipStreamSynchronize(ctx->stream));
        BDF_HIP(hipMemcpy(sc->rows_host.data(), rows_dev, (size_t)n_rows * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (int64_t r = 0; r < n_rows; r++)
            BDF_REQUIRE(sc->rows_host[(size_t)r] >= 0, BDF_ERR_BOUNDS, "bdf_scores_create: rows[%lld] = %d is negative (0-based rows of U)", (long long)r,
                        sc->rows_host[(size_t)r]);
        BDF_HIP(hipMemcpy(sc->rows_dev, sc->rows_host.data(), (size_t)n_rows * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    if (sum_bytes) BDF_HIP(hipMemsetAsync(sc->sum_dev, 0, sum_bytes, ctx->stream));
    BDF_HIP(hipMemsetAsync(sc->sum_dev + (size_t)n_rows * (size_t)M, 0xff, BDF_REC_GUARD * sizeof(double), ctx->stream));      // (NaN)
    BDF_HIP(hipStreamSynchronize(ctx->stream));
    guard.p = nullptr;
    *out = sc;
    return BDF_OK;
}

extern "C" int bdf_scores_flush(bdf_scores *sc)
{
    BDF_REQUIRE(sc != nullptr, BDF_ERR_ARG, "bdf_scores_flush: NULL argument");
    if (sc->held == 0) return BDF_OK;
    bdf_ctx *ctx = sc->ctx;
    BDF_HIP(hipSetDevice(ctx->device));
    const int held = sc->held;
    sc->held = 0;
    if (sc->n_rows == 0 || sc->M == 0) return BDF_OK;
    const int64_t tiles_n = (sc->n_rows + BDF_REC_TN - 1) / BDF_REC_TN, tiles_m = (sc->M + BDF_REC_TM - 1) / BDF_REC_TM;
    const int64_t tiles = tiles_n * tiles_m;
    const dim3 grid((unsigned)std::min<int64_t>(tiles, (int64_t)std::max(ctx->n_cus, 1) * 8));
    const int DP = sc->D <= 16 ? 16 : (sc->D <= 32 ? 32 : 64);
    if (DP == 16) hipLaunchKernelGGL(k_scores_accum<16>, grid, dim3(256), 0, ctx->stream, sc->sum_dev, (const double *)sc->ring_dev, sc->n_rows, sc->M, sc->nblk, held, tiles_m, tiles);
    else if (DP == 32) hipLaunchKernelGGL(k_scores_accum<32>, grid, dim3(256), 0, ctx->stream, sc->sum_dev, (const double *)sc->ring_dev, sc->n_rows, sc->M, sc->nblk, held, tiles_m, tiles);
    else hipLaunchKernelGGL(k_scores_accum<64>, grid, dim3(256), 0, ctx->stream, sc->sum_dev, (const double *)sc->ring_dev, sc->n_rows, sc->M, sc->nblk, held, tiles_m, tiles);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}

int bdf_ring_push(bdf_ctx *ctx, const double *U, const double *V, const int32_t *rows_dev, int64_t n_rows, int64_t M, int D, int nblk, double *slot)
{
    const int64_t quads = (n_rows + M) * nblk;
    if (quads > 0) {
        const dim3 grid((unsigned)std::min<int64_t>((quads + 255) / 256, 65536));
        hipLaunchKernelGGL(k_scores_push, grid, dim3(256), 0, ctx->stream, U, V, rows_dev, n_rows, M, D, nblk, slot);
        BDF_HIP(hipGetLastError());
    }
    return BDF_OK;
}

extern "C" int bdf_scores_push(bdf_scores *sc, const double *U, const double *V)
{
    BDF_REQUIRE(sc && U && V, BDF_ERR_ARG, "bdf_scores_push: NULL argument");
    bdf_ctx *ctx = sc->ctx;
    BDF_HIP(hipSetDevice(ctx->device));
    const int64_t quads = (sc->n_rows + sc->M) * sc->nblk;
    const int rc = bdf_ring_push(ctx, U, V, sc->rows_dev, sc->n_rows, sc->M, sc->D, sc->nblk, sc->ring_dev + (int64_t)sc->held * quads * 4);
    if (rc) return rc;
    sc->held++;
    sc->draws += 1.0;
    return sc->held == sc->batch ? bdf_scores_flush(sc) : BDF_OK;
}

extern "C" int bdf_scores_copy(bdf_scores *sc, double *buf_dev, int64_t first, int64_t count, int write)
{
    BDF_REQUIRE(sc && buf_dev, BDF_ERR_ARG, "bdf_scores_copy: NULL argument");
    const int64_t cells = sc->n_rows * sc->M + BDF_REC_GUARD;
    BDF_REQUIRE(first >= 0 && count >= 0 && first <= cells && count <= cells - first, BDF_ERR_BOUNDS,
                "bdf_scores_copy: cells %lld .. %lld are outside the sum and its guard (%lld doubles)", (long long)first, (long long)(first + count), (long long)cells);
    const int rc = bdf_scores_flush(sc);
    if (rc) return rc;
    BDF_HIP(hipSetDevice(sc->ctx->device));
    if (count) BDF_HIP(hipMemcpyAsync(write ? sc->sum_dev + first : buf_dev, write ? buf_dev : sc->sum_dev + first, (size_t)count * sizeof(double),
                                      hipMemcpyDeviceToDevice, sc->ctx->stream));
    return BDF_OK;
}

extern "C" int bdf_scores_set_draws(bdf_scores *sc, double draws)
{
    BDF_REQUIRE(sc != nullptr && draws >= 0.0, BDF_ERR_ARG, "bdf_scores_set_draws: NULL argument or a negative count");
    BDF_REQUIRE(sc->held == 0, BDF_ERR_ARG, "bdf_scores_set_draws: %d draws are buffered (bdf_scores_flush first)", sc->held);
    sc->draws = draws;
    return BDF_OK;
}

int bdf_topk_plane(bdf_ctx *ctx, const char *who, const double *plane, int64_t n_rows, int64_t M, const int32_t *rows_dev,
                   const std::vector<int32_t> &rows_host, const bdf_rel *rel, int K, double draws, double mean_value, int32_t *items_out,
                   double *scores_out)
{
    BDF_REQUIRE(K >= 1 && K <= BDF_REC_MAX_K, BDF_ERR_ARG, "%s: K=%d must be in 1..%d", who, K, BDF_REC_MAX_K);
    const int64_t *rowptr = nullptr;
    const int32_t *colidx = nullptr;
    if (rel) {
        BDF_REQUIRE(rel->n_modes == 2 && !rel->sharded, BDF_ERR_ARG, "%s: the listed cells come from a two-mode relation on one rank", who);
        BDF_REQUIRE(rel->dims[1] == M, BDF_ERR_ARG, "%s: the relation has %lld columns, the scores %lld", who, (long long)rel->dims[1], (long long)M);
        const int64_t N = rel->dims[0];
        if (rows_dev) {
            for (int64_t r = 0; r < n_rows; r++)
                BDF_REQUIRE(rows_host[(size_t)r] < N, BDF_ERR_BOUNDS, "%s: rows[%lld] = %d is outside the relation's %lld rows", who, (long long)r,
                            rows_host[(size_t)r], (long long)N);
        } else {
            BDF_REQUIRE(n_rows <= N, BDF_ERR_ARG, "%s: %lld scored rows, the relation has %lld", who, (long long)n_rows, (long long)N);
        }
        rowptr = rel->idx[0].rowptr_dev; colidx = rel->idx[0].colidx_dev;
    }
    if (n_rows == 0) return BDF_OK;
    BDF_HIP(hipSetDevice(ctx->device));
    const dim3 grid((unsigned)std::min<int64_t>(n_rows, 1 << 20));
    hipLaunchKernelGGL(k_topk_rows, grid, dim3(64), 0, ctx->stream, plane, n_rows, M, rows_dev, rowptr, colidx, K, draws, mean_value, items_out, scores_out);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}

extern "C" int bdf_scores_topk(bdf_scores *sc, const bdf_rel *rel, int K, double mean_value, int32_t *items_out, double *scores_out)
{
    BDF_REQUIRE(sc && items_out && scores_out, BDF_ERR_ARG, "bdf_scores_topk: NULL argument");
    BDF_REQUIRE(K >= 1 && K <= BDF_REC_MAX_K, BDF_ERR_ARG, "bdf_scores_topk: K=%d must be in 1..%d", K, BDF_REC_MAX_K);
    const int rc = bdf_scores_flush(sc);
    if (rc) return rc;
    return bdf_topk_plane(sc->ctx, "bdf_scores_topk", sc->sum_dev, sc->n_rows, sc->M, sc->rows_dev, sc->rows_host, rel, K, sc->draws, mean_value,
                          items_out, scores_out);
}

extern "C" int bdf_scores_metrics(bdf_scores *sc, const int32_t *items, int K, const bdf_pairs *test, double class_cut, double *out)
{
    BDF_REQUIRE(sc && items && test && out, BDF_ERR_ARG, "bdf_scores_metrics: NULL argument");
    BDF_REQUIRE(K >= 1 && K <= BDF_REC_MAX_K, BDF_ERR_ARG, "bdf_scores_metrics: K=%d must be in 1..%d", K, BDF_REC_MAX_K);
    BDF_REQUIRE(test->n_modes == 2, BDF_ERR_ARG, "bdf_scores_metrics: the test cells belong to a two-mode relation, not %d modes", test->n_modes);
    bdf_ctx *ctx = sc->ctx;
    BDF_HIP(hipSetDevice(ctx->device));
    const int64_t n_rows = sc->n_rows;
    if (sc->rel_pairs != test || sc->rel_cut != class_cut || !sc->rel_ptr_dev) {
        // the relevant test cells (value > class_cut) by scored row, each row's items ascending and distinct
        const int64_t n = test->n;
        const int32_t *ti = test->ids_host.data(), *tj = ti + n;
        std::map<int32_t, int32_t> slot_of;
        if (sc->rows_dev)
            for (int64_t r = 0; r < n_rows; r++) slot_of[sc->rows_host[(size_t)r]] = (int32_t)r;
        std::vector<std::pair<int32_t, int32_t>> cells;
        for (int64_t k = 0; k < n; k++) {
            if (!(test->values_host[(size_t)k] > class_cut) || tj[k] >= sc->M) continue;
            int32_t r;
            if (sc->rows_dev) {
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
        if (sc->rel_ptr_dev) { hipFree(sc->rel_ptr_dev); sc->rel_ptr_dev = nullptr; }
        if (sc->rel_items_dev) { hipFree(sc->rel_items_dev); sc->rel_items_dev = nullptr; }
        int rc;
        if ((rc = bdf_upload(&sc->rel_ptr_dev, ptr))) return rc;
        if ((rc = bdf_upload(&sc->rel_items_dev, its))) return rc;
        if (!sc->row_metrics_dev) BDF_HIP(hipMalloc((void **)&sc->row_metrics_dev, std::max<size_t>((size_t)n_rows * 4 * sizeof(double), 16)));
        sc->rel_pairs = test; sc->rel_cut = class_cut;
    }
    if (n_rows > 0) {
        const dim3 grid((unsigned)std::min<int64_t>(n_rows, 1 << 20));
        hipLaunchKernelGGL(k_rec_metrics, grid, dim3(64), 0, ctx->stream, items, K, n_rows, (const int64_t *)sc->rel_ptr_dev, (const int32_t *)sc->rel_items_dev,
                           sc->row_metrics_dev);
    }
    hipLaunchKernelGGL(k_rec_metrics_final, dim3(1), dim3(256), 0, ctx->stream, (const double *)sc->row_metrics_dev, n_rows, sc->draws, out);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}
