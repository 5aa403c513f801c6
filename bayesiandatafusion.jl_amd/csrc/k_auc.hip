// k_auc.hip -- AUC_ROC (src/ROC.jl:1-11) and a fixed-order 2-norm, on the device.
//
// AUC_ROC sorts the scores with a STABLE sort (Julia's sortperm, numpy's argsort(kind="stable")) and integrates the ROC
// curve.  With P positives and Nn negatives that is C / (P Nn), where C counts the pairs (negative, positive) with the
// negative sorted before the positive: C = (sum of the positives' 0-based sorted positions) - P (P - 1) / 2.  C is an exact
// int64 here; the double is C / (P Nn), rounded once.  P = 0 or Nn = 0: NaN, as driver.AUC_ROC.
//
// The sort is a stable LSD radix sort of 64-bit order-preserving keys (8-bit digits) with a one-byte label payload:
//   k_auc_keys     keys and labels in the CALLER's order (sorted pairs are scattered through their permutation, so that
//                  ties break by the caller's index) and all eight digit histograms, in one read
//   k_auc_plan     which passes run: a digit whose histogram has one occupied bin leaves the order as it is and is skipped;
//                  decided on the device, so a report needs no read-back between the passes
//   per pass: k_auc_count (per-tile digit counts, digit-major), k_auc_scan (one workgroup per digit: the digit's base plus
//             an exclusive scan over the tiles = the global offset of every (digit, tile)), k_auc_scatter (stable rank
//             inside the tile: 64-bit ballot digit matching and popcount per 64 keys, the four waves combined in order
//             through LDS)
//   k_auc_sum      the positives' positions and their number (integer atomics: the result does not depend on their order)
//   k_auc_finish   C, P, Nn and the AUC
// No floating-point atomics, no workgroup waits for another.
#include "bdf_common.h"
#include <cmath>

namespace {

constexpr int AUC_THREADS = 256;
constexpr int AUC_WAVES = AUC_THREADS / 64;
constexpr int AUC_CHUNKS = 16;                                  // 64-key chunks per wave
constexpr int64_t AUC_TILE = (int64_t)AUC_THREADS * AUC_CHUNKS; // 4096 keys per tile
constexpr int AUC_PASSES = 8;
constexpr int AUC_HIST_GRID = 256;                              // workgroups of k_auc_keys (grid-stride)
constexpr uint64_t AUC_NAN_KEY = 0xFFF0000000000001ull;        // one above +inf's key

// order-preserving key: negatives ~bits, the rest bits | 1 << 63; -0.0 folded into +0.0, every NaN one key above +inf
__device__ inline uint64_t auc_key(double x)
{
    if (x != x) return AUC_NAN_KEY;
    const uint64_t b = x == 0.0 ? 0ull : (uint64_t)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | (1ull << 63));
}

// workspace: key[2] (8 n each), lab[2] (n each), hist (8 x 256 u32) and acc (2 u64) adjacent (one memset), plan, tile counts
struct AucWs {
    uint64_t *key0, *key1;
    uint8_t *lab0, *lab1;
    uint32_t *hist;                 // [pass][digit]
    unsigned long long *acc;        // {sum of the positives' sorted positions, P}
    int32_t *plan;                  // [0, 8): pass runs; [8, 16): the key buffer pass d reads; [16]: the buffer holding the result
    uint32_t *tcount;               // [digit][tile]: counts, then (scanned in place) global offsets
    int64_t ntiles;
};

inline size_t auc_align(size_t b) { return (b + 255) & ~(size_t)255; }

size_t auc_layout(int64_t n, char *base, AucWs *w)
{
    const int64_t ntiles = std::max<int64_t>(1, (n + AUC_TILE - 1) / AUC_TILE);
    const size_t kb = auc_align((size_t)std::max<int64_t>(n, 1) * 8), lb = auc_align((size_t)std::max<int64_t>(n, 1));
    const size_t hb = AUC_PASSES * 256 * 4 + 2 * 8, pb = auc_align(32 * 4), tb = auc_align((size_t)256 * ntiles * 4);
    size_t off = 0;
    if (w) {
        w->key0 = (uint64_t *)(base + off);
        w->key1 = (uint64_t *)(base + off + kb);
        w->lab0 = (uint8_t *)(base + off + 2 * kb);
        w->lab1 = (uint8_t *)(base + off + 2 * kb + lb);
    }
    off += 2 * kb + 2 * lb;
    if (w) {
        w->hist = (uint32_t *)(base + off);
        w->acc = (unsigned long long *)(base + off + AUC_PASSES * 256 * 4);
    }
    off += auc_align(hb);
    if (w) w->plan = (int32_t *)(base + off);
    off += pb;
    if (w) { w->tcount = (uint32_t *)(base + off); w->ntiles = ntiles; }
    off += tb;
    return off;
}

// keys and labels at the caller's index (orig: storage -> caller; NULL: identity) and the eight digit histograms.
// labels != NULL: label = labels[i] != 0, score = scores[i]; else label = values[i] < cut, score = -scores[i] (roc_avg of
// macau.jl:200: AUC_ROC(values .< class_cut, -avg))
__global__ __launch_bounds__(AUC_THREADS) void k_auc_keys(int64_t n, const uint8_t *labels, const double *scores,
                                                           const double *values, double cut, const int32_t *orig, AucWs w)
{
    __shared__ uint32_t h[AUC_PASSES][256];
    const int tid = threadIdx.x;
#pragma unroll
    for (int d = 0; d < AUC_PASSES; d++) h[d][tid] = 0;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * AUC_THREADS + tid; i < n; i += (int64_t)gridDim.x * AUC_THREADS) {
        const double s = labels ? scores[i] : -scores[i];
        const uint8_t lab = labels ? (labels[i] != 0) : (values[i] < cut);
        const uint64_t k = auc_key(s);
        const int64_t c = orig ? (int64_t)orig[i] : i;
        w.key0[c] = k;
        w.lab0[c] = lab;
#pragma unroll
        for (int d = 0; d < AUC_PASSES; d++) atomicAdd(&h[d][(k >> (8 * d)) & 255], 1u);
    }
    __syncthreads();
#pragma unroll
    for (int d = 0; d < AUC_PASSES; d++)
        if (h[d][tid]) atomicAdd(&w.hist[d * 256 + tid], h[d][tid]);
}

__global__ __launch_bounds__(AUC_THREADS) void k_auc_plan(int64_t n, AucWs w)
{
    __shared__ int one_bin[AUC_PASSES];
    const int tid = threadIdx.x;
    if (tid < AUC_PASSES) one_bin[tid] = 0;
    __syncthreads();
#pragma unroll
    for (int d = 0; d < AUC_PASSES; d++)
        if ((int64_t)w.hist[d * 256 + tid] == n) one_bin[d] = 1;       // (every writer writes 1)
    __syncthreads();
    if (tid == 0) {
        int buf = 0;
        for (int d = 0; d < AUC_PASSES; d++) {
            const int run = n > 0 && !one_bin[d];
            w.plan[d] = run;
            w.plan[AUC_PASSES + d] = buf;
            buf ^= run;
        }
        w.plan[2 * AUC_PASSES] = buf;
    }
}

__global__ __launch_bounds__(AUC_THREADS) void k_auc_count(int64_t n, int pass, AucWs w)
{
    if (!w.plan[pass]) return;
    const uint64_t *src = w.plan[AUC_PASSES + pass] ? w.key1 : w.key0;
    __shared__ uint32_t h[256];
    const int tid = threadIdx.x;
    h[tid] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * AUC_TILE;
#pragma unroll 4
    for (int c = 0; c < AUC_CHUNKS; c++) {
        const int64_t i = base + (int64_t)c * AUC_THREADS + tid;
        if (i < n) atomicAdd(&h[(src[i] >> (8 * pass)) & 255], 1u);
    }
    __syncthreads();
    w.tcount[(int64_t)tid * w.ntiles + blockIdx.x] = h[tid];
}

// exclusive scan of the 256 threads' values (wave scans, then the wave totals in order); returns the block total
__device__ inline uint32_t block_exclusive_scan(uint32_t x, uint32_t &excl)
{
    __shared__ uint32_t wt[AUC_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    uint32_t incl = x;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t y = __shfl_up(incl, off);
        if (lane >= off) incl += y;
    }
    if (lane == 63) wt[wv] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < AUC_WAVES; k++) {
        before += k < wv ? wt[k] : 0u;
        total += wt[k];
    }
    __syncthreads();                 // (wt is reused by the next call)
    excl = before + incl - x;
    return total;
}

// one workgroup per digit b: offset(b, tile) = (keys with a smaller digit) + (keys with digit b in earlier tiles)
__global__ __launch_bounds__(AUC_THREADS) void k_auc_scan(int pass, AucWs w)
{
    if (!w.plan[pass]) return;
    const int b = blockIdx.x, tid = threadIdx.x;
    const uint32_t *h = w.hist + pass * 256;
    if (h[b] == 0) return;                                        // no key has this digit: its offsets are never read
    uint32_t excl;
    uint32_t carry = block_exclusive_scan(tid < b ? h[tid] : 0u, excl);
    uint32_t *row = w.tcount + (int64_t)b * w.ntiles;
    for (int64_t start = 0; start < w.ntiles; start += AUC_THREADS) {
        const int64_t t = start + tid;
        const uint32_t x = t < w.ntiles ? row[t] : 0u;
        const uint32_t total = block_exclusive_scan(x, excl);
        if (t < w.ntiles) row[t] = carry + excl;
        carry += total;
    }
}

// stable scatter of one tile: wave wv takes the keys [tile + wv * 1024, tile + (wv + 1) * 1024) in 16 chunks of 64 in order
__global__ __launch_bounds__(AUC_THREADS) void k_auc_scatter(int64_t n, int pass, AucWs w)
{
    if (!w.plan[pass]) return;
    const int from = w.plan[AUC_PASSES + pass];
    const uint64_t *ksrc = from ? w.key1 : w.key0;
    uint64_t *kdst = from ? w.key0 : w.key1;
    const uint8_t *lsrc = from ? w.lab1 : w.lab0;
    uint8_t *ldst = from ? w.lab0 : w.lab1;
    __shared__ uint32_t cnt[AUC_WAVES][256];     // per wave: keys of each digit so far; then the wave's first position per digit
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int shift = 8 * pass;
#pragma unroll
    for (int k = 0; k < AUC_WAVES; k++) cnt[k][tid] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * AUC_TILE + (int64_t)wv * (AUC_CHUNKS * 64) + lane;
    const uint64_t lt = (1ull << lane) - 1ull;
    uint64_t key[AUC_CHUNKS];
    uint32_t rank[AUC_CHUNKS];
#pragma unroll
    for (int c = 0; c < AUC_CHUNKS; c++) {
        const int64_t i = base + (int64_t)c * 64;
        const bool valid = i < n;
        key[c] = valid ? ksrc[i] : 0ull;
    }
#pragma unroll
    for (int c = 0; c < AUC_CHUNKS; c++) {
        const int64_t i = base + (int64_t)c * 64;
        const bool valid = i < n;
        const uint32_t dg = (uint32_t)(key[c] >> shift) & 255u;
        // lanes of this chunk holding the same digit (valid lanes only)
        uint64_t match = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 8; bit++) {
            const bool set = (dg >> bit) & 1u;
            const uint64_t bb = __ballot(set);
            match &= set ? bb : ~bb;
        }
        const uint32_t prior = cnt[wv][dg];
        rank[c] = prior + (uint32_t)__popcll(match & lt);
        // the group's lowest lane advances the wave's count of the digit (every lane of the group read it above)
        if (valid && (match & lt) == 0ull) cnt[wv][dg] = prior + (uint32_t)__popcll(match);
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    {
        uint32_t off = w.tcount[(int64_t)tid * w.ntiles + blockIdx.x];
#pragma unroll
        for (int k = 0; k < AUC_WAVES; k++) {
            const uint32_t t = cnt[k][tid];
            cnt[k][tid] = off;
            off += t;
        }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < AUC_CHUNKS; c++) {
        const int64_t i = base + (int64_t)c * 64;
        if (i < n) {
            const uint32_t dg = (uint32_t)(key[c] >> shift) & 255u;
            const uint32_t pos = cnt[wv][dg] + rank[c];
            kdst[pos] = key[c];
            ldst[pos] = lsrc[i];
        }
    }
}

__global__ __launch_bounds__(AUC_THREADS) void k_auc_sum(int64_t n, AucWs w)
{
    __shared__ unsigned long long part[2][AUC_WAVES];
    const uint8_t *lab = w.plan[2 * AUC_PASSES] ? w.lab1 : w.lab0;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    unsigned long long s = 0, p = 0;
    for (int64_t i = (int64_t)blockIdx.x * AUC_THREADS + tid; i < n; i += (int64_t)gridDim.x * AUC_THREADS)
        if (lab[i]) { s += (unsigned long long)i; p += 1; }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        s += __shfl_xor(s, off);
        p += __shfl_xor(p, off);
    }
    if (lane == 0) { part[0][wv] = s; part[1][wv] = p; }
    __syncthreads();
    if (tid == 0) {
        unsigned long long S = 0, Pc = 0;
#pragma unroll
        for (int k = 0; k < AUC_WAVES; k++) { S += part[0][k]; Pc += part[1][k]; }
        if (Pc) { atomicAdd(&w.acc[0], S); atomicAdd(&w.acc[1], Pc); }
    }
}

__global__ void k_auc_finish(int64_t n, AucWs w, double *auc_out, int64_t *counts_out)
{
    if (threadIdx.x != 0) return;
    const int64_t S = (int64_t)w.acc[0], P = (int64_t)w.acc[1], Nn = n - P;
    const int64_t C = S - P * (P - 1) / 2;
    *auc_out = (P == 0 || Nn == 0) ? __builtin_nan("") : (double)C / ((double)P * (double)Nn);
    if (counts_out) { counts_out[0] = C; counts_out[1] = P; counts_out[2] = Nn; }
}

// ---- ||x||_2 in a fixed order: workgroup b sums the squares of a fixed contiguous range (lanes strided, waves in order),
// the partials are added in order by one workgroup
constexpr int NORM_MAX_BLOCKS = 1024;

__device__ inline double block_sum_fixed(double v)
{
    __shared__ double wsum[AUC_WAVES];
    const int tid = threadIdx.x;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    if ((tid & 63) == 0) wsum[tid >> 6] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < AUC_WAVES; k++) t += wsum[k];
    return t;
}

__global__ __launch_bounds__(AUC_THREADS) void k_norm2_part(int64_t n, int64_t per_block, const double *x, double *part)
{
    const int64_t lo = (int64_t)blockIdx.x * per_block, hi = std::min<int64_t>(n, lo + per_block);
    double s = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += AUC_THREADS) {
        const double v = x[i];
        s += v * v;
    }
    s = block_sum_fixed(s);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(AUC_THREADS) void k_norm2_final(int nblocks, const double *part, double *out)
{
    double s = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += AUC_THREADS) s += part[b];
    s = block_sum_fixed(s);
    if (threadIdx.x == 0) *out = sqrt(s);
}

constexpr int64_t AUC_MAX_N = (int64_t)1 << 31;     // positions and counts are 32-bit

int auc_enqueue(const char *who, bdf_ctx *ctx, int64_t n, const uint8_t *labels, const double *scores, const double *values,
                double cut, const int32_t *orig, void *workspace, double *auc_out, int64_t *counts_out)
{
    BDF_REQUIRE(n >= 0 && n < AUC_MAX_N - AUC_TILE, BDF_ERR_ARG, "%s: n=%lld out of range", who, (long long)n);
    BDF_REQUIRE(workspace && auc_out, BDF_ERR_ARG, "%s: NULL argument", who);
    BDF_REQUIRE(n == 0 || (scores && (labels || values)), BDF_ERR_ARG, "%s: NULL argument", who);
    AucWs w;
    auc_layout(n, (char *)workspace, &w);
    hipStream_t st = ctx->stream;
    BDF_HIP(hipMemsetAsync(w.hist, 0, AUC_PASSES * 256 * 4 + 2 * 8, st));
    if (n > 0) {
        const unsigned ntiles = (unsigned)w.ntiles;
        const unsigned kgrid = (unsigned)std::min<int64_t>(AUC_HIST_GRID, (n + AUC_THREADS - 1) / AUC_THREADS);
        hipLaunchKernelGGL(k_auc_keys, dim3(kgrid), dim3(AUC_THREADS), 0, st, n, labels, scores, values, cut, orig, w);
        hipLaunchKernelGGL(k_auc_plan, dim3(1), dim3(AUC_THREADS), 0, st, n, w);
        for (int d = 0; d < AUC_PASSES; d++) {
            hipLaunchKernelGGL(k_auc_count, dim3(ntiles), dim3(AUC_THREADS), 0, st, n, d, w);
            hipLaunchKernelGGL(k_auc_scan, dim3(256), dim3(AUC_THREADS), 0, st, d, w);
            hipLaunchKernelGGL(k_auc_scatter, dim3(ntiles), dim3(AUC_THREADS), 0, st, n, d, w);
        }
        const unsigned sgrid = (unsigned)std::min<int64_t>(1024, (n + AUC_THREADS * 4 - 1) / (AUC_THREADS * 4));
        hipLaunchKernelGGL(k_auc_sum, dim3(sgrid), dim3(AUC_THREADS), 0, st, n, w);
    }
    hipLaunchKernelGGL(k_auc_finish, dim3(1), dim3(64), 0, st, n, w, auc_out, counts_out);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}

}  // namespace

extern "C" int64_t bdf_auc_workspace_bytes(int64_t n)
{
    if (n < 0) return -1;
    return (int64_t)auc_layout(n, nullptr, nullptr);
}

extern "C" int bdf_auc_roc(bdf_ctx *ctx, int64_t n, const uint8_t *labels, const double *scores, void *workspace,
                           double *auc_out, int64_t *counts_out)
{
    BDF_REQUIRE(ctx != nullptr, BDF_ERR_ARG, "bdf_auc_roc: NULL context");
    BDF_REQUIRE(n == 0 || labels, BDF_ERR_ARG, "bdf_auc_roc: labels is NULL");
    return auc_enqueue("bdf_auc_roc", ctx, n, labels, scores, nullptr, 0.0, nullptr, workspace, auc_out, counts_out);
}

extern "C" int bdf_pairs_auc(bdf_ctx *ctx, bdf_pairs *p, double class_cut, double *auc_out, int64_t *counts_out)
{
    BDF_REQUIRE(ctx && p, BDF_ERR_ARG, "bdf_pairs_auc: NULL argument");
    if (!p->auc_ws) {
        // (first use: the pairs' previous work may still be in flight on their streams; the allocation does not wait for it, and
        // nothing reads the block before the launches below)
        const size_t bytes = (size_t)bdf_auc_workspace_bytes(p->n);
        BDF_HIP(hipSetDevice(ctx->device));
        if (int rc = p->auc_ws.alloc_bytes(bytes)) return rc;
    }
    return auc_enqueue("bdf_pairs_auc", ctx, p->n, nullptr, p->avg_dev, p->values_dev, class_cut, p->orig_dev, p->auc_ws,
                       auc_out, counts_out);
}

extern "C" int bdf_norm2(bdf_ctx *ctx, int64_t n, const double *x, double *out)
{
    BDF_REQUIRE(ctx && out && (n == 0 || x), BDF_ERR_ARG, "bdf_norm2: NULL argument");
    BDF_REQUIRE(n >= 0, BDF_ERR_ARG, "bdf_norm2: n=%lld < 0", (long long)n);
    if (!ctx->norm_part) {
        BDF_HIP(hipSetDevice(ctx->device));
        if (int rc = ctx->norm_part.alloc(NORM_MAX_BLOCKS)) return rc;
    }
    const int64_t chunk = (int64_t)AUC_THREADS * 16;
    const int nblocks = (int)std::max<int64_t>(1, std::min<int64_t>(NORM_MAX_BLOCKS, (n + chunk - 1) / chunk));
    const int64_t per_block = (n + nblocks - 1) / nblocks;
    hipLaunchKernelGGL(k_norm2_part, dim3(nblocks), dim3(AUC_THREADS), 0, ctx->stream, n, per_block, x, ctx->norm_part);
    hipLaunchKernelGGL(k_norm2_final, dim3(1), dim3(AUC_THREADS), 0, ctx->stream, nblocks, (const double *)ctx->norm_part, out);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}
