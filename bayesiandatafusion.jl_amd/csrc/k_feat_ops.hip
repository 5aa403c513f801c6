// k_feat_ops.hip -- K2..K5: the side-information (Entity.F) operators.
//
//   Entity.F operator contract: F*B, At_mul_B(F,B), AtA_mul_B! for dense F, SparseMatrixCSR
//   (src/parallel_csr.jl:36-54) and binary sparse F (src/sparsebin_csr.jl:22-63, src/parallel_matrix.jl:19-24,
//   242-267).  Sparse operators keep the CSR of F and the CSR of F' so that both products are row gathers with
//   no atomics (the reference's COO At_mul_B! scatters, parallel_matrix.jl:258-267).
//   uhat = (F beta)'                                   F_mul_beta, src/RelationData.jl:314-320; macau.jl:103,112
#include "feat.h"
#include "wave_linalg.h"
#include "dpp_rows16.h"
#include <algorithm>
#include <cmath>

namespace {

// ---- strided dense GEMM: C(i,j) = sum_k A(i,k) B(k,j), optional second output C2 = C + bias[j] -------------
constexpr int TM = 32, TN = 32, TK = 16;

// blockIdx.z = K chunk (split-K): with more than one chunk the tile goes to part[z][i][j] (M x N row-major per chunk) and
// k_gemm_reduce adds the chunks in order -- a tall-and-skinny F' T (K = rows of F) would otherwise run on a handful of CUs
__global__ __launch_bounds__(256) void k_gemm(GemmArgs g, int64_t kchunk, double *part, const int *skip)
{
    if (skip && *skip == 0) return;
    __shared__ double As[TK][TM + 1];
    __shared__ double Bs[TK][TN + 1];
    const int tid = threadIdx.x;
    const int tx = tid % 16, ty = tid / 16;
    const int64_t i0 = (int64_t)blockIdx.x * TM, j0 = (int64_t)blockIdx.y * TN;
    const int64_t kb = (int64_t)blockIdx.z * kchunk, ke = (kb + kchunk < g.K) ? kb + kchunk : g.K;
    double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
    const bool a_fast_i = g.ars <= g.acs, b_fast_k = g.brs <= g.bcs;
    for (int64_t k0 = kb; k0 < ke; k0 += TK) {
        for (int e = tid; e < TM * TK; e += 256) {
            const int ii = a_fast_i ? e % TM : e / TK, kk = a_fast_i ? e / TM : e % TK;
            const int64_t i = i0 + ii, k = k0 + kk;
            As[kk][ii] = (i < g.M && k < ke) ? g.A[i * g.ars + k * g.acs] : 0.0;
        }
        for (int e = tid; e < TN * TK; e += 256) {
            const int kk = b_fast_k ? e % TK : e / TN, jj = b_fast_k ? e / TK : e % TN;
            const int64_t k = k0 + kk, j = j0 + jj;
            Bs[kk][jj] = (k < ke && j < g.N) ? g.B[k * g.brs + j * g.bcs] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < TK; kk++) {
            const double a0 = As[kk][tx], a1 = As[kk][tx + 16];
            const double b0 = Bs[kk][ty], b1 = Bs[kk][ty + 16];
            acc[0][0] = fma(a0, b0, acc[0][0]); acc[0][1] = fma(a0, b1, acc[0][1]);
            acc[1][0] = fma(a1, b0, acc[1][0]); acc[1][1] = fma(a1, b1, acc[1][1]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < 2; u++)
#pragma unroll
        for (int v = 0; v < 2; v++) {
            const int64_t i = i0 + tx + 16 * u, j = j0 + ty + 16 * v;
            if (i < g.M && j < g.N) {
                if (part) {
                    part[((int64_t)blockIdx.z * g.M + i) * g.N + j] = acc[u][v];
                } else {
                    g.C[i * g.crs + j * g.ccs] = acc[u][v];
                    if (g.C2) g.C2[i * g.crs + j * g.ccs] = acc[u][v] + g.bias[j];
                }
            }
        }
}

__global__ __launch_bounds__(256) void k_gemm_reduce(GemmArgs g, int nchunks, const double *part, const int *skip)
{
    if (skip && *skip == 0) return;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= g.M * g.N) return;
    const int64_t i = e / g.N, j = e % g.N;
    double s = 0.0;
    for (int z = 0; z < nchunks; z++) s += part[(int64_t)z * g.M * g.N + e];       // fixed order
    g.C[i * g.crs + j * g.ccs] = s;
    if (g.C2) g.C2[i * g.crs + j * g.ccs] = s + g.bias[j];
}

}  // namespace

int feat_gemm(bdf_ctx *ctx, const GemmArgs &g)
{
    if (g.M == 0 || g.N == 0) return BDF_OK;
    const int64_t tiles = ((g.M + TM - 1) / TM) * ((g.N + TN - 1) / TN);
    int nchunks = 1;
    if (tiles < 512 && g.K >= 128) {                       // too few tiles to fill the chip and a long K: split it
        nchunks = (int)std::min<int64_t>(64, std::min<int64_t>((g.K + 63) / 64, (1024 + tiles - 1) / tiles));
        if (nchunks < 1) nchunks = 1;
    }
    dim3 grid((unsigned)((g.M + TM - 1) / TM), (unsigned)((g.N + TN - 1) / TN), (unsigned)nchunks);
    if (nchunks == 1) {
        hipLaunchKernelGGL(k_gemm, grid, dim3(256), 0, ctx->stream, g, g.K, (double *)nullptr, ctx->skip_flag);
    } else {
        void *sc;
        int rc = bdf_scratch2(ctx, (size_t)nchunks * g.M * g.N * sizeof(double), &sc);
        if (rc) return rc;
        const int64_t kchunk = ((g.K + nchunks - 1) / nchunks + TK - 1) / TK * TK;
        hipLaunchKernelGGL(k_gemm, grid, dim3(256), 0, ctx->stream, g, kchunk, (double *)sc, ctx->skip_flag);
        hipLaunchKernelGGL(k_gemm_reduce, dim3((unsigned)((g.M * g.N + 255) / 256)), dim3(256), 0, ctx->stream, g, nchunks,
                           (const double *)sc, ctx->skip_flag);
    }
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}

namespace {

// ---- dense feature matrices on the matrix cores (v_mfma_f64_16x16x4_f64), at most 64 right-hand columns --------------
// F is N x numF column-major.  These are the two genuinely dense contractions of the path (F beta and F' T over
// the 24 MB of a 6040 x 500 F, AI ~ 8 flop/B per pass).

// Y(r, c) = sum_k F(r, k) B(k, c) for a column-major F: one wave per 16 rows x all columns, every operand straight from
// global memory in the MFMA's lane layout, no LDS, no barrier.  Lane (i = l & 15, h = l >> 4) supplies F(row i, k) -- 16
// consecutive rows of a column are one 128-byte read -- and B(k, column i).  Which k of a 16-chunk a lane takes in MFMA
// step t is free as long as A and B agree: k = 4h + t when B is column-major (the lane's four values of B are then 32
// contiguous bytes), k = 4t + h otherwise (the 16 lanes of an h read 128 contiguous bytes of a row of B).  B is small
// (K x ncol) and shared by all waves: it stays in L1/L2.  The chunk after the current one is loaded before the current
// one's MFMAs.  The four waves of a workgroup share the 16 rows and split K (a 500 x 500 F'F has only 32 row tiles), wave
// 0 adds their results in wave order.  (A version that staged B through LDS for four waves of different rows took 36 us
// for the 6040 x 500 x 32 product and as long for the 500 x 500 x 32 one: 95 resp. 8 workgroups, two barriers per 64 k.)
template <int CB, bool CM>
__global__ __launch_bounds__(256) void k_dense_nn(const double *__restrict__ F, int64_t M, int64_t K, const double *__restrict__ B,
                                                 int64_t brs, int64_t bcs, int ncol, double *__restrict__ Y, int64_t yrs,
                                                 int64_t ycs, const double *__restrict__ bias, double *__restrict__ Y2,
                                                 const int *skip)
{
    __shared__ double red[3][CB][4][64];
    if (skip && *skip == 0) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, h = lane >> 4;
    const int64_t r0 = (int64_t)blockIdx.x * 16;
    const int64_t row = r0 + i;
    const bool rok = row < M;
    const int64_t kq = ((K + 3) / 4 + 15) / 16 * 16;      // this wave's K range: [kb, ke)
    const int64_t kb = wave * kq, ke = (kb + kq < K) ? kb + kq : K;
    fd4 acc[CB];
#pragma unroll
    for (int cb = 0; cb < CB; cb++) acc[cb] = fd4{0.0, 0.0, 0.0, 0.0};
    double a[2][4], b[2][CB][4];
    auto load = [&](int64_t k0, int S) {
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int64_t k = k0 + (CM ? 4 * h + t : 4 * t + h);
            const bool kok = k < ke;
            a[S][t] = (rok && kok) ? F[row + k * M] : 0.0;
#pragma unroll
            for (int cb = 0; cb < CB; cb++) {
                const int c = 16 * cb + i;
                b[S][cb][t] = (kok && c < ncol) ? B[k * brs + (int64_t)c * bcs] : 0.0;
            }
        }
    };
    load(kb, 0);
    for (int64_t k0 = kb; k0 < ke; k0 += 32) {
        load(k0 + 16, 1);                               // beyond the range: zeros
#pragma unroll
        for (int t = 0; t < 4; t++)
#pragma unroll
            for (int cb = 0; cb < CB; cb++) acc[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[0][t], b[0][cb][t], acc[cb], 0, 0, 0);
        load(k0 + 32, 0);
#pragma unroll
        for (int t = 0; t < 4; t++)
#pragma unroll
            for (int cb = 0; cb < CB; cb++) acc[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[1][t], b[1][cb][t], acc[cb], 0, 0, 0);
    }
    if (wave > 0) {
#pragma unroll
        for (int cb = 0; cb < CB; cb++)
#pragma unroll
            for (int r = 0; r < 4; r++) red[wave - 1][cb][r][lane] = acc[cb][r];
    }
    __syncthreads();
    if (wave > 0) return;
#pragma unroll
    for (int cb = 0; cb < CB; cb++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const double v = ((acc[cb][r] + red[0][cb][r][lane]) + red[1][cb][r][lane]) + red[2][cb][r][lane];
            const int64_t rr = r0 + h + 4 * r;
            const int c = 16 * cb + i;
            if (rr < M && c < ncol) {
                Y[rr * yrs + (int64_t)c * ycs] = v;
                if (Y2) Y2[rr * yrs + (int64_t)c * ycs] = v + bias[c];
            }
        }
}

// part[z][f][c] = sum over the rows of chunk z of F(row, f) B(row, c)   (= F' B by chunks; k_gemm_reduce adds the chunks
// in order).  A workgroup owns 16 features and one row chunk; its waves take 64-row tiles in turn: the F tile goes through
// LDS (read along the rows, 512 contiguous bytes per feature; the MFMA wants feature-major), B operands from global.
template <int CB>
__global__ __launch_bounds__(256) void k_dense_tn(const double *__restrict__ F, int64_t M, int64_t numF, const double *__restrict__ B,
                                                  int64_t brs, int64_t bcs, int ncol, int64_t rows_per_chunk,
                                                  double *__restrict__ part, const int *skip)
{
    __shared__ double tile[4][16][65];
    if (skip && *skip == 0) return;
    __shared__ double red[3][CB][4][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 15, h = lane >> 4;
    const int64_t f0 = (int64_t)blockIdx.x * 16;
    const int64_t c0 = (int64_t)blockIdx.y * rows_per_chunk, c1 = (c0 + rows_per_chunk < M) ? c0 + rows_per_chunk : M;
    fd4 acc[CB];
#pragma unroll
    for (int cb = 0; cb < CB; cb++) acc[cb] = fd4{0.0, 0.0, 0.0, 0.0};
    for (int64_t rr = c0 + 64 * wave; rr < c1; rr += 256) {
        const int64_t myrow = rr + lane;
#pragma unroll
        for (int ff = 0; ff < 16; ff++)
            tile[wave][ff][lane] = (myrow < c1 && f0 + ff < numF) ? F[myrow + (f0 + ff) * M] : 0.0;
        double b[16][CB];
#pragma unroll
        for (int s = 0; s < 16; s++) {
            const int64_t row = rr + 4 * s + h;
#pragma unroll
            for (int cb = 0; cb < CB; cb++) {
                const int c = 16 * cb + i;
                b[s][cb] = (row < c1 && c < ncol) ? B[row * brs + (int64_t)c * bcs] : 0.0;
            }
        }
        wave_sync();
#pragma unroll
        for (int s = 0; s < 16; s++) {
            const double a = tile[wave][i][4 * s + h];
#pragma unroll
            for (int cb = 0; cb < CB; cb++) acc[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[s][cb], acc[cb], 0, 0, 0);
        }
        wave_sync();
    }
    if (wave > 0)
#pragma unroll
        for (int cb = 0; cb < CB; cb++)
#pragma unroll
            for (int r = 0; r < 4; r++) red[wave - 1][cb][r][lane] = acc[cb][r];
    __syncthreads();
    if (wave == 0) {
        double *p = part + (int64_t)blockIdx.y * numF * ncol;
#pragma unroll
        for (int cb = 0; cb < CB; cb++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                double v = acc[cb][r];
#pragma unroll
                for (int w = 0; w < 3; w++) v += red[w][cb][r][lane];
                const int64_t ff = f0 + h + 4 * r;
                const int c = 16 * cb + i;
                if (ff < numF && c < ncol) p[ff * ncol + c] = v;
            }
    }
}

}  // namespace

// Y = A B for a dense column-major M x K matrix A (a feature matrix, or the precomputed F'F), ncol <= 64
int feat_dense_nn(bdf_ctx *ctx, const double *A, int64_t M, int64_t K, const double *B, int64_t brs, int64_t bcs, int ncol,
                  double *Y, int64_t yrs, int64_t ycs, const double *bias, double *Y2)
{
    const int CB = (ncol + 15) / 16;
    const bool cm = brs == 1 && bcs != 1;         // column-major B
    dim3 grid((unsigned)((M + 15) / 16));
#define NN(C) do { if (cm) hipLaunchKernelGGL((k_dense_nn<C, true>), grid, dim3(256), 0, ctx->stream, A, M, K, B, brs, bcs, ncol, Y, yrs, ycs, bias, Y2, ctx->skip_flag); \
                   else hipLaunchKernelGGL((k_dense_nn<C, false>), grid, dim3(256), 0, ctx->stream, A, M, K, B, brs, bcs, ncol, Y, yrs, ycs, bias, Y2, ctx->skip_flag); } while (0)
    if (CB == 1) NN(1); else if (CB == 2) NN(2); else if (CB == 3) NN(3); else NN(4);
#undef NN
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}

namespace {

#ifndef BDF_TN_WGS
#define BDF_TN_WGS 1024       // workgroups the F' B product aims at (feature tiles x row chunks)
#endif
int dense_apply(bdf_ctx *ctx, const bdf_feat *f, bool transpose, const double *B, int64_t brs, int64_t bcs, int ncol,
                double *Y, int64_t yrs, int64_t ycs, const double *bias, double *Y2)
{
    const int CB = (ncol + 15) / 16;
    if (!transpose) return feat_dense_nn(ctx, f->dense_dev, f->m, f->n, B, brs, bcs, ncol, Y, yrs, ycs, bias, Y2);
    const int64_t ftiles = (f->n + 15) / 16;
    int64_t nchunks = std::max<int64_t>(1, std::min<int64_t>((f->m + 255) / 256, (BDF_TN_WGS + ftiles - 1) / ftiles));
    const int64_t rpc = ((f->m + nchunks - 1) / nchunks + 63) / 64 * 64;
    nchunks = (f->m + rpc - 1) / rpc;
    void *sc;
    int rc = bdf_scratch2(ctx, (size_t)nchunks * f->n * ncol * sizeof(double), &sc);
    if (rc) return rc;
    dim3 grid((unsigned)ftiles, (unsigned)nchunks);
#define TN(C) hipLaunchKernelGGL(k_dense_tn<C>, grid, dim3(256), 0, ctx->stream, (const double *)f->dense_dev, f->m, f->n, B, brs, bcs, ncol, rpc, (double *)sc, ctx->skip_flag)
    if (CB == 1) TN(1); else if (CB == 2) TN(2); else if (CB == 3) TN(3); else TN(4);
#undef TN
    GemmArgs g;
    g.M = f->n; g.N = ncol; g.K = f->m; g.A = nullptr; g.ars = g.acs = 0; g.B = nullptr; g.brs = g.bcs = 0;
    g.C = Y; g.crs = yrs; g.ccs = ycs; g.bias = bias; g.C2 = Y2;
    hipLaunchKernelGGL(k_gemm_reduce, dim3((unsigned)((g.M * g.N + 255) / 256)), dim3(256), 0, ctx->stream, g, (int)nchunks,
                       (const double *)sc, ctx->skip_flag);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}

// ---- sparse (CSR) x dense: Y(r,c) = sum_q val_q B(col_q, c); vals == NULL means implicit 1.0 ------------------
// The kernel wants both dense operands ROW-major (a gathered row of B is then one contiguous read of 8 ncol bytes shared
// by the lanes that walk the columns; with a column-major B every nonzero touches ncol different cache lines: measured
// 2.0 ms per product on config C5's 100,000 x 50,000 binary matrix, 5M nonzeros, 32 columns, against ~0.3 ms).  Operands in
// another layout -- the CG state and beta are column-major like the reference's matrices -- pass through a tiled transpose
// into / out of scratch.
struct SpmmArgs {
    int64_t m, kin; int ncol;        // m rows of the sparse operand (outputs), kin rows of B
    const int64_t *rowptr; const int32_t *colind; const double *vals;
    const double *B; int64_t brs, bcs;
    double *Y; int64_t yrs, ycs;
    const double *bias; double *Y2;
    const int64_t *panel_ptr = nullptr; int n_panels = 0;     // column panels of the sparse operand (bdf_feat::panel_*), or none
};

// rows of B per column panel: 3 MiB of a 32-column operand (a 4 MiB XCD L2 keeps the panel beside the streams of the launch)
#define BDF_SPMM_PANEL_ROWS 12288

// B(i,c) at B[i*ldb + c], Y(r,c) at Y[r*ldy + c].  32 lanes walk the columns, 8 rows per block; the row's nonzeros four at a
// time (independent gathers), accumulated in order (the result does not depend on the unrolling).
__global__ __launch_bounds__(256) void k_spmm_rm(int64_t m, int ncol, const int64_t *__restrict__ rowptr,
                                                 const int32_t *__restrict__ colind, const double *__restrict__ vals,
                                                 const double *__restrict__ B, int64_t ldb, double *__restrict__ Y, int64_t ldy,
                                                 const double *__restrict__ bias, double *__restrict__ Y2, const int *skip)
{
    if (skip && *skip == 0) return;
    const int c0 = threadIdx.x % 32;
    const int64_t r = (int64_t)blockIdx.x * 8 + threadIdx.x / 32;
    if (r >= m) return;
    const int64_t beg = rowptr[r], end = rowptr[r + 1];
    for (int c = c0; c < ncol; c += 32) {
        double acc = 0.0;
        int64_t q = beg;
        for (; q + 4 <= end; q += 4) {
            const int32_t i0 = colind[q], i1 = colind[q + 1], i2 = colind[q + 2], i3 = colind[q + 3];
            const double b0 = B[(int64_t)i0 * ldb + c], b1 = B[(int64_t)i1 * ldb + c], b2 = B[(int64_t)i2 * ldb + c],
                         b3 = B[(int64_t)i3 * ldb + c];
            if (vals) {
                acc = fma(vals[q], b0, acc); acc = fma(vals[q + 1], b1, acc);
                acc = fma(vals[q + 2], b2, acc); acc = fma(vals[q + 3], b3, acc);
            } else {
                acc = fma(1.0, b0, acc); acc = fma(1.0, b1, acc); acc = fma(1.0, b2, acc); acc = fma(1.0, b3, acc);
            }
        }
        for (; q < end; q++) acc = fma(vals ? vals[q] : 1.0, B[(int64_t)colind[q] * ldb + c], acc);
        Y[r * ldy + c] = acc;
        if (Y2) Y2[r * ldy + c] = acc + bias[c];
    }
}

// The same product for up to 32 columns taken in pairs (C5: D = 32, 5 M nonzeros; the kernel above ran 149 us per product there,
// 0.05 of what its bytes cost at the HBM rate -- four 8-byte gathers in flight per lane, one dependent round trip after the
// other).  SIXTEEN lanes per row, 16 bytes per lane (a 256-byte row of B is one instruction of the lane row), four rows per wave,
// sixteen rows per workgroup; a row's column indices come sixteen at a time -- lane l of the lane row loads index l of the chunk,
// one coalesced read -- and are handed round by DPP row broadcasts, and all (up to) sixteen gathers of a chunk are issued before
// the first is used: 256 bytes x 16 x 4 rows = 16 KB in flight per wave.  Same sums in the same order as k_spmm_rm (entry q of
// the row after entry q - 1): the two kernels agree to the last bit.
typedef double spd2 __attribute__((ext_vector_type(2)));
template <int J>
__device__ __forceinline__ void spmm_gather16(spd2 (&g)[16], int32_t myi, int left, const double *__restrict__ B, int64_t ldb, int c, bool cv)
{
    if constexpr (J < 16) {
        const int32_t ij = (int32_t)row_bcast_u32<J>((uint32_t)myi);
        g[J] = (cv && J < left) ? *(const spd2 *)(B + (int64_t)ij * ldb + c) : spd2{0.0, 0.0};
        spmm_gather16<J + 1>(g, myi, left, B, ldb, c, cv);
    }
}
template <bool HASV, int J>
__device__ __forceinline__ void spmm_acc16(const spd2 (&g)[16], double myv, int left, double &a0, double &a1)
{
    if constexpr (J < 16) {
        const double w = HASV ? row_bcast_f64<J>(myv) : (J < left ? 1.0 : 0.0);
        a0 = fma(w, g[J][0], a0);
        a1 = fma(w, g[J][1], a1);
        spmm_acc16<HASV, J + 1>(g, myv, left, a0, a1);
    }
}
template <bool HASV>
__global__ __launch_bounds__(256) void k_spmm_rm16(int64_t m, int ncol, const int64_t *__restrict__ rowptr,
                                                   const int32_t *__restrict__ colind, const double *__restrict__ vals,
                                                   const double *__restrict__ B, int64_t ldb, double *__restrict__ Y, int64_t ldy,
                                                   const double *__restrict__ bias, double *__restrict__ Y2, const int *skip)
{
    if (skip && *skip == 0) return;
    const int l = threadIdx.x & 15;
    const int64_t r = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    const bool rv = r < m;                       // (every lane stays: the broadcasts run over whole lane rows)
    const int64_t beg = rv ? rowptr[r] : 0, end = rv ? rowptr[r + 1] : 0;
    const int c = 2 * l;
    const bool cv = c < ncol;
    double a0 = 0.0, a1 = 0.0;
    // (the longest row of the wave sets the trip count: wave-uniform, the DPP instructions never sit under a divergent branch)
    int64_t nq = end - beg;
    nq = max(nq, __shfl_xor(nq, 16));
    nq = max(nq, __shfl_xor(nq, 32));
    nq = __builtin_amdgcn_readfirstlane((int)nq);
    // (the NEXT chunk's indices -- and values -- are loaded before this chunk's gathers are issued: a chunk then costs one dependent
    // round trip, its gathers, instead of two)
    int32_t myi = beg + l < end ? colind[beg + l] : 0;
    double myv = 0.0;
    if (HASV) myv = beg + l < end ? vals[beg + l] : 0.0;
    for (int64_t o = 0; o < nq; o += 16) {
        const int left = (int)min((int64_t)16, end - beg - o);          // entries of this lane row's chunk (<= 0: none)
        const int64_t qn = beg + o + 16 + l;
        const int32_t nxi = qn < end ? colind[qn] : 0;
        double nxv = 0.0;
        if (HASV) nxv = qn < end ? vals[qn] : 0.0;
        spd2 g[16];
        spmm_gather16<0>(g, myi, left, B, ldb, c, cv);
        spmm_acc16<HASV, 0>(g, myv, left, a0, a1);
        myi = nxi; myv = nxv;
    }
    if (rv && cv) {
        *(spd2 *)(Y + r * ldy + c) = spd2{a0, a1};
        if (Y2) *(spd2 *)(Y2 + r * ldy + c) = spd2{a0 + bias[c], a1 + bias[c + 1]};
    }
}

// The column panels of a product in ONE launch (round 6; until then one launch of the kernel above per panel, the rows' running
// sums carried through Y: 5 + 9 launches per F'(F p) on configuration C5, and Y -- 25.6 MB -- written and read back between them).
// A PERSISTENT grid, one workgroup per resident slot: workgroup w owns the row blocks w, w + G, ... (KB of them, sixteen rows
// each), walks the panels in order and inside a panel its row blocks, and keeps every row's two running sums in registers from the
// first panel to the last -- Y is written once.  Nothing synchronises the workgroups: they start together and do the same amount of
// work per panel, so the chip is inside one panel (two at the edges) at any moment and every XCD's L2 holds the 3 MiB of the operand
// its gathers want.  A row's entries are taken in the order of k_spmm_rm16 (column order: panel after panel): the same sums to the
// last bit.  The walk is pipelined over the units (row block, panel): the unit after the next one's bounds and the next one's
// first sixteen indices are loaded before this unit's gathers are issued -- a unit of ~10 entries per row is ONE dependent round
// trip, its gathers.
template <bool HASV>
__global__ __launch_bounds__(256, 4) void k_spmm_rm16p(int64_t m, int ncol, const int32_t *__restrict__ colind, const double *__restrict__ vals,
                                                       const double *__restrict__ B, int64_t ldb, double *__restrict__ Y, int64_t ldy,
                                                       const double *__restrict__ bias, double *__restrict__ Y2, const int *skip,
                                                       const int64_t *__restrict__ panel_ptr, int np, int KB, int64_t rb0, int64_t nblocks)
{
    // the rows' running sums: KB pairs per thread, in LDS (in registers they cost the kernel its fourth wave per SIMD -- and a grid
    // sized for four that holds three runs its last quarter as a second generation, out of step with the panels)
    extern __shared__ __attribute__((aligned(16))) double spmm_acc[];
    // (A counter the workgroups add to after every panel and briefly wait on was tried as a hint to keep them in step: its ~900
    // pollers on one word starve the arrivals -- every wait ran into its bound, 510 us per product instead of 120.  Not kept.)
    if (skip && *skip == 0) return;
    const int l = threadIdx.x & 15;
    const int c = 2 * l;
    const bool cv = c < ncol;
    const int64_t G = gridDim.x;
    spd2 *acc = (spd2 *)spmm_acc + threadIdx.x;                   // pair k of this thread: acc[k * 256]
    for (int k = 0; k < KB; k++) acc[k * 256] = spd2{0.0, 0.0};
    // unit u = p * KB + k: row block rb0 + blockIdx.x + k G, panel p
    auto row_of = [&](int k) -> int64_t {
        const int64_t rb = rb0 + blockIdx.x + (int64_t)k * G;
        const int64_t r = rb * 16 + (threadIdx.x >> 4);
        return (rb < nblocks && r < m) ? r : -1;
    };
    const int n_units = np * KB;
    // the pipeline's registers: bounds two units ahead, bounds + first indices one unit ahead
    int64_t b2 = 0, e2 = 0, b1 = 0, e1 = 0;
    int32_t i1 = 0;
    double v1 = 0.0;
    int k2 = 0, p2 = 0;                                           // (k, p) of the unit whose bounds are loaded next
    auto bounds = [&](int64_t &b, int64_t &e) {
        b = e = 0;
        if (p2 < np) {
            const int64_t r = row_of(k2);
            if (r >= 0) { const int64_t *pp = panel_ptr + (int64_t)p2 * m + r; b = pp[0]; e = pp[m]; }
        }
        if (++k2 == KB) { k2 = 0; p2++; }
    };
    bounds(b1, e1);
    bounds(b2, e2);
    i1 = b1 + l < e1 ? colind[b1 + l] : 0;
    if (HASV) v1 = b1 + l < e1 ? vals[b1 + l] : 0.0;
    (void)n_units;
#pragma unroll 1
    for (int p = 0; p < np; p++) {
#pragma unroll 1
        for (int k = 0; k < KB; k++) {
            const int64_t beg = b1, end = e1;
            int32_t myi = i1;
            double myv = v1;
            // the next unit's first indices and the one after's bounds: in flight under this unit's gathers
            b1 = b2; e1 = e2;
            i1 = b1 + l < e1 ? colind[b1 + l] : 0;
            if (HASV) v1 = b1 + l < e1 ? vals[b1 + l] : 0.0;
            bounds(b2, e2);
            int64_t nq = end - beg;
            nq = max(nq, __shfl_xor(nq, 16));
            nq = max(nq, __shfl_xor(nq, 32));
            nq = __builtin_amdgcn_readfirstlane((int)nq);
            if (nq <= 0) continue;
            spd2 av = acc[k * 256];
            double a0 = av[0], a1 = av[1];
            for (int64_t o = 0; o < nq; o += 16) {
                const int left = (int)min((int64_t)16, end - beg - o);
                const int64_t qn = beg + o + 16 + l;
                int32_t nxi = 0;
                double nxv = 0.0;
                if (o + 16 < nq) {                                   // (rare: a row with more than sixteen entries in one panel)
                    nxi = qn < end ? colind[qn] : 0;
                    if (HASV) nxv = qn < end ? vals[qn] : 0.0;
                }
                spd2 g[16];
                spmm_gather16<0>(g, myi, left, B, ldb, c, cv);
                spmm_acc16<HASV, 0>(g, myv, left, a0, a1);
                myi = nxi; myv = nxv;
            }
            acc[k * 256] = spd2{a0, a1};
        }
    }
    for (int k = 0; k < KB; k++) {
        const int64_t r = row_of(k);
        if (r >= 0 && cv) {
            const spd2 av = acc[k * 256];
            *(spd2 *)(Y + r * ldy + c) = av;
            if (Y2) *(spd2 *)(Y2 + r * ldy + c) = spd2{av[0] + bias[c], av[1] + bias[c + 1]};
        }
    }
}

// out[i*ncol + c] = in[i*irs + c*ics]  (32 x 32 tiles through LDS: coalesced on both sides for a column-major `in`)
__global__ __launch_bounds__(256) void k_to_rowmajor(int64_t n, int ncol, const double *__restrict__ in, int64_t irs, int64_t ics,
                                                     double *__restrict__ out, const int *skip)
{
    __shared__ double t[32][33];
    if (skip && *skip == 0) return;
    const int64_t i0 = (int64_t)blockIdx.x * 32;
    const int c0 = blockIdx.y * 32, a = threadIdx.x % 32;
    for (int b = threadIdx.x / 32; b < 32; b += 8) {
        const int64_t i = i0 + a;
        const int c = c0 + b;
        t[b][a] = (i < n && c < ncol) ? in[i * irs + c * ics] : 0.0;
    }
    __syncthreads();
    for (int b = threadIdx.x / 32; b < 32; b += 8) {
        const int64_t i = i0 + b;
        const int c = c0 + a;
        if (i < n && c < ncol) out[i * ncol + c] = t[a][b];
    }
}

// out[i*ors + c*ocs] = in[i*ncol + c]  (+ the biased copy out2)
__global__ __launch_bounds__(256) void k_from_rowmajor(int64_t n, int ncol, const double *__restrict__ in, double *__restrict__ out,
                                                       int64_t ors, int64_t ocs, const double *__restrict__ bias,
                                                       double *__restrict__ out2, const int *skip)
{
    __shared__ double t[32][33];
    if (skip && *skip == 0) return;
    const int64_t i0 = (int64_t)blockIdx.x * 32;
    const int c0 = blockIdx.y * 32, a = threadIdx.x % 32;
    for (int b = threadIdx.x / 32; b < 32; b += 8) {
        const int64_t i = i0 + b;
        const int c = c0 + a;
        t[b][a] = (i < n && c < ncol) ? in[i * ncol + c] : 0.0;
    }
    __syncthreads();
    for (int b = threadIdx.x / 32; b < 32; b += 8) {
        const int64_t i = i0 + a;
        const int c = c0 + b;
        if (i < n && c < ncol) {
            const double v = t[a][b];
            out[i * ors + c * ocs] = v;
            if (out2) out2[i * ors + c * ocs] = v + bias[c];
        }
    }
}

// ---- elementwise helpers -------------------------------------------------------------------------------------
__global__ void k_axpy_lambda(int64_t n, double lambda, const double *x, double *y)   // y += lambda x
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = fma(lambda, x[i], y[i]);
}

}  // namespace

// the transposes' launches, for spmm below and for the row-major solve of k_feat_cg.hip (a kernel lives in one unit)
void feat_to_rowmajor(bdf_ctx *ctx, int64_t n, int ncol, const double *in, int64_t irs, int64_t ics, double *out, const int *skip)
{
    hipLaunchKernelGGL(k_to_rowmajor, dim3((unsigned)((n + 31) / 32), (unsigned)((ncol + 31) / 32)), dim3(256), 0, ctx->stream, n, ncol, in,
                       irs, ics, out, skip);
}

void feat_from_rowmajor(bdf_ctx *ctx, int64_t n, int ncol, const double *in, double *out, int64_t ors, int64_t ocs,
                        const double *bias, double *out2, const int *skip)
{
    hipLaunchKernelGGL(k_from_rowmajor, dim3((unsigned)((n + 31) / 32), (unsigned)((ncol + 31) / 32)), dim3(256), 0, ctx->stream, n, ncol, in,
                       out, ors, ocs, bias, out2, skip);
}

static int spmm(bdf_ctx *ctx, const SpmmArgs &s)
{
    if (s.m == 0 || s.ncol == 0) return BDF_OK;
    const bool b_rm = s.bcs == 1 || s.ncol == 1, y_rm = s.ycs == 1 || s.ncol == 1;
    const double *B = s.B;
    int64_t ldb = s.brs;
    double *Y = s.Y;
    int64_t ldy = s.yrs;
    if (!b_rm || !y_rm) {
        void *sc;
        int rc = bdf_scratch2(ctx, (size_t)((b_rm ? 0 : s.kin) + (y_rm ? 0 : s.m)) * s.ncol * sizeof(double), &sc);
        if (rc) return rc;
        double *tb = (double *)sc, *ty = (double *)sc + (b_rm ? 0 : s.kin * s.ncol);
        if (!b_rm) {
            if (s.kin > 0) feat_to_rowmajor(ctx, s.kin, s.ncol, s.B, s.brs, s.bcs, tb, ctx->skip_flag);
            B = tb; ldb = s.ncol;
        }
        if (!y_rm) { Y = ty; ldy = s.ncol; }
    }
    // up to 32 columns in pairs, rows 16-byte aligned: sixteen lanes per row, sixteen gathers of 16 bytes in flight per lane
    const bool wide = s.ncol >= 2 && s.ncol <= 32 && s.ncol % 2 == 0 && ldb % 2 == 0 && ldy % 2 == 0 && ((uintptr_t)B & 15) == 0 &&
                      ((uintptr_t)Y & 15) == 0 && (!(y_rm && s.Y2) || (((uintptr_t)s.Y2 & 15) == 0));
    if (wide) {
        // a gathered operand of several L2 sizes is taken by COLUMN PANEL (3 MiB: every XCD's L2 holds the panel its workgroups
        // gather from, 23 TB/s of 16-byte lanes instead of the Infinity Cache's 8.6), all panels in ONE launch of a persistent grid
        // (k_spmm_rm16p).  Measured on configuration C5 against a launch per panel (profiles/r06_c5_fused_panels.txt, rocprofv3; that
        // path was retired after a70b66d): F p -- 6,250 row blocks, 5 panels -- 5 x 23.7 = 118 us panel by panel, 117 fused; F't --
        // 3,125 row blocks, 9 panels, every panel launch 2.4 generations of workgroups ending on a half-empty chip -- 9 x 15.8 =
        // 142 us against 125-130 fused: 241 us per F'(F p) instead of 260, 1.28 GB of gathered rows per product at 10-11 TB/s
        // (between the Infinity Cache's 8.6 and an L2-resident table's 23: the workgroups drift out of step by a panel or two).
        const int np = (s.panel_ptr && s.n_panels >= 2 && s.n_panels <= 64 && (size_t)s.kin * s.ncol * sizeof(double) >= ((size_t)8 << 20))
                           ? s.n_panels : 1;
        const double *bias = y_rm ? s.bias : nullptr;
        double *Y2 = y_rm ? s.Y2 : nullptr;
        if (np > 1) {
            // a persistent grid of as many workgroups as the stream's CUs hold, every one with KB row blocks' running sums in LDS
            // (4 KB each): the smallest KB whose grid is resident at once
            const int avail = ctx->on_reserved ? std::max(1, ctx->reserve_cus) : std::max(1, ctx->n_cus - ctx->reserve_cus);
            const int64_t nblocks = (s.m + 15) / 16;
            for (int64_t rb0 = 0; rb0 < nblocks;) {
                const int64_t left = nblocks - rb0;
                int kb = 1;
                int64_t G = 1;
                for (;; kb++) {
                    int occ = 0;
                    if (s.vals) BDF_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_spmm_rm16p<true>, 256, (size_t)kb * 4096));
                    else BDF_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_spmm_rm16p<false>, 256, (size_t)kb * 4096));
                    G = (int64_t)avail * std::max(1, occ);
                    if (G * kb >= left || kb == 12) break;
                }
                const dim3 pg((unsigned)std::min<int64_t>(G, (left + kb - 1) / kb));
                if (s.vals) hipLaunchKernelGGL(k_spmm_rm16p<true>, pg, dim3(256), (size_t)kb * 4096, ctx->stream, s.m, s.ncol, s.colind, s.vals, B, ldb, Y, ldy,
                                               bias, Y2, ctx->skip_flag, s.panel_ptr, np, kb, rb0, nblocks);
                else hipLaunchKernelGGL(k_spmm_rm16p<false>, pg, dim3(256), (size_t)kb * 4096, ctx->stream, s.m, s.ncol, s.colind, s.vals, B, ldb, Y, ldy,
                                        bias, Y2, ctx->skip_flag, s.panel_ptr, np, kb, rb0, nblocks);
                rb0 += (int64_t)pg.x * kb;
            }
        } else {
            const dim3 grid((unsigned)((s.m + 15) / 16));
            if (s.vals) hipLaunchKernelGGL(k_spmm_rm16<true>, grid, dim3(256), 0, ctx->stream, s.m, s.ncol, s.rowptr, s.colind, s.vals, B, ldb, Y, ldy,
                                           bias, Y2, ctx->skip_flag);
            else hipLaunchKernelGGL(k_spmm_rm16<false>, grid, dim3(256), 0, ctx->stream, s.m, s.ncol, s.rowptr, s.colind, s.vals, B, ldb, Y, ldy,
                                    bias, Y2, ctx->skip_flag);
        }
    } else
    hipLaunchKernelGGL(k_spmm_rm, dim3((unsigned)((s.m + 7) / 8)), dim3(256), 0, ctx->stream, s.m, s.ncol, s.rowptr, s.colind, s.vals,
                       B, ldb, Y, ldy, y_rm ? s.bias : nullptr, y_rm ? s.Y2 : nullptr, ctx->skip_flag);
    if (!y_rm) feat_from_rowmajor(ctx, s.m, s.ncol, Y, s.Y, s.yrs, s.ycs, s.bias, s.Y2, ctx->skip_flag);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}

// Y = op(F) B for any feature kind.  B(i,c) at B[i*brs + c*bcs], Y(r,c) at Y[r*yrs + c*ycs].
int feat_apply(bdf_ctx *ctx, const bdf_feat *f, bool transpose, const double *B, int64_t brs, int64_t bcs, int ncol,
               double *Y, int64_t yrs, int64_t ycs, const double *bias, double *Y2)
{
    if (f->kind == 0 && ncol <= 64 && f->m > 0 && f->n > 0) return dense_apply(ctx, f, transpose, B, brs, bcs, ncol, Y, yrs, ycs, bias, Y2);
    if (f->kind == 0) {
        GemmArgs g;
        g.M = transpose ? f->n : f->m; g.N = ncol; g.K = transpose ? f->m : f->n;
        g.A = f->dense_dev;
        g.ars = transpose ? f->m : 1; g.acs = transpose ? 1 : f->m;
        g.B = B; g.brs = brs; g.bcs = bcs; g.C = Y; g.crs = yrs; g.ccs = ycs; g.bias = bias; g.C2 = Y2;
        return feat_gemm(ctx, g);
    }
    SpmmArgs s;
    s.m = transpose ? f->n : f->m; s.kin = transpose ? f->m : f->n; s.ncol = ncol;
    s.rowptr = transpose ? f->colptr_dev : f->rowptr_dev;
    s.colind = transpose ? f->rowind_dev : f->colind_dev;
    s.vals = f->kind == 1 ? (transpose ? f->cvals_dev : f->rvals_dev) : nullptr;
    s.B = B; s.brs = brs; s.bcs = bcs; s.Y = Y; s.yrs = yrs; s.ycs = ycs; s.bias = bias; s.Y2 = Y2;
    s.panel_ptr = transpose ? f->panel_tr_dev : f->panel_fwd_dev; s.n_panels = transpose ? f->n_panels_tr : f->n_panels_fwd;
    return spmm(ctx, s);
}

static int ensure_dense(bdf_feat *f)
{
    if (f->dense_dev) return BDF_OK;
    bdf_ctx *ctx = f->ctx;
    BDF_REQUIRE((double)f->m * (double)f->n * 8.0 <= 4e9, BDF_ERR_ARG,
                "FF path needs F'F of a sparse F with %lld x %lld entries: too large, use the CG path (compute_ff_size)",
                (long long)f->m, (long long)f->n);
    // densify by applying F to the identity: dense(:, j) = F e_j
    size_t nn = (size_t)f->n * (size_t)f->n;
    DevBuf<double> eye, dense;
    int rc;
    if ((rc = eye.alloc_bytes(std::max<size_t>(nn * sizeof(double), 8)))) return rc;
    std::vector<double> h(nn, 0.0);
    for (int64_t j = 0; j < f->n; j++) h[(size_t)j * f->n + j] = 1.0;
    BDF_HIP(hipMemcpy(eye, h.data(), nn * sizeof(double), hipMemcpyHostToDevice));
    if ((rc = dense.alloc_bytes(std::max<size_t>((size_t)f->m * f->n * sizeof(double), 8)))) return rc;
    if ((rc = feat_apply(ctx, f, false, eye, 1, f->n, (int)f->n, dense, 1, f->m))) return rc;
    BDF_HIP(hipStreamSynchronize(ctx->stream));
    f->dense_dev = std::move(dense);
    return BDF_OK;
}

int feat_ensure_FF(bdf_feat *f)
{
    if (f->FF_dev) return BDF_OK;
    bdf_ctx *ctx = f->ctx;
    int rc = ensure_dense(f);
    if (rc) return rc;
    if ((rc = f->FF_dev.alloc_bytes(std::max<size_t>((size_t)f->n * f->n * sizeof(double), 8)))) return rc;
    GemmArgs g;                          // FF = full(At_mul_B(F, F)), RelationData.jl:338
    g.M = f->n; g.N = f->n; g.K = f->m;
    g.A = f->dense_dev; g.ars = f->m; g.acs = 1;
    g.B = f->dense_dev; g.brs = 1; g.bcs = f->m;
    g.C = f->FF_dev; g.crs = 1; g.ccs = f->n; g.bias = nullptr; g.C2 = nullptr;
    return feat_gemm(ctx, g);
}

static int create_sparse(bdf_ctx *ctx, int64_t m, int64_t n, int64_t nnz, const int32_t *rows, const int32_t *cols,
                         const double *vals, bdf_feat **out)
{
    BDF_REQUIRE(ctx && out, BDF_ERR_ARG, "bdf_feat_create: NULL argument");
    BDF_REQUIRE(m >= 0 && n >= 0 && nnz >= 0 && (nnz == 0 || (rows && cols)), BDF_ERR_ARG, "bdf_feat_create: bad argument");
    for (int64_t q = 0; q < nnz; q++) {
        BDF_REQUIRE(rows[q] >= 1 && rows[q] <= m && cols[q] >= 1 && cols[q] <= n, BDF_ERR_BOUNDS,
                    "bdf_feat_create: entry %lld (%d,%d) outside %lld x %lld", (long long)q, rows[q], cols[q], (long long)m, (long long)n);
    }
    BDF_HIP(hipSetDevice(ctx->device));
    auto build = [&](const int32_t *major, const int32_t *minor, int64_t nmajor, std::vector<int64_t> &ptr,
                     std::vector<int32_t> &ind, std::vector<double> &v) {
        ptr.assign((size_t)nmajor + 1, 0);
        for (int64_t q = 0; q < nnz; q++) ptr[(size_t)major[q]]++;
        for (int64_t j = 0; j < nmajor; j++) ptr[(size_t)j + 1] += ptr[(size_t)j];
        std::vector<int64_t> cur(ptr.begin(), ptr.end() - 1);
        ind.assign((size_t)nnz, 0);
        if (vals) v.assign((size_t)nnz, 0.0);
        for (int64_t q = 0; q < nnz; q++) {          // stable in input order (sortperm, sparsebin_csr.jl:23)
            int64_t dst = cur[(size_t)major[q] - 1]++;
            ind[(size_t)dst] = minor[q] - 1;
            if (vals) v[(size_t)dst] = vals[q];
        }
    };
    std::unique_ptr<bdf_feat> f(new bdf_feat());       // error paths free what was uploaded
    f->ctx = ctx; f->kind = vals ? 1 : 2; f->m = m; f->n = n; f->nnz = nnz;
    std::vector<int64_t> ptr; std::vector<int32_t> ind; std::vector<double> v;
    int rc;
    // column panels (spmm): where each row's entries cross a multiple of BDF_SPMM_PANEL_ROWS columns -- only when every row's entries
    // are in column order (the panels must keep the order of the row's sum) and the operand is large enough to be worth it
    auto panels = [&](int64_t nmajor, int64_t nminor, DevBuf<int64_t> &dev, int *np_out) -> int {
        const int64_t P = (nminor + BDF_SPMM_PANEL_ROWS - 1) / BDF_SPMM_PANEL_ROWS;
        *np_out = 0;
        if (P < 2 || P > 64 || (size_t)(P + 1) * nmajor * sizeof(int64_t) > ((size_t)256 << 20)) return BDF_OK;
        std::vector<int64_t> pp((size_t)(P + 1) * nmajor);
        for (int64_t r = 0; r < nmajor; r++) {
            int64_t q = ptr[(size_t)r];
            const int64_t e = ptr[(size_t)r + 1];
            for (int64_t k = q + 1; k < e; k++)
                if (ind[(size_t)k] < ind[(size_t)k - 1]) return BDF_OK;           // not in column order: one pass
            for (int64_t p = 0; p <= P; p++) {
                while (q < e && ind[(size_t)q] < p * BDF_SPMM_PANEL_ROWS) q++;
                pp[(size_t)p * nmajor + r] = (p == P) ? e : q;
            }
        }
        int rc2 = dev.upload(pp);
        if (!rc2) *np_out = (int)P;
        return rc2;
    };
    build(rows, cols, m, ptr, ind, v);
    if ((rc = f->rowptr_dev.upload(ptr)) || (rc = f->colind_dev.upload(ind))) return rc;
    if (vals && (rc = f->rvals_dev.upload(v))) return rc;
    if ((rc = panels(m, n, f->panel_fwd_dev, &f->n_panels_fwd))) return rc;
    build(cols, rows, n, ptr, ind, v);
    if ((rc = f->colptr_dev.upload(ptr)) || (rc = f->rowind_dev.upload(ind))) return rc;
    if (vals && (rc = f->cvals_dev.upload(v))) return rc;
    if ((rc = panels(n, m, f->panel_tr_dev, &f->n_panels_tr))) return rc;
    *out = f.release();
    return BDF_OK;
}

extern "C" int bdf_feat_create_dense(bdf_ctx *ctx, int64_t m, int64_t n, const double *F, bdf_feat **out)
{
    BDF_REQUIRE(ctx && out && m >= 0 && n >= 0 && (m * n == 0 || F), BDF_ERR_ARG, "bdf_feat_create_dense: bad argument");
    BDF_HIP(hipSetDevice(ctx->device));
    std::unique_ptr<bdf_feat> f(new bdf_feat());
    f->ctx = ctx; f->kind = 0; f->m = m; f->n = n; f->nnz = m * n;
    if (int rc = f->dense_dev.alloc_bytes(std::max<size_t>((size_t)m * n * sizeof(double), 8))) return rc;
    if (m * n) BDF_HIP(hipMemcpy(f->dense_dev, F, (size_t)m * n * sizeof(double), hipMemcpyHostToDevice));
    *out = f.release();
    return BDF_OK;
}

extern "C" int bdf_feat_create_csr(bdf_ctx *ctx, int64_t m, int64_t n, int64_t nnz, const int32_t *rows,
                                   const int32_t *cols, const double *vals, bdf_feat **out)
{
    BDF_REQUIRE(nnz == 0 || vals, BDF_ERR_ARG, "bdf_feat_create_csr: vals is NULL");
    static const double one = 1.0;
    return create_sparse(ctx, m, n, nnz, rows, cols, nnz ? vals : &one, out);
}

extern "C" int bdf_feat_create_bin(bdf_ctx *ctx, int64_t m, int64_t n, int64_t nnz, const int32_t *rows,
                                   const int32_t *cols, bdf_feat **out)
{
    return create_sparse(ctx, m, n, nnz, rows, cols, nullptr, out);
}

bdf_feat::~bdf_feat()
{
    if (!ctx) return;
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
}

extern "C" int bdf_feat_destroy(bdf_feat *f)
{
    if (f) delete f;
    return BDF_OK;
}

extern "C" int bdf_feat_set_row_ids(bdf_feat *f, const int32_t *row_ids_host)
{
    BDF_REQUIRE(f, BDF_ERR_ARG, "bdf_feat_set_row_ids: NULL argument");
    f->row_ids_dev.reset();
    if (row_ids_host && f->m > 0) {
        if (int rc = f->row_ids_dev.alloc((size_t)f->m)) return rc;
        BDF_HIP(hipMemcpy(f->row_ids_dev, row_ids_host, (size_t)f->m * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    return BDF_OK;
}

extern "C" int bdf_feat_size(const bdf_feat *f, int64_t *m, int64_t *n, int64_t *nnz)
{
    BDF_REQUIRE(f && m && n && nnz, BDF_ERR_ARG, "bdf_feat_size: NULL argument");
    *m = f->m; *n = f->n; *nnz = f->nnz;
    return BDF_OK;
}

extern "C" int bdf_feat_mul(bdf_ctx *ctx, const bdf_feat *f, const double *B, int ncol, double *out, int transpose)
{
    BDF_REQUIRE(ctx && f && B && out && ncol >= 1, BDF_ERR_ARG, "bdf_feat_mul: bad argument");
    const int64_t kin = transpose ? f->m : f->n, kout = transpose ? f->n : f->m;
    return feat_apply(ctx, f, transpose != 0, B, 1, kin, ncol, out, 1, kout);
}

extern "C" int bdf_feat_AtA_mul(bdf_ctx *ctx, const bdf_feat *f, const double *X, int ncol, double lambda, double *out)
{
    BDF_REQUIRE(ctx && f && X && out && ncol >= 1, BDF_ERR_ARG, "bdf_feat_AtA_mul: bad argument");
    void *tmp;
    int rc = bdf_scratch(ctx, (size_t)f->m * ncol * sizeof(double), &tmp);
    if (rc) return rc;
    if ((rc = feat_apply(ctx, f, false, X, 1, f->n, ncol, (double *)tmp, 1, f->m))) return rc;
    if ((rc = feat_apply(ctx, f, true, (const double *)tmp, 1, f->m, ncol, out, 1, f->n))) return rc;
    const int64_t tot = f->n * ncol;
    hipLaunchKernelGGL(k_axpy_lambda, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, ctx->stream, tot, lambda, X, out);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}

extern "C" int bdf_uhat(bdf_ctx *ctx, const bdf_feat *f, int D, const double *beta, const double *mu,
                        double *uhat_out, double *mu_matrix_out)
{
    BDF_REQUIRE(ctx && f && beta && uhat_out, BDF_ERR_ARG, "bdf_uhat: NULL argument");
    BDF_REQUIRE(D >= 1 && D <= BDF_MAX_D, BDF_ERR_ARG, "bdf_uhat: num_latent=%d must be in 1..%d", D, BDF_MAX_D);
    BDF_REQUIRE(!mu_matrix_out || mu, BDF_ERR_ARG, "bdf_uhat: mu is NULL");
    // (F beta)(i,d) written at uhat[d + i*D]
    return feat_apply(ctx, f, false, beta, 1, f->n, D, uhat_out, D, 1, mu, mu_matrix_out);
}
