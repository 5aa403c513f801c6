// k_vb.hip -- variational BPMF (src/macau_vb.jl:103-140): the row update update_u! and the prior update update_prior!.
//
// Row update (one launch per half-iteration, all rows of the entity).  A workgroup of four waves takes G = 64 / DP rows
// (DP = 16, 32, 64 is the padded dimension) of the degree-descending order:
//   1. gather: the four waves deal the row's neighbours among them (neighbour q to wave q mod 4) and sum their records
//      (packed Euu_v and, weighted by the centred value rr_v, mu_v) in registers -- every lane owns two consecutive doubles
//      of every 128-double stretch of a record, so that one neighbour is read as whole lines, U neighbours in flight;
//   2. the four waves' sums are added in LDS in wave order (fixed: the result does not depend on timing);
//   3. wave 0 unpacks them into the column-per-lane layout of wave_linalg.h (lane (g, c) holds column c of row g's
//      matrix), adds A = nu_N W_N, and inverts L by the symmetric sweep (Gauss-Jordan without pivoting, stable for SPD):
//      Euu_u needs the explicit inverse, Euu_u = inv(L) + mu mu';
//   4. the new records go through LDS and are written as whole lines, with the block's partial sums for update_prior!.
// Prior update: the partial sums are reduced in a fixed order (VB_SLICES slices, then the slices) and one wave forms and
// inverts the D x D matrix of update_prior!.  No floating-point atomics anywhere: every run gives the same bits.
#include "vb.h"
#include "wave_linalg.h"

namespace {

template <int DP>
struct VBL {
    static constexpr int G = 64 / DP;                      // rows per workgroup (= matrices per wave in the inversion)
    static constexpr int RSMAX = (DP * (DP + 1) / 2 + DP + 15) / 16 * 16;
    static constexpr int NL = (RSMAX + 127) / 128;         // double2 loads per lane and neighbour
    static constexpr int U = DP == 64 ? 2 : 4;             // neighbours in flight per wave
};

// In: col[i] = L[i][c] (lane c of its group; the padding is the identity).  Out: col[i] = -inv(L)[i][c].
// Step k sweeps pivot k: every lane publishes its col[k] (= row k, entry c, by symmetry) to bc, reads the row back and
// updates its column with one fma per element; the pivot's own column becomes the scaled row, its pivot -1/d.
// The step number is a run-time value (the DP steps are not unrolled): col[k] is picked and replaced by selects over the
// unrolled element loop, so that the column stays in registers.
// Returns true if a pivot was not positive (L not positive definite).
template <int DP>
__device__ __forceinline__ bool vb_sweep(double (&col)[DP], double *bc, int c)
{
    bool notpd = false;
#pragma nounroll
    for (int k = 0; k < DP; k++) {
        double ck = 0.0;
#pragma unroll
        for (int i = 0; i < DP; i++) ck = (i == k) ? col[i] : ck;
        wave_sync();
        bc[c] = ck;
        wave_sync();
        const double d = bc[k];
        if (!(d > 0.0)) notpd = true;
        const double rd = 1.0 / d;
        const bool own = c == k;
        const double f = ck * rd;
        const double nk = own ? -rd : f;
        // chunks of 8 broadcast values at a time (a compiler-only barrier keeps the reads from all being hoisted)
#pragma unroll
        for (int i0 = 0; i0 < DP; i0 += 8) {
            double r[8];
#pragma unroll
            for (int u = 0; u < 8; u++) r[u] = (i0 + u < DP) ? bc[i0 + u] : 0.0;
            asm volatile("" ::: "memory");
#pragma unroll
            for (int u = 0; u < 8; u++)
                if (i0 + u < DP) {
                    const double x = own ? r[u] * rd : fma(-r[u], f, col[i0 + u]);
                    col[i0 + u] = (i0 + u == k) ? nk : x;
                }
        }
    }
    wave_sync();
    return notpd;
}

template <int DP>
__global__ __launch_bounds__(256) void k_vb_rows(VBRowArgs a)
{
    using L = VBL<DP>;
    constexpr int G = L::G, NL = L::NL, U = L::U, RSM = L::RSMAX;
    __shared__ double buf[G][RSM];         // the rows' summed records, then their new records
    __shared__ double bc[G][DP];           // the sweep's broadcast row
    __shared__ double vec[G][DP];          // right-hand side, then mu
    __shared__ double nrm;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t s0 = (int64_t)blockIdx.x * G;

    // ---- 1. gather
    double2 acc[G][NL];
#pragma unroll
    for (int g = 0; g < G; g++)
#pragma unroll
        for (int j = 0; j < NL; j++) acc[g][j] = double2{0.0, 0.0};
#pragma unroll
    for (int g = 0; g < G; g++) {
        if (s0 + g >= a.N) break;                          // block-uniform
        const int32_t row = a.order[s0 + g];
        const int64_t q0 = a.rowptr[row], q1 = a.rowptr[row + 1];
        for (int64_t q = q0 + wave; q < q1; q += 4 * U) {
            const double *src[U];
            double rr[U];
            bool ok[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int64_t qq = q + 4 * u;
                ok[u] = qq < q1;
                const int32_t nb = ok[u] ? a.colidx[qq] : 0;
                rr[u] = ok[u] ? a.vals[qq] : 0.0;
                src[u] = a.rec_other + (int64_t)nb * a.RS;
            }
            double2 x[U][NL];
#pragma unroll
            for (int u = 0; u < U; u++)
#pragma unroll
                for (int j = 0; j < NL; j++) {
                    const int t = 2 * lane + 128 * j;
                    x[u][j] = (ok[u] && t < a.RS) ? *(const double2 *)(src[u] + t) : double2{0.0, 0.0};
                }
#pragma unroll
            for (int u = 0; u < U; u++)
#pragma unroll
                for (int j = 0; j < NL; j++) {
                    const int t = 2 * lane + 128 * j;
                    // Euu entries are summed as they are, mu entries weighted by the value (the padding is zero)
                    acc[g][j].x = fma(t < a.T ? 1.0 : rr[u], x[u][j].x, acc[g][j].x);
                    acc[g][j].y = fma(t + 1 < a.T ? 1.0 : rr[u], x[u][j].y, acc[g][j].y);
                }
        }
    }

    // ---- 2. the waves' sums, added in wave order
#pragma unroll
    for (int w = 0; w < 4; w++) {
        if (wave == w) {
#pragma unroll
            for (int g = 0; g < G; g++)
#pragma unroll
                for (int j = 0; j < NL; j++) {
                    const int t = 2 * lane + 128 * j;
                    if (t < a.RS) {
                        if (w == 0) { buf[g][t] = acc[g][j].x; buf[g][t + 1] = acc[g][j].y; }
                        else { buf[g][t] += acc[g][j].x; buf[g][t + 1] += acc[g][j].y; }
                    }
                }
        }
        __syncthreads();
    }

    // ---- 3. L = A + alpha sum Euu_v, inv(L), mu = inv(L) (b + alpha sum rr_v mu_v), Euu_u = inv(L) + mu mu'
    if (wave == 0) {
        const int g = lane / DP, c = lane % DP;
        const bool live = s0 + g < a.N;
        const int D = a.D;
        const double *S = buf[g];
        double col[DP];
#pragma unroll
        for (int i = 0; i < DP; i++) {
            double v = (i == c) ? 1.0 : 0.0;
            if (live && i < D && c < D) {
                const int pi = i <= c ? c * (c + 1) / 2 + i : i * (i + 1) / 2 + c;
                v = a.pack[c * D + i] + a.alpha * S[pi];
            }
            col[i] = v;
        }
        vec[g][c] = (live && c < D) ? a.pack[D * D + c] + a.alpha * S[a.T + c] : 0.0;
        const bool notpd = vb_sweep<DP>(col, bc[g], c);
        if (live && notpd && c == 0) atomicOr_system(a.flag, 1);
        double m = 0.0;
#pragma unroll
        for (int i = 0; i < DP; i++) m = fma(-col[i], vec[g][i], m);
        wave_sync();
        vec[g][c] = m;
        wave_sync();
        if (live && c < D) {
            double *E = buf[g] + c * (c + 1) / 2;
#pragma unroll
            for (int i = 0; i < DP; i++)
                if (i <= c) E[i] = -col[i] + vec[g][i] * m;
            buf[g][a.T + c] = m;
        }
        double sq = (live && c < D) ? m * m : 0.0;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) sq += __shfl_xor(sq, off);
        if (lane == 0) nrm = sq;
    }
    __syncthreads();

    // ---- 4. new records (whole lines), means, and the block's partial sums for update_prior!
    int32_t rows[G];
#pragma unroll
    for (int g = 0; g < G; g++) rows[g] = (s0 + g < a.N) ? a.order[s0 + g] : -1;
    double *part = a.partial + (int64_t)blockIdx.x * a.PW;
    for (int t = tid; t < a.RS; t += 256) {
        double s = 0.0;
#pragma unroll
        for (int g = 0; g < G; g++)
            if (rows[g] >= 0) {
                const double v = buf[g][t];
                a.rec_out[(int64_t)rows[g] * a.RS + t] = v;
                s += v;
            }
        if (t < a.PW - 1) part[t] = s;
    }
    if (tid == 0) part[a.PW - 1] = nrm;
    for (int e = tid; e < G * a.D; e += 256) {
        const int g = e / a.D, c = e % a.D;
        if (s0 + g < a.N) a.mu_out[(int64_t)a.order[s0 + g] * a.D + c] = buf[g][a.T + c];
    }
}

// partial sums of the blocks [s nblocks / VB_SLICES, (s + 1) nblocks / VB_SLICES) -> slice s, in block order
__global__ __launch_bounds__(256) void k_vb_prior_reduce(VBPriorArgs a)
{
    const int e = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
    if (e >= a.PW) return;
    const int64_t b0 = a.nblocks * s / VB_SLICES, b1 = a.nblocks * (s + 1) / VB_SLICES;
    double v = 0.0;
    for (int64_t b = b0; b < b1; b++) v += a.partial[b * a.PW + e];
    a.slices[(int64_t)s * a.PW + e] = v;
}

// update_prior! (macau_vb.jl:132-140) and the next row update's A = nu_N W_N, b = A mu_N (:104-105)
template <int DP>
__global__ __launch_bounds__(256) void k_vb_prior(VBPriorArgs a)
{
    __shared__ double tot[DP * (DP + 1) / 2 + DP + 1];
    __shared__ double bc[DP], mun[DP];
    const int tid = threadIdx.x, D = a.D;
    for (int e = tid; e < a.PW; e += 256) {
        double v = 0.0;
        for (int s = 0; s < VB_SLICES; s++) v += a.slices[(int64_t)s * a.PW + e];
        tot[e] = v;
    }
    __syncthreads();
    if (tid < DP) mun[tid] = tid < D ? (a.b_0 * a.mu0[tid] + tot[a.T + tid]) / a.b_N : 0.0;
    __syncthreads();
    if (tid < DP) {
        const int c = tid;
        double col[DP];
#pragma unroll
        for (int i = 0; i < DP; i++) {
            double v = (i == c) ? 1.0 : 0.0;
            if (i < D && c < D) {
                const int pi = i <= c ? c * (c + 1) / 2 + i : i * (i + 1) / 2 + c;
                v = ((a.Winv0[c * D + i] + tot[pi]) + (a.b_0 * a.mu0[i]) * a.mu0[c]) - (a.b_N * mun[i]) * mun[c];
            }
            col[i] = v;
        }
        const bool notpd = vb_sweep<DP>(col, bc, c);
        if (notpd && c == 0) atomicOr_system(a.flag, 2);
        if (c < D) {
            double b = 0.0;
#pragma unroll
            for (int i = 0; i < DP; i++) {
                if (i < D) {
                    const double w = -col[i];
                    const double A = w * a.nu_N;
                    a.W_N[c * D + i] = w;
                    a.pack[c * D + i] = A;
                    b = fma(A, mun[i], b);
                }
            }
            a.pack[D * D + c] = b;
            a.mu_N[c] = mun[c];
        }
        if (c == 0) *a.normsq = tot[a.T + D];
    }
}

template <int DP>
int launch_rows(hipStream_t s, const VBRowArgs &a)
{
    const int64_t nb = (a.N + VBL<DP>::G - 1) / VBL<DP>::G;
    hipLaunchKernelGGL(k_vb_rows<DP>, dim3((unsigned)nb), dim3(256), 0, s, a);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}

}  // namespace

int vb_row_blocks(int D, int64_t N)
{
    const int G = D <= 16 ? 4 : (D <= 32 ? 2 : 1);
    return (int)((N + G - 1) / G);
}

int vb_launch_rows(hipStream_t s, const VBRowArgs &a)
{
    if (a.N == 0) return BDF_OK;
    if (a.D <= 16) return launch_rows<16>(s, a);
    if (a.D <= 32) return launch_rows<32>(s, a);
    return launch_rows<64>(s, a);
}

int vb_launch_prior(hipStream_t s, const VBPriorArgs &a)
{
    hipLaunchKernelGGL(k_vb_prior_reduce, dim3((unsigned)((a.PW + 255) / 256), VB_SLICES), dim3(256), 0, s, a);
    if (a.D <= 16) hipLaunchKernelGGL(k_vb_prior<16>, dim3(1), dim3(256), 0, s, a);
    else if (a.D <= 32) hipLaunchKernelGGL(k_vb_prior<32>, dim3(1), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_vb_prior<64>, dim3(1), dim3(256), 0, s, a);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}
