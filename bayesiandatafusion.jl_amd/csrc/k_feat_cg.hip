// k_feat_cg.hip -- K4: the batched conjugate-gradient solve of the beta update.
//   beta = (F'F + lb I) \ rhs                          solve_full :314-320 | solve_cg2 parallel_matrix.jl:488-507
//   all D conjugate-gradient solves advance together, each column keeping the reference's own stopping rule
//   (cg_AtA, src/parallel_cg.jl:63-94: stop when ||r|| < tol ||b||, checked before an iteration; maxiter).
#include "feat.h"
#include <algorithm>
#include <cmath>

namespace {

// ---- batched CG --------------------------------------------------------------------------------------------------
struct CgState {
    int64_t n; int D;
    double *X, *R, *P, *Z;               // n x D column-major
    double *bknum, *bkden, *tolb;        // D
    int *active, *iters, *nactive;
    int *done_blocks;                    // columns (workgroups) that have finished the current step
    volatile uint64_t *status;           // host-mapped: [0] = generation << 32 | last completed iteration, [1] = active columns
    uint32_t gen;
    int *flag;                           // BDF_WARN_CG_MAXITER: a column still active after the last iteration
};

__device__ __forceinline__ double block_sum(double v, double *red)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < (int)(blockDim.x >> 6); w++) s += red[w];
    return s;
}

// The CG kernels take one workgroup per column (no grid-wide reduction); long columns get 1024 threads (CG_THREADS_LONG)
// (bar, nullable: the hand-over counter of k_cg_resident, zeroed here)
__global__ __launch_bounds__(1024) void k_cg_init(CgState s, const double *rhs, double tol, unsigned *bar)
{
    __shared__ double red[16];
    const int d = blockIdx.x;
    const int64_t off = (int64_t)d * s.n;
    double nb = 0.0;
    for (int64_t i = threadIdx.x; i < s.n; i += blockDim.x) {
        const double b = rhs[off + i];
        s.X[off + i] = 0.0; s.R[off + i] = b; s.P[off + i] = b;
        nb = fma(b, b, nb);
    }
    nb = block_sum(nb, red);
    if (threadIdx.x == 0) {
        s.tolb[d] = tol * sqrt(nb);      // tol = tol * norm(b), parallel_cg.jl:65
        s.bkden[d] = 0.0; s.active[d] = 1; s.iters[d] = 0;
        if (d == 0) { *s.nactive = s.D; *s.done_blocks = 0; if (bar) *bar = 0u; }
    }
}

// top of iteration `iter` (1-based): residual check, direction update (parallel_cg.jl:74-83)
__device__ __forceinline__ void cg_pre(const CgState &s, int iter, double *red, int &go)
{
    const int d = blockIdx.x;
    if (!s.active[d]) return;
    const int64_t off = (int64_t)d * s.n;
    double bknum = 0.0;
    for (int64_t i = threadIdx.x; i < s.n; i += blockDim.x) bknum = fma(s.R[off + i], s.R[off + i], bknum);
    bknum = block_sum(bknum, red);
    if (threadIdx.x == 0) {
        go = !(sqrt(bknum) < s.tolb[d]);
        if (!go) { s.active[d] = 0; atomicSub(s.nactive, 1); }
    }
    __syncthreads();
    if (!go) return;
    if (iter > 1) {
        const double bk = bknum / s.bkden[d];
        for (int64_t i = threadIdx.x; i < s.n; i += blockDim.x) s.P[off + i] = fma(bk, s.P[off + i], s.R[off + i]);
    }
    __syncthreads();
    if (threadIdx.x == 0) { s.bkden[d] = bknum; s.bknum[d] = bknum; s.iters[d] = iter; }
}

__global__ __launch_bounds__(1024) void k_cg_pre(CgState s, int iter)
{
    __shared__ double red[16];
    __shared__ int go;
    cg_pre(s, iter, red, go);
}

// The CG step -- bottom of iteration `iter` (z = Z + lambda p; ak = bknum / (z.p); x += ak p; r -= ak z, parallel_cg.jl:85-91) and
// top of iteration `iter + 1` in one launch, a column per workgroup -- for short columns (n <= 256 EPT): the column's p, z, x, r are
// read ONCE into registers, both halves of the step run on them, and what changed is written once -- a general step kernel that
// walked the column four times, each walk a global-memory round trip, took 8.6 us per iteration at n = 500, where the arithmetic is
// nothing (it was retired after a70b66d).  The dot products are summed thread-strided as in block_sum's callers.
template <int EPT>
__global__ __launch_bounds__(256) void k_cg_step_short(CgState s, const double *lambda_p, int iter, int maxiter)
{
    __shared__ double red[16];
    __shared__ int go;
    if (*s.nactive == 0) {
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            s.status[1] = 0;
            __threadfence_system();
            s.status[0] = ((uint64_t)s.gen << 32) | (uint32_t)iter;
        }
        return;
    }
    const int d = blockIdx.x, tid = threadIdx.x;
    const int64_t off = (int64_t)d * s.n;
    const bool mine = s.active[d] && s.iters[d] == iter;
    if (mine) {
        const double lambda = *lambda_p;
        double p[EPT], z[EPT], x[EPT], r[EPT];
#pragma unroll
        for (int e = 0; e < EPT; e++) {
            const int64_t i = tid + 256 * e;
            const bool ok = i < s.n;
            p[e] = ok ? s.P[off + i] : 0.0; z[e] = ok ? s.Z[off + i] : 0.0;
            x[e] = ok ? s.X[off + i] : 0.0; r[e] = ok ? s.R[off + i] : 0.0;
        }
        double zp = 0.0;
#pragma unroll
        for (int e = 0; e < EPT; e++) {
            z[e] = fma(lambda, p[e], z[e]);
            zp = fma(z[e], p[e], zp);
        }
        zp = block_sum(zp, red);
        const double ak = s.bknum[d] / zp;
        double bknum = 0.0;
#pragma unroll
        for (int e = 0; e < EPT; e++) {
            x[e] = fma(ak, p[e], x[e]);
            r[e] = fma(-ak, z[e], r[e]);
            bknum = fma(r[e], r[e], bknum);
        }
        bool proceed = false;
        if (iter >= maxiter && tid == 0) atomicOr_system(s.flag, (int)BDF_WARN_CG_MAXITER);
        if (iter < maxiter) {                              // top of iteration iter + 1 (cg_pre)
            bknum = block_sum(bknum, red);
            if (tid == 0) {
                go = !(sqrt(bknum) < s.tolb[d]);
                if (!go) { s.active[d] = 0; atomicSub(s.nactive, 1); }
            }
            __syncthreads();
            proceed = go != 0;
            if (proceed) {
                const double bk = bknum / s.bkden[d];
#pragma unroll
                for (int e = 0; e < EPT; e++) p[e] = fma(bk, p[e], r[e]);
            }
        }
#pragma unroll
        for (int e = 0; e < EPT; e++) {
            const int64_t i = tid + 256 * e;
            if (i < s.n) {
                s.X[off + i] = x[e]; s.R[off + i] = r[e];
                if (proceed) s.P[off + i] = p[e];
            }
        }
        __syncthreads();
        if (proceed && tid == 0) { s.bkden[d] = bknum; s.bknum[d] = bknum; s.iters[d] = iter + 1; }
    }
    __syncthreads();
    if (tid == 0) {
        __threadfence();
        if (atomicAdd(s.done_blocks, 1) == s.D - 1) {
            *s.done_blocks = 0;
            const int na = __hip_atomic_load(s.nactive, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s.status[1] = (uint64_t)(iter < maxiter ? na : 0);
            __threadfence_system();
            s.status[0] = ((uint64_t)s.gen << 32) | (uint32_t)iter;
        }
    }
}

// ---- the whole solve in ONE launch for a small resident operator (F'F of at most 512 features, at most 32 columns) -----------------
// An iteration of the batched solve is two dependent launches (product 10.4 us, step 7.2 us at numF = 500, D = 32), and both
// are the floor of a dependent launch of a few workgroups (~5 us) plus a little work: fifteen iterations are 0.26 of configuration
// C3's 0.54 ms.  Here ceil(numF / 16) workgroups stay resident for the whole solve.  Workgroup w is (a) the owner of the rows
// 16 w .. 16 w + 15 of the operator -- its waves keep their quarter of K of those rows in REGISTERS as matrix operands across all
// iterations -- and (b) the owner of column w of the solve: that column's p, x, r and scalars live in its registers.  An
// iteration: every workgroup multiplies its rows into all columns of P (read from memory past the caches) and writes its rows of Z
// write-through; a grid-wide hand-over; the column owners run EXACTLY k_cg_step_short's arithmetic on their column (same sums in
// the same order) and write the new p write-through; a second hand-over.  The hand-overs are a monotonic counter (arrive after
// the wave's write-through stores have completed, poll with agent-scope loads); nothing is fenced: what crosses workgroups is
// written with write-through stores and read with agent-scope loads.  All workgroups are co-resident (at most 32 of 256 threads).
struct CgResident {
    CgState s;
    const double *FF;                 // n x n, column-major, symmetric
    const double *lambda_p;
    int maxiter, nwg;
    unsigned *bar;                    // zeroed before the launch
};

#ifdef BDF_CG_STAMPS      // diagnostic build (tools/c3_cg_stamps.py): workgroup 0's clock (s_memrealtime, 100 MHz) at eight points of every iteration
__device__ unsigned long long g_cgstamps[64 * 8];
#define CGSTAMP(it, k) do { if (blockIdx.x == 0 && threadIdx.x == 0 && (it) < 64) g_cgstamps[(it) * 8 + (k)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define CGSTAMP(it, k) do { } while (0)
#endif

__device__ __forceinline__ void cg_grid_sync(unsigned *bar, unsigned target, int *flag)
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this thread's write-through stores have completed
    __syncthreads();
    if (threadIdx.x == 0) {
        __hip_atomic_fetch_add(bar, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int spins = 0;
        while (__hip_atomic_load(bar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
            __builtin_amdgcn_s_sleep(1);
            if (++spins > (1 << 21)) { atomicOr_system(flag, 16); break; }       // bounded (~0.2 s): a workgroup that is not resident must not hang the device
        }
    }
    __syncthreads();
}

template <int CB>
__global__ __launch_bounds__(256) void k_cg_resident(CgResident c)
{
    __shared__ double red[3][CB][4][64];
    __shared__ double sred[16];
    __shared__ int go;
    // P staged for the product: column c at Pl + c * PSTR (517: an odd stride, the sixteen columns of a matrix operand in sixteen banks)
    constexpr int PSTR = 517, PLD = 32 * CB;               // n <= 512 rows, 16 CB columns: at most 32 CB elements per thread
    __shared__ double Pl[16 * CB * PSTR + 2];
    const CgState &s = c.s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, h = lane >> 4;
    const int w = blockIdx.x;
    const int64_t n = s.n;
    const int D = s.D;
    // (a) this workgroup's rows of the operator: every wave keeps its quarter of K of rows 16 w + i as matrix operands
    // (k_dense_nn's split of K over the waves and its assignment of k to lanes and matrix instructions: the same sums in the same
    // order, so the iterates -- and the iteration counts -- are those of the two-launch solve to the last bit)
    constexpr int KS = 32;
    const int64_t kq = ((n + 3) / 4 + 15) / 16 * 16;               // <= 128 = 4 KS for n <= 512
    const int64_t row = (int64_t)w * 16 + i, kb = (int64_t)wave * kq, ke = (kb + kq < n) ? kb + kq : n;
    double a[KS];
#pragma unroll
    for (int t = 0; t < KS; t++) {
        const int64_t k = kb + 16 * (t >> 2) + 4 * h + (t & 3);
        a[t] = (row < n && k < ke) ? c.FF[k + row * n] : 0.0;      // (symmetric: row `row` is the contiguous column `row`)
    }
    // (b) column w of the solve (k_cg_init and k_cg_pre(1) have run: x = 0, r = p = b, bknum = bkden = |b|^2, iters = 1)
    const int d = w;
    const bool owner = d < D;
    const int64_t off = (int64_t)d * n;
    constexpr int EPT = 2;
    double p[EPT], x[EPT], r[EPT];
    bool active = false;
    double bknum_d = 0.0, bkden_d = 0.0, tolb_d = 0.0;
    int iters_d = 0;
    if (owner) {
#pragma unroll
        for (int e = 0; e < EPT; e++) {
            const int64_t q = tid + 256 * e;
            const bool ok = q < n;
            p[e] = ok ? s.P[off + q] : 0.0; x[e] = ok ? s.X[off + q] : 0.0; r[e] = ok ? s.R[off + q] : 0.0;
        }
        active = s.active[d] != 0; bknum_d = s.bknum[d]; bkden_d = s.bkden[d]; tolb_d = s.tolb[d]; iters_d = s.iters[d];
    }
    const double lambda = *c.lambda_p;
    unsigned sync_no = 0;
    for (int iter = 1; iter <= c.maxiter; iter++) {
        if (__hip_atomic_load(s.nactive, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) break;      // (the same value in every workgroup: read after a hand-over)
        CGSTAMP(iter, 0);
        // ---- Z[rows of w, :] = FF[rows of w, :] P
        // P -- n x D, the columns one after the other: 128 KB at n = 500, D = 32, written by the other workgroups a moment ago -- comes
        // into LDS by COALESCED loads past the L2, all of them in flight at once (a thread's elements are 256 apart), and the matrix
        // operands are read from there.  (Until round 6 every lane fetched its operands itself, 8 bytes at a stride of a column:
        // sixty-four cache lines per instruction -- 7.25 us of an iteration's 12.9, profiles/r06_c3_cg_handover.txt.)  Same operand
        // values into the same matrix instructions in the same order: the iterates are unchanged to the last bit.
        {
            const int64_t total = n * (int64_t)D;
            double pv[PLD];
            // (no branches: an element beyond the end reads the last one again and is not stored)
#pragma unroll
            for (int q = 0; q < PLD; q++) {
                const int64_t e = tid + 256 * q;
                pv[q] = __hip_atomic_load(s.P + (e < total ? e : total - 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            int col = 0;
            int k = tid;
#pragma unroll
            for (int q = 0; q < PLD; q++) {
                // (n >= 128 -- cg_solve takes this kernel for no smaller operator -- : at most two columns' ends per 256 elements)
                const bool w1 = k >= (int)n;
                k -= w1 ? (int)n : 0; col += w1 ? 1 : 0;
                const bool w2 = k >= (int)n;
                k -= w2 ? (int)n : 0; col += w2 ? 1 : 0;
                Pl[col < D ? col * PSTR + k : 16 * CB * PSTR] = pv[q];               // (beyond the end: a spare slot)
                k += 256;
            }
        }
        __syncthreads();
        fd4 acc[CB];
#pragma unroll
        for (int cb = 0; cb < CB; cb++) acc[cb] = fd4{0.0, 0.0, 0.0, 0.0};
        {
#pragma unroll
            for (int t = 0; t < KS; t++) {
                const int64_t k = kb + 16 * (t >> 2) + 4 * h + (t & 3);
#pragma unroll
                for (int cb = 0; cb < CB; cb++) {
                    const int col = 16 * cb + i;
                    const double b = (k < ke && col < D) ? Pl[col * PSTR + k] : 0.0;
                    acc[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t], b, acc[cb], 0, 0, 0);
                }
            }
        }
        CGSTAMP(iter, 1);                  // P loaded (128 KB past the L2, agent scope), the matrix instructions issued
        if (wave > 0) {
#pragma unroll
            for (int cb = 0; cb < CB; cb++)
#pragma unroll
                for (int rr = 0; rr < 4; rr++) red[wave - 1][cb][rr][lane] = acc[cb][rr];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int cb = 0; cb < CB; cb++)
#pragma unroll
                for (int rr = 0; rr < 4; rr++) {
                    const double v = ((acc[cb][rr] + red[0][cb][rr][lane]) + red[1][cb][rr][lane]) + red[2][cb][rr][lane];
                    const int64_t zr = (int64_t)w * 16 + h + 4 * rr;
                    const int col = 16 * cb + i;
                    if (zr < n && col < D) __hip_atomic_store(s.Z + zr + (int64_t)col * n, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
        }
        CGSTAMP(iter, 2);                  // the waves' sums added, Z's rows stored (write-through, not yet drained)
        cg_grid_sync(c.bar, ++sync_no * (unsigned)c.nwg, s.flag);
        CGSTAMP(iter, 3);                  // first hand-over passed: every workgroup's rows of Z are in memory
        // ---- the step of column w: bottom of iteration `iter`, top of iteration `iter + 1` (k_cg_step_short's arithmetic)
        if (owner && active && iters_d == iter) {           // (workgroup-uniform)
            double z[EPT];
            double zp = 0.0;
#pragma unroll
            for (int e = 0; e < EPT; e++) {
                const int64_t q = tid + 256 * e;
                z[e] = q < n ? __hip_atomic_load(s.Z + off + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
                z[e] = fma(lambda, p[e], z[e]);
                zp = fma(z[e], p[e], zp);
            }
            zp = block_sum(zp, sred);
            const double ak = bknum_d / zp;
            double bknum = 0.0;
#pragma unroll
            for (int e = 0; e < EPT; e++) {
                x[e] = fma(ak, p[e], x[e]);
                r[e] = fma(-ak, z[e], r[e]);
                bknum = fma(r[e], r[e], bknum);
            }
            if (iter >= c.maxiter) {
                if (tid == 0) atomicOr_system(s.flag, (int)BDF_WARN_CG_MAXITER);
            } else {
                bknum = block_sum(bknum, sred);
                if (tid == 0) go = !(sqrt(bknum) < tolb_d);
                __syncthreads();
                if (go) {
                    const double bk = bknum / bkden_d;
#pragma unroll
                    for (int e = 0; e < EPT; e++) {
                        p[e] = fma(bk, p[e], r[e]);
                        const int64_t q = tid + 256 * e;
                        if (q < n) __hip_atomic_store(s.P + off + q, p[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                    bkden_d = bknum; bknum_d = bknum; iters_d = iter + 1;
                } else {
                    active = false;
                    if (tid == 0) __hip_atomic_fetch_sub(s.nactive, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                __syncthreads();                          // (`go` is rewritten in the next iteration)
            }
        }
        CGSTAMP(iter, 4);                  // column w's step: Z's column read, two block sums, p stored
        cg_grid_sync(c.bar, ++sync_no * (unsigned)c.nwg, s.flag);
        CGSTAMP(iter, 5);                  // second hand-over passed: every column's new p is in memory
    }
    if (owner) {
#pragma unroll
        for (int e = 0; e < EPT; e++) {
            const int64_t q = tid + 256 * e;
            if (q < n) { s.X[off + q] = x[e]; s.R[off + q] = r[e]; }
        }
        if (tid == 0) { s.active[d] = active ? 1 : 0; s.iters[d] = iters_d; s.bknum[d] = bknum_d; s.bkden[d] = bkden_d; }
    }
}

#ifdef BDF_CG_STAMPS
extern "C" int bdf_debug_cg_stamps(unsigned long long *host512)
{
    BDF_HIP(hipDeviceSynchronize());
    BDF_HIP(hipMemcpyFromSymbol(host512, HIP_SYMBOL(g_cgstamps), sizeof(unsigned long long) * 64 * 8));
    return BDF_OK;
}
#endif

// The CG step for long columns (n > 2048): one workgroup per column is one CU's bandwidth per column (82 us per iteration at
// n = 50,000, D = 32: 32 CUs moving 100 MB).  Here a column is cut into G chunks, grid (D, G), and the step becomes three
// launches with the two dot products summed over the chunks in chunk order by every workgroup that needs them:
//   a: z = Z + lambda p, partial z.p          b: ak; x += ak p; r -= ak z; partial r.r          c: stop test; p = bk p + r
// bkden is double-buffered by iteration parity (slot 1 = s.bkden, written by k_cg_pre at iteration 1; slot 0 = bkden0): in c
// every workgroup of a column reads the old value and the new one goes to the other slot.  active / iters have no second slot: they
// are written by the workgroup of c that finishes last, after every chunk of every column has read them (chunk 0 of a column used to
// write them while the column's other chunks -- unordered against it -- could still be about to read them and then skip their part
// of p: harmless while the grid is resident at once, wrong iterates when it is not).
struct CgChunks { int G; int64_t len; double *partA, *partB, *bkden0; };

__device__ __forceinline__ bool cg_all_stopped(const CgState &s, int iter)
{
    if (*s.nactive != 0) return false;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        s.status[1] = 0;
        __threadfence_system();
        s.status[0] = ((uint64_t)s.gen << 32) | (uint32_t)iter;
    }
    return true;
}

__global__ __launch_bounds__(256) void k_cg_long_a(CgState s, CgChunks c, const double *lambda_p, int iter)
{
    __shared__ double red[16];
    if (cg_all_stopped(s, iter)) return;
    const int d = blockIdx.x, g = blockIdx.y;
    if (!s.active[d] || s.iters[d] != iter) return;
    const double lambda = *lambda_p;
    const int64_t off = (int64_t)d * s.n, i0 = g * c.len, i1 = (i0 + c.len < s.n) ? i0 + c.len : s.n;
    double zp = 0.0;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
        const double p = s.P[off + i];
        const double z = fma(lambda, p, s.Z[off + i]);
        s.Z[off + i] = z;
        zp = fma(z, p, zp);
    }
    zp = block_sum(zp, red);
    if (threadIdx.x == 0) c.partA[d * c.G + g] = zp;
}

__global__ __launch_bounds__(256) void k_cg_long_b(CgState s, CgChunks c, int iter)
{
    __shared__ double red[16];
    if (*s.nactive == 0) return;
    const int d = blockIdx.x, g = blockIdx.y;
    if (!s.active[d] || s.iters[d] != iter) return;
    double zp = 0.0;
    for (int q = 0; q < c.G; q++) zp += c.partA[d * c.G + q];
    const double ak = s.bknum[d] / zp;
    const int64_t off = (int64_t)d * s.n, i0 = g * c.len, i1 = (i0 + c.len < s.n) ? i0 + c.len : s.n;
    double rr = 0.0;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
        s.X[off + i] = fma(ak, s.P[off + i], s.X[off + i]);
        const double r = fma(-ak, s.Z[off + i], s.R[off + i]);
        s.R[off + i] = r;
        rr = fma(r, r, rr);
    }
    rr = block_sum(rr, red);
    if (threadIdx.x == 0) c.partB[d * c.G + g] = rr;
}

__global__ __launch_bounds__(256) void k_cg_long_c(CgState s, CgChunks c, int iter, int maxiter)
{
    if (*s.nactive == 0) return;                          // (a) has reported
    const int d = blockIdx.x, g = blockIdx.y;
    if (s.active[d] && s.iters[d] == iter && iter >= maxiter && g == 0 && threadIdx.x == 0) atomicOr_system(s.flag, (int)BDF_WARN_CG_MAXITER);
    if (s.active[d] && s.iters[d] == iter && iter < maxiter) {      // top of iteration iter + 1 (cg_pre)
        double rr = 0.0;
        for (int q = 0; q < c.G; q++) rr += c.partB[d * c.G + q];
        const bool go = !(sqrt(rr) < s.tolb[d]);
        const double *bk_old = (iter & 1) ? s.bkden : c.bkden0;
        if (go) {
            const double bk = rr / bk_old[d];
            const int64_t off = (int64_t)d * s.n, i0 = g * c.len, i1 = (i0 + c.len < s.n) ? i0 + c.len : s.n;
            for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) s.P[off + i] = fma(bk, s.P[off + i], s.R[off + i]);
        }
    }
    // the columns' bookkeeping by the workgroup that FINISHES LAST, a thread per column (every other workgroup -- the other chunks of
    // the column among them, which nothing orders against chunk 0 -- has read active / iters by then; as in k_cg_rm_c): the same
    // sum of the partials in the same order
    __shared__ int last;
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        last = atomicAdd(s.done_blocks, 1) == s.D * c.G - 1;
    }
    __syncthreads();
    if (!last) return;
    const int dd = threadIdx.x;
    if (dd < s.D && iter < maxiter && s.active[dd] && s.iters[dd] == iter) {
        double rr = 0.0;
        for (int q = 0; q < c.G; q++) rr += c.partB[dd * c.G + q];
        double *bk_new = (iter & 1) ? c.bkden0 : s.bkden;
        if (sqrt(rr) < s.tolb[dd]) { s.active[dd] = 0; atomicSub(s.nactive, 1); }
        else { bk_new[dd] = rr; s.bknum[dd] = rr; s.iters[dd] = iter + 1; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        *s.done_blocks = 0;
        __threadfence();
        const int na = __hip_atomic_load(s.nactive, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s.status[1] = (uint64_t)(iter < maxiter ? na : 0);
        __threadfence_system();
        s.status[0] = ((uint64_t)s.gen << 32) | (uint32_t)iter;
    }
}

// ---- the same solve with its state ROW-MAJOR (element (i, d) at [i * D + d]) -- sparse features (round 6).  The sparse products gather
// ROWS of their dense operand (256 contiguous bytes at D = 32), so with the state column-major, as the reference's matrices are,
// every F'(F p) was wrapped in two tiled transposes (k_to_rowmajor / k_from_rowmajor: 912 + 912 launches per sweep of configuration
// C5).  Here P, Z, R, X live row-major from the solve's first launch to its last: the products take and leave them as they are, and
// the three vector steps take a chunk of rows per workgroup, a thread per (row, column) with the column fastest: 32 lanes read one
// row.  A column's dot products are summed over the chunk's rows in row order by the eight row lanes of a column, then over the
// chunks in chunk order (another order than the column-major kernels': the iterates agree to rounding, not to the bit).
//   rm_init: R = P = b (row-major copy made by k_to_rowmajor), X = 0, partial |b|^2        rm_start: tol |b|, bknum = bkden = |b|^2, iters = 1
//   rm_a / rm_b / rm_c: k_cg_long_a / _b / _c's arithmetic
struct CgRm { int G; int64_t len; double *partA, *partB, *bkden0, *zp, *rrs; };
#define BDF_CG_RM_MAXG 1024

__device__ __forceinline__ double rm_colsum(double v, double (*red)[32], int d, int rl)
{
    // the eight row lanes of column d, added in row-lane order (every thread gets the sum)
    __syncthreads();
    red[rl][d] = v;
    __syncthreads();
    double sum = 0.0;
#pragma unroll
    for (int q = 0; q < 8; q++) sum += red[q][d];
    return sum;
}

// this workgroup's per-column partial to part[d * G + g]; the workgroup that finishes LAST adds the G partials of every column --
// row lane rl those of chunks rl, rl + 8, ..., then the eight row lanes in order: a fixed order whichever workgroup it is -- and
// returns true in it (with the column's sum in `total`)
__device__ __forceinline__ bool rm_reduce(const CgState &s, const CgRm &c, double *part, double v, bool keep, double (*red)[32], int d, int rl, double &total)
{
    __shared__ int last;
    const double mine = rm_colsum(v, red, d, rl);
    if (rl == 0 && keep) __hip_atomic_store(part + d * c.G + blockIdx.x, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) last = __hip_atomic_fetch_add(s.done_blocks, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == c.G - 1;
    __syncthreads();
    if (!last) return false;
    if (threadIdx.x == 0) __hip_atomic_store(s.done_blocks, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // (the partials were written through by the other workgroups: one acquire, then plain loads -- many in flight; taken one by one
    // past the L2 the ~50 loads of a row lane were ~50 round trips: 55 us per iteration)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    double acc = 0.0;
    if (keep) {
        const double *pp = part + d * c.G;
#pragma unroll 8
        for (int q = rl; q < c.G; q += 8) acc += pp[q];
    }
    total = rm_colsum(acc, red, d, rl);
    return true;
}

// the G partials of every column added by THIS workgroup (row lane rl those of chunks rl, rl + 8, ..., then the row lanes in order: the
// same fixed order in every workgroup) -- the vector steps read their dot products this way: a kernel boundary lies between the
// partials' writers and their readers, nothing to wait for
__device__ __forceinline__ double rm_sum_parts(const CgRm &c, const double *part, bool keep, double (*red)[32], int d, int rl)
{
    double acc = 0.0;
    if (keep) {
        const double *pp = part + d * c.G;
#pragma unroll 8
        for (int q = rl; q < c.G; q += 8) acc += pp[q];
    }
    return rm_colsum(acc, red, d, rl);
}

__global__ __launch_bounds__(256) void k_cg_rm_init(CgState s, CgRm c, double tol)
{
    __shared__ double red[8][32];
    const int d = threadIdx.x & 31, rl = threadIdx.x >> 5, g = blockIdx.x;
    const bool dok = d < s.D;
    const int64_t i0 = g * c.len, i1 = (i0 + c.len < s.n) ? i0 + c.len : s.n;
    double nb = 0.0;
    if (dok)
        for (int64_t i = i0 + rl; i < i1; i += 8) {
            const double b = s.R[i * s.D + d];
            s.P[i * s.D + d] = b; s.X[i * s.D + d] = 0.0;
            nb = fma(b, b, nb);
        }
    double tot = 0.0;
    if (!rm_reduce(s, c, c.partA, nb, dok, red, d, rl, tot)) return;
    if (rl == 0 && dok) {
        s.tolb[d] = tol * sqrt(tot);                     // tol = tol * norm(b), parallel_cg.jl:65
        const bool go = !(sqrt(tot) < s.tolb[d]);        // top of iteration 1 (cg_pre): the residual is b
        s.active[d] = go ? 1 : 0; s.iters[d] = go ? 1 : 0;
        s.bkden[d] = tot; s.bknum[d] = tot;
        if (!go) atomicSub(s.nactive, 1);
    }
}

__global__ __launch_bounds__(256) void k_cg_rm_a(CgState s, CgRm c, const double *lambda_p, int iter)
{
    __shared__ double red[8][32];
    if (cg_all_stopped(s, iter)) return;
    const int d = threadIdx.x & 31, rl = threadIdx.x >> 5, g = blockIdx.x;
    const bool act = d < s.D && s.active[d] && s.iters[d] == iter;
    const double lambda = *lambda_p;
    const int64_t i0 = g * c.len, i1 = (i0 + c.len < s.n) ? i0 + c.len : s.n;
    double zp = 0.0;
    if (act)
#pragma unroll 4
        for (int64_t i = i0 + rl; i < i1; i += 8) {
            const double p = s.P[i * s.D + d];
            const double z = fma(lambda, p, s.Z[i * s.D + d]);
            s.Z[i * s.D + d] = z;
            zp = fma(z, p, zp);
        }
    zp = rm_colsum(zp, red, d, rl);
    if (rl == 0 && act) c.partA[d * c.G + g] = zp;
}

__global__ __launch_bounds__(256) void k_cg_rm_b(CgState s, CgRm c, int iter)
{
    __shared__ double red[8][32];
    if (*s.nactive == 0) return;
    const int d = threadIdx.x & 31, rl = threadIdx.x >> 5, g = blockIdx.x;
    const bool act = d < s.D && s.active[d] && s.iters[d] == iter;
    double rr = 0.0;
    const double zp = rm_sum_parts(c, c.partA, act, red, d, rl);
    if (act) {
        const double ak = s.bknum[d] / zp;
        const int64_t i0 = g * c.len, i1 = (i0 + c.len < s.n) ? i0 + c.len : s.n;
#pragma unroll 4
        for (int64_t i = i0 + rl; i < i1; i += 8) {
            const int64_t e = i * s.D + d;
            s.X[e] = fma(ak, s.P[e], s.X[e]);
            const double r = fma(-ak, s.Z[e], s.R[e]);
            s.R[e] = r;
            rr = fma(r, r, rr);
        }
    }
    rr = rm_colsum(rr, red, d, rl);
    if (rl == 0 && act) c.partB[d * c.G + g] = rr;
}

__global__ __launch_bounds__(256) void k_cg_rm_c(CgState s, CgRm c, int iter, int maxiter)
{
    if (*s.nactive == 0) return;                          // (a) has reported
    const int d = threadIdx.x & 31, rl = threadIdx.x >> 5, g = blockIdx.x;
    const bool act = d < s.D && s.active[d] && s.iters[d] == iter;
    if (act && iter >= maxiter && g == 0 && rl == 0) atomicOr_system(s.flag, (int)BDF_WARN_CG_MAXITER);
    bool go = false;
    __shared__ double red[8][32];
    const double rr = rm_sum_parts(c, c.partB, act && iter < maxiter, red, d, rl);
    if (act && iter < maxiter) {                          // top of iteration iter + 1 (cg_pre)
        go = !(sqrt(rr) < s.tolb[d]);
        if (go) {
            const double bk = rr / s.bkden[d];
            const int64_t i0 = g * c.len, i1 = (i0 + c.len < s.n) ? i0 + c.len : s.n;
    #pragma unroll 4
        for (int64_t i = i0 + rl; i < i1; i += 8) { const int64_t e = i * s.D + d; s.P[e] = fma(bk, s.P[e], s.R[e]); }
        }
    }
    // the columns' bookkeeping by the workgroup that FINISHES LAST (every other one has read active / iters / bkden by then)
    __shared__ int last;
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        last = atomicAdd(s.done_blocks, 1) == c.G - 1;
    }
    __syncthreads();
    if (!last) return;
    if (rl == 0 && act && iter < maxiter) {
        if (!go) { s.active[d] = 0; atomicSub(s.nactive, 1); }
        else { s.bkden[d] = rr; s.bknum[d] = rr; s.iters[d] = iter + 1; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        *s.done_blocks = 0;
        __threadfence();
        const int na = __hip_atomic_load(s.nactive, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s.status[1] = (uint64_t)(iter < maxiter ? na : 0);
        __threadfence_system();
        s.status[0] = ((uint64_t)s.gen << 32) | (uint32_t)iter;
    }
}

__global__ void k_cg_rm_zero(CgState s)
{
    if (threadIdx.x == 0) { *s.nactive = s.D; *s.done_blocks = 0; }
}

}  // namespace

// D simultaneous cg_AtA solves of (F'F + lambda I) X = rhs (solve_cg2, parallel_matrix.jl:488-507); with use_ff the operator
// is the precomputed F'F.  R, P, Z: numF x D; Tm: N x D; scal: 3 D doubles; ints: 2 D + 1 ints.
// ctx->cg_part: the partial dot products of the chunked steps -- the column-major kernels' (2 x BDF_MAX_D x 64 + BDF_MAX_D) or the
// row-major ones' (2 x 32 x BDF_CG_RM_MAXG + 128)
constexpr size_t CG_PART_DOUBLES = (size_t)2 * 32 * BDF_CG_RM_MAXG + 128 > (size_t)2 * BDF_MAX_D * 64 + BDF_MAX_D ? (size_t)2 * 32 * BDF_CG_RM_MAXG + 128 : (size_t)2 * BDF_MAX_D * 64 + BDF_MAX_D;
int feat_cg_solve(bdf_ctx *ctx, bdf_feat *f, bool use_ff, int D, const double *lambda_beta_dev, const double *rhs,
                  double *beta_out, double tol, int maxiter, double *R, double *P, double *Z, double *Tm, double *scal,
                  int *ints, int **iters_dev, double *Xrm /* numF x D spare (the row-major solve's X), or NULL */)
{
    const int64_t numF = f->n;
    int rc;
    CgState s;
    s.n = numF; s.D = D; s.X = beta_out; s.R = R; s.P = P; s.Z = Z;
    s.bknum = scal; s.bkden = scal + D; s.tolb = scal + 2 * D;
    s.active = ints; s.iters = ints + D; s.nactive = ints + 2 * D;
    s.done_blocks = ints + 2 * D + 1;
    if (!ctx->cg_status) {
        if (int rc = ctx->cg_status.alloc(2)) return rc;
        ctx->cg_status[0] = ctx->cg_status[1] = 0;
    }
    struct SkipGuard { bdf_ctx *c; ~SkipGuard() { c->skip_flag = nullptr; } } guard{ctx};
    s.status = ctx->cg_status;
    s.flag = ctx->flag_dev;
    s.gen = ++ctx->cg_gen;
    const dim3 cgb(numF >= 8192 ? 1024 : 256);      // threads per column
    // a small resident operator: the whole solve in one launch (k_cg_resident; BDF_CG_RESIDENT=0: the two launches per iteration)
    static const bool resident_ok = !(getenv("BDF_CG_RESIDENT") && atoi(getenv("BDF_CG_RESIDENT")) == 0);
    bool resident = resident_ok && use_ff && numF >= 128 && numF <= 512 && D <= 32 && D <= (numF + 15) / 16;
    if (resident) {
        // its workgroups hand over through a counter they all poll: ALL ceil(numF / 16) of them must be resident at once.  One
        // workgroup per CU is what the kernel's registers and LDS allow for certain (asked of the runtime below), so the stream
        // needs that many CUs: not the reserved hyperprior stream (a handful of CUs), and the row context's CUs minus the
        // reserved ones.  (A caller-supplied CU-masked stream the library cannot see is covered by the spin bound: flag 16.)
        static int occ32 = -1, occ16 = -1;
        if (occ16 < 0) {
            BDF_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ16, k_cg_resident<1>, 256, 0));
            BDF_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ32, k_cg_resident<2>, 256, 0));
        }
        const int avail = ctx->on_reserved ? 0 : std::max(0, ctx->n_cus - ctx->reserve_cus);
        const int per_cu = std::min(1, D <= 16 ? occ16 : occ32);
        resident = (int64_t)per_cu * avail >= (numF + 15) / 16;
    }
    if (resident && !ctx->cg_bar) { if (int rc = ctx->cg_bar.alloc(1)) return rc; }
    // sparse features, long columns: the state ROW-MAJOR from the first launch to the last (k_cg_rm_*): no transposes around the products
    const bool rm = Xrm && !use_ff && f->kind != 0 && numF > 2048 && D <= 32;
    CgRm cr;
    cr.len = 256;                                             // rows per workgroup: thirty-two per row lane (G ~ 200 at 50,000 rows: every workgroup adds G partials per column)
    cr.G = (int)((numF + cr.len - 1) / cr.len);
    if (cr.G > BDF_CG_RM_MAXG) { cr.G = BDF_CG_RM_MAXG; cr.len = (numF + cr.G - 1) / cr.G; cr.G = (int)((numF + cr.len - 1) / cr.len); }
    cr.partA = cr.partB = cr.bkden0 = cr.zp = cr.rrs = nullptr;
    if (rm) {
        if (!ctx->cg_part) { if (int rc = ctx->cg_part.alloc(CG_PART_DOUBLES)) return rc; }
        cr.partA = ctx->cg_part; cr.partB = cr.partA + (size_t)32 * BDF_CG_RM_MAXG; cr.zp = cr.partB + (size_t)32 * BDF_CG_RM_MAXG; cr.rrs = cr.zp + 64;
        // (X row-major in the caller's spare buffer: beta_out is column-major and receives the solution at the end)
        hipLaunchKernelGGL(k_cg_rm_zero, dim3(1), dim3(64), 0, ctx->stream, s);
        feat_to_rowmajor(ctx, numF, D, rhs, 1, numF, R, nullptr);
        s.X = Xrm;
        hipLaunchKernelGGL(k_cg_rm_init, dim3(cr.G), dim3(256), 0, ctx->stream, s, cr, tol);
        BDF_HIP(hipGetLastError());
    } else {
    hipLaunchKernelGGL(k_cg_init, dim3(D), cgb, 0, ctx->stream, s, (const double *)rhs, tol, resident ? ctx->cg_bar : (unsigned *)nullptr);
    BDF_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_cg_pre, dim3(D), cgb, 0, ctx->stream, s, 1);
    }
    // The host enqueues iterations AHEAD of the device (no stream synchronisation: the device never idles between
    // iterations) and reads the (iteration, active columns) word the device writes to host-mapped memory after every
    // iteration.  Run-ahead is bounded to CG_AHEAD iterations; once every column has stopped, the launches already enqueued
    // return at once (product kernels through ctx->skip_flag, the step kernels by themselves).
    // long columns: G chunks per column (k_cg_long_*); the partial dot products live behind the spare scalars
    const bool long_cols = numF > 2048;
    CgChunks ch;
    ch.G = (int)std::min<int64_t>(64, (numF + 4095) / 4096);
    ch.len = (numF + ch.G - 1) / ch.G;
    ch.partA = ch.partB = ch.bkden0 = nullptr;
    if (long_cols) {
        if (!ctx->cg_part) { if (int rc = ctx->cg_part.alloc(CG_PART_DOUBLES)) return rc; }     // (the scratch buffers are reused by the products inside the loop)
        ch.partA = ctx->cg_part; ch.partB = ch.partA + (size_t)BDF_MAX_D * 64; ch.bkden0 = ch.partB + (size_t)BDF_MAX_D * 64;
    }
    if (resident) {
        CgResident c;
        c.s = s; c.FF = f->FF_dev; c.lambda_p = lambda_beta_dev; c.maxiter = maxiter; c.nwg = (int)((numF + 15) / 16); c.bar = ctx->cg_bar;
        if (D <= 16) hipLaunchKernelGGL(k_cg_resident<1>, dim3(c.nwg), dim3(256), 0, ctx->stream, c);
        else hipLaunchKernelGGL(k_cg_resident<2>, dim3(c.nwg), dim3(256), 0, ctx->stream, c);
        BDF_HIP(hipGetLastError());
        *iters_dev = s.iters;
        return BDF_OK;
    }
    constexpr int CG_AHEAD = 3;
    ctx->skip_flag = s.nactive;
    for (int iter = 1; iter <= maxiter; iter++) {
        if (iter > CG_AHEAD) {
            const uint64_t want = ((uint64_t)s.gen << 32) | (uint32_t)(iter - CG_AHEAD);
            uint64_t st;
            long spins = 0;
            while ((st = s.status[0]) < want || (st >> 32) != s.gen) {
                if (++spins > 2000000000L || ((spins & 0xfffff) == 0 && hipStreamQuery(ctx->stream) != hipErrorNotReady)) {
                    // the stream drained without the report (a device fault): stop enqueuing
                    st = s.status[0];
                    if (st < want || (st >> 32) != s.gen) { bdf_set_error("cg_solve: the device did not report iteration %d", iter - CG_AHEAD); return BDF_ERR_HIP; }
                    break;
                }
            }
            if (s.status[1] == 0) break;
        }
        if (use_ff && D <= 64) {
            if ((rc = feat_dense_nn(ctx, f->FF_dev, numF, numF, P, 1, numF, D, Z, 1, numF, nullptr, nullptr))) return rc;
        } else if (use_ff) {
            GemmArgs g;
            g.M = numF; g.N = D; g.K = numF; g.A = f->FF_dev; g.ars = 1; g.acs = numF;
            g.B = P; g.brs = 1; g.bcs = numF; g.C = Z; g.crs = 1; g.ccs = numF; g.bias = nullptr; g.C2 = nullptr;
            if ((rc = feat_gemm(ctx, g))) return rc;
        } else {
            // the N x D intermediate row-major: contiguous writes of the first product, contiguous operand rows of the second
            if (rm) {
                if ((rc = feat_apply(ctx, f, false, P, D, 1, D, Tm, D, 1))) return rc;
                if ((rc = feat_apply(ctx, f, true, Tm, D, 1, D, Z, D, 1))) return rc;
            } else {
                if ((rc = feat_apply(ctx, f, false, P, 1, numF, D, Tm, D, 1))) return rc;
                if ((rc = feat_apply(ctx, f, true, Tm, D, 1, D, Z, 1, numF))) return rc;
            }
        }
        // bottom of this iteration and top of the next in one launch
        if (numF <= 512) hipLaunchKernelGGL(k_cg_step_short<2>, dim3(D), dim3(256), 0, ctx->stream, s, (const double *)lambda_beta_dev, iter, maxiter);
        else if (numF <= 1024) hipLaunchKernelGGL(k_cg_step_short<4>, dim3(D), dim3(256), 0, ctx->stream, s, (const double *)lambda_beta_dev, iter, maxiter);
        else if (numF <= 2048) hipLaunchKernelGGL(k_cg_step_short<8>, dim3(D), dim3(256), 0, ctx->stream, s, (const double *)lambda_beta_dev, iter, maxiter);
        else if (rm) {
            hipLaunchKernelGGL(k_cg_rm_a, dim3(cr.G), dim3(256), 0, ctx->stream, s, cr, (const double *)lambda_beta_dev, iter);
            hipLaunchKernelGGL(k_cg_rm_b, dim3(cr.G), dim3(256), 0, ctx->stream, s, cr, iter);
            hipLaunchKernelGGL(k_cg_rm_c, dim3(cr.G), dim3(256), 0, ctx->stream, s, cr, iter, maxiter);
        } else {
            hipLaunchKernelGGL(k_cg_long_a, dim3(D, ch.G), dim3(256), 0, ctx->stream, s, ch, (const double *)lambda_beta_dev, iter);
            hipLaunchKernelGGL(k_cg_long_b, dim3(D, ch.G), dim3(256), 0, ctx->stream, s, ch, iter);
            hipLaunchKernelGGL(k_cg_long_c, dim3(D, ch.G), dim3(256), 0, ctx->stream, s, ch, iter, maxiter);
        }
        BDF_HIP(hipGetLastError());
    }
    ctx->skip_flag = nullptr;
    if (rm) {
        // the solution, row-major in s.X, into the caller's column-major beta_out
        feat_from_rowmajor(ctx, numF, D, s.X, beta_out, 1, numF, nullptr, nullptr, nullptr);
        BDF_HIP(hipGetLastError());
    }
    *iters_dev = s.iters;
    return BDF_OK;
}
