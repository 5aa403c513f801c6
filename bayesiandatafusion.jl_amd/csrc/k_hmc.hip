// k_hmc.hip -- Hamiltonian Monte Carlo BPMF (src/macau_hmc.jl:35-86, 152-264): the leapfrog, the energies and the Metropolis
// step.
//
// Leapfrog (one launch per hmc_update_u! call, every row of the entity).  Within a call the other entity is fixed, and row n's
// gradient reads only u_n, its momentum, the other entity's rows, Lambda and mu: so a launch runs all L_inner inner steps of
// every row with no barrier between them.  A workgroup of four waves takes one row of the degree-descending order: it is
// cut into 256 / DP groups of DP lanes (DP = 16, 32, 64 is the padded dimension), lane c of every group holding element c
// of u_n and of its momentum, and the groups deal the row's neighbours among them (the longest rows, thousands of
// neighbours on MovieLens, bound the launch: one group per row was latency-bound at ~0.5 ms a launch).  The gradient is
// taken in the residual form
//     g_n = Lambda (u_n - mu) - alpha sum_j v_j (r_j - v_j . u_n)
// over the summed-duplicate CSR (the reference's sparse(vid, uid, val)), re-gathering the other entity's rows for every
// evaluation (a group of DP lanes reads row j as consecutive doubles, four neighbours in flight per group; the dot products
// by a butterfly, which gives every lane of the group the same bits; the groups' sums added in group order through LDS).
// The energies ride on the same launches: the first launch of an entity draws its momentum (Philox stream
// BDF_P_HMC_MOMENTUM), keeps the start copy and sums the start terms; the last one sums the final terms; U's launches add the
// data term of every observation, c d^2 - 2 d sum(val) + sum(val^2) per summed duplicate group.  Every launch leaves
// per-block partial sums, and a one-workgroup kernel adds them in block order, forms dH, draws the uniform and decides: no
// floating-point atomics, so reruns give the same bits.
#include "hmc.h"
#include "wave_linalg.h"

namespace {

template <int DP>
__global__ __launch_bounds__(256) void k_hmc_leap(HMCLeapArgs a)
{
    constexpr int NG = 256 / DP;                       // lane groups of the workgroup, all on the same row
    constexpr int U = 4;                               // neighbours in flight per group
    __shared__ double sLam[DP * DP];                   // Lambda, zero-padded (column k at k DP)
    __shared__ double sm[DP];                          // Lambda mu
    __shared__ double su[NG][DP];                      // every group's copy of the current u, for Lambda u
    __shared__ double sacc[NG][DP];                    // the groups' sums over their neighbours
    __shared__ double sds[NG];                         // ... and their data terms
    __shared__ double red[4][HMC_PW];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int g = tid / DP, c = tid % DP, D = a.D;
    for (int t = tid; t < DP * DP; t += 256) {
        const int i = t % DP, k = t / DP;
        sLam[t] = (i < D && k < D) ? a.Lambda[k * D + i] : 0.0;
    }
    __syncthreads();
    if (tid < DP) {
        double m = 0.0;
        for (int k = 0; k < D; k++) m = fma(sLam[k * DP + tid], a.mu[k], m);
        sm[tid] = m;                                   // zero past D (sLam is)
    }
    __syncthreads();

    // one row per workgroup (grid = N): every group keeps the row's u and momentum (the same bits), group 0 writes them
    const int32_t row = a.order[blockIdx.x];
    const int64_t q0 = a.rowptr[row], q1 = a.rowptr[row + 1];
    const bool inD = c < D, own = g == 0 && c < D;
    const int64_t idx = (int64_t)row * D + c;
    const double Gc = inD ? a.G[c] : 1.0, mc = sm[c];
    double u = inD ? a.sample[idx] : 0.0, r = inD ? a.mom[idx] : 0.0;
    double part[HMC_PW];
#pragma unroll
    for (int f = 0; f < HMC_PW; f++) part[f] = 0.0;

    if ((a.flags & HMC_DRAW) && inD) {
        // sample!(m) (macau_hmc.jl:153-160): r = randn() / sqrt(G)
        const double z = bdf_normal(a.seed, a.sweep, BDF_P_HMC_MOMENTUM, a.tag, (uint64_t)row, c);
        r = z / sqrt(Gc);
        if (own) {
            a.start[idx] = u;
            part[HMC_KIN_S] = r * r * Gc + log(Gc);
            part[HMC_USQ_S] = u * u;
        }
    }

    // grad(n, ...) (macau_hmc.jl:228-246) at uu; w = (Lambda uu)_c; with `data` the row's data term goes to dsum
    auto grad = [&](double uu, bool data, double &w, double &dsum) -> double {
        wave_sync();
        su[g][c] = uu;
        wave_sync();
        double ww = 0.0;
        for (int k = 0; k < D; k++) ww = fma(sLam[k * DP + c], su[g][k], ww);
        double acc = 0.0, ds = 0.0;
        for (int64_t q = q0 + g; q < q1; q += NG * U) {     // neighbour q to group (q - q0) mod NG; uniform within a group
            double v[U], rv[U], d[U];
            bool ok[U];
#pragma unroll
            for (int t = 0; t < U; t++) {
                ok[t] = q + NG * t < q1;
                const int64_t j = ok[t] ? (int64_t)a.colidx[q + NG * t] : 0;
                rv[t] = ok[t] ? a.vals[q + NG * t] : 0.0;
                v[t] = (ok[t] && inD) ? a.other[j * D + c] : 0.0;
            }
#pragma unroll
            for (int t = 0; t < U; t++) d[t] = v[t] * uu;
#pragma unroll
            for (int off = 1; off < DP; off <<= 1)
#pragma unroll
                for (int t = 0; t < U; t++) d[t] += __shfl_xor(d[t], off);
#pragma unroll
            for (int t = 0; t < U; t++) acc = fma(v[t], rv[t] - d[t], acc);
            if (data && c == 0) {
#pragma unroll
                for (int t = 0; t < U; t++)
                    if (ok[t]) {
                        const double2 cq = *(const double2 *)(a.cs + 2 * (q + NG * t));
                        ds += (cq.x * (d[t] * d[t]) - 2.0 * d[t] * rv[t]) + cq.y;
                    }
            }
        }
        // the groups' sums, added in group order by every lane (the same bits everywhere)
        __syncthreads();
        sacc[g][c] = acc;
        if (c == 0) sds[g] = ds;
        __syncthreads();
        double tot = 0.0, dt = 0.0;
#pragma unroll
        for (int k = 0; k < NG; k++) tot += sacc[k][c];
        if (data) {
#pragma unroll
            for (int k = 0; k < NG; k++) dt += sds[k];
        }
        w = ww;
        dsum += dt;
        return (ww - mc) - a.alpha * tot;
    };

    // hmc_update_u! (macau_hmc.jl:163-191)
    const double e = a.eps, h = 0.5 * a.eps;
    const bool dat = (a.flags & HMC_DATA) != 0;
    double w = 0.0, dsum = 0.0;
    double gr = grad(u, dat && (a.flags & HMC_DRAW), w, dsum);
    if ((a.flags & HMC_DRAW) && own) {
        part[HMC_PRI_S] = u * (0.5 * w - mc);
        if (c == 0) part[HMC_DAT_S] = dsum;
    }
    r = r - h * gr;
    for (int i = 1; i <= a.L_inner; i++) {
        u = u + e * r;
        dsum = 0.0;
        gr = grad(u, dat && (a.flags & HMC_FINAL) && i == a.L_inner, w, dsum);
        if (i < a.L_inner) r = r - e * gr;
    }
    r = r - h * gr;

    if (own) {
        a.sample[idx] = u;
        a.mom[idx] = r;
        part[HMC_MSQ] = r * r;
        part[HMC_USQ] = u * u;
        if (a.flags & HMC_FINAL) {
            part[HMC_KIN_F] = r * r * Gc + log(Gc);
            part[HMC_PRI_F] = u * (0.5 * w - mc);
            if (c == 0) part[HMC_DAT_F] = dsum;
        }
    }
    // the workgroup's partial sums: lanes by a butterfly, then the four waves in order (only group 0's lanes hold any)
#pragma unroll
    for (int f = 0; f < HMC_PW; f++) {
        double x = part[f];
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) x += __shfl_xor(x, off);
        if (lane == 0) red[wave][f] = x;
    }
    __syncthreads();
    if (tid < HMC_PW) a.partial[(int64_t)blockIdx.x * HMC_PW + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

__device__ __forceinline__ int64_t slot_offset(const HMCAcceptArgs &a, int s)
{
    // launches alternate U, V, U, ..., U: before launch s lie (s + 1) / 2 U launches and s / 2 V launches
    return ((int64_t)((s + 1) / 2) * a.nb[0] + (int64_t)(s / 2) * a.nb[1]) * HMC_PW;
}

// macau_hmc.jl:73-105: the energies, dH, the Metropolis decision and the step-size adaptation; the iteration record
__global__ __launch_bounds__(1024) void k_hmc_accept(HMCAcceptArgs a)
{
    constexpr int NE = 14;
    __shared__ double res[NE];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int L = a.L, nlog = 2 * L + 1;
    // energy task k: (launch, field)
    const int es[NE] = {0, 0, 0, 0, 1, 1, 1, 2 * L, 2 * L, 2 * L, 2 * L, 2 * L - 1, 2 * L - 1, 2 * L - 1};
    const int ef[NE] = {HMC_KIN_S, HMC_PRI_S, HMC_DAT_S, HMC_USQ_S, HMC_KIN_S, HMC_PRI_S, HMC_USQ_S,
                        HMC_KIN_F, HMC_PRI_F, HMC_DAT_F, HMC_USQ, HMC_KIN_F, HMC_PRI_F, HMC_USQ};
    for (int t = wave; t < nlog + NE; t += 16) {
        const int s = t < nlog ? t : es[t - nlog];
        const int f = t < nlog ? HMC_MSQ : ef[t - nlog];
        const int64_t nb = a.nb[s & 1];
        const double *p = a.partial + slot_offset(a, s) + f;
        double x = 0.0;
        for (int64_t b = lane; b < nb; b += 64) x += p[b * HMC_PW];
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) x += __shfl_xor(x, off);
        if (lane == 0) {
            if (t < nlog) a.rec[HMC_REC_LOG + t] = sqrt(x);
            else res[t - nlog] = x;
        }
    }
    __syncthreads();
    if (tid != 0) return;
    // computeKinetic (:206-215) and computePotential (:218-243) of U plus V
    const double kin_s = 0.5 * res[0] + 0.5 * res[4];
    const double kin_f = 0.5 * res[7] + 0.5 * res[11];
    const double pot_s = (res[2] * (a.alpha / 2.0) + res[1]) + res[5];
    const double pot_f = (res[9] * (a.alpha / 2.0) + res[8]) + res[12];
    const double dH = pot_s - pot_f + kin_s - kin_f;
    const double uni = bdf_uniform(a.seed, a.sweep, BDF_P_HMC_ACCEPT, 0, 0, 0);
    const bool accept = uni < exp(dH);
    double eps_new = a.eps;
    int L_new = L;
    if (!accept && dH < -6.0) {
        eps_new = a.eps / 2.0;
        L_new = (int)ceil((double)L * 1.6);
    }
    if (!(isfinite(kin_s) && isfinite(kin_f) && isfinite(pot_s) && isfinite(pot_f))) atomicOr_system(a.flag, HMC_FLAG_ENERGY);
    double *rec = a.rec;
    rec[HMC_REC_I] = (double)a.sweep;
    rec[HMC_REC_EPS] = a.eps;
    rec[HMC_REC_L] = (double)L;
    rec[HMC_REC_KIN_S] = kin_s;
    rec[HMC_REC_KIN_F] = kin_f;
    rec[HMC_REC_POT_S] = pot_s;
    rec[HMC_REC_POT_F] = pot_f;
    rec[HMC_REC_DH] = dH;
    rec[HMC_REC_ACCEPT] = accept ? 1.0 : 0.0;
    rec[HMC_REC_EPS_NEW] = eps_new;
    rec[HMC_REC_L_NEW] = (double)L_new;
    rec[HMC_REC_NORM_U] = sqrt(accept ? res[10] : res[3]);
    rec[HMC_REC_NORM_V] = sqrt(accept ? res[13] : res[6]);
    rec[HMC_REC_UNIFORM] = uni;
}

// copy!(sample, start) on rejection (:90-91), both entities
__global__ __launch_bounds__(256) void k_hmc_restore(HMCRestoreArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (a.rec[HMC_REC_ACCEPT] != 0.0) return;
#pragma unroll
    for (int e = 0; e < 2; e++)
        if (i < a.n[e]) a.sample[e][i] = a.start[e][i];
}

// yhat = clamp!(pred(rel, test)), update_yhat_post! (:110-113, 277-288) and the two squared errors, per block
__global__ __launch_bounds__(256) void k_hmc_predict(HMCPredictArgs a)
{
    __shared__ double red[4][2];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t i = (int64_t)blockIdx.x * 256 + tid;
    double e1 = 0.0, e2 = 0.0;
    if (i < a.n) {
        const double *u = a.U + (int64_t)a.ids[i] * a.D, *v = a.V + (int64_t)a.ids[a.n + i] * a.D;
        double d = 0.0;
        for (int k = 0; k < a.D; k++) d = fma(u[k], v[k], d);
        double y = d + a.mean;
        const bool cl = a.lo <= a.hi;
        if (cl && y < a.lo) y = a.lo;
        if (cl && y > a.hi) y = a.hi;
        // clamp! works in place: the running mean is of the clamped predictions
        const double avg = a.copy ? y : (a.count * a.avg[i] + y) / (a.count + 1.0);
        a.avg[i] = avg;
        double ac = avg;
        if (cl && ac < a.lo) ac = a.lo;
        if (cl && ac > a.hi) ac = a.hi;
        const double t = a.values[i];
        e1 = (y - t) * (y - t);
        e2 = (ac - t) * (ac - t);
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        e1 += __shfl_xor(e1, off);
        e2 += __shfl_xor(e2, off);
    }
    if (lane == 0) { red[wave][0] = e1; red[wave][1] = e2; }
    __syncthreads();
    if (tid < 2) a.partial[(int64_t)blockIdx.x * 2 + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

template <int DP>
int launch_leap(hipStream_t s, const HMCLeapArgs &a)
{
    hipLaunchKernelGGL(k_hmc_leap<DP>, dim3((unsigned)hmc_row_blocks(a.D, a.N)), dim3(256), 0, s, a);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}

}  // namespace

int64_t hmc_row_blocks(int, int64_t N) { return N; }

int hmc_launch_leap(hipStream_t s, const HMCLeapArgs &a)
{
    if (a.N == 0) return BDF_OK;
    if (a.D <= 16) return launch_leap<16>(s, a);
    if (a.D <= 32) return launch_leap<32>(s, a);
    return launch_leap<64>(s, a);
}

int hmc_launch_accept(hipStream_t s, const HMCAcceptArgs &a)
{
    hipLaunchKernelGGL(k_hmc_accept, dim3(1), dim3(1024), 0, s, a);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}

int hmc_launch_restore(hipStream_t s, const HMCRestoreArgs &a)
{
    const int64_t n = a.n[0] > a.n[1] ? a.n[0] : a.n[1];
    if (n == 0) return BDF_OK;
    hipLaunchKernelGGL(k_hmc_restore, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}

int64_t hmc_predict_blocks(int64_t n) { return (n + 255) / 256; }

int hmc_launch_predict(hipStream_t s, const HMCPredictArgs &a)
{
    if (a.n == 0) return BDF_OK;
    hipLaunchKernelGGL(k_hmc_predict, dim3((unsigned)hmc_predict_blocks(a.n)), dim3(256), 0, s, a);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}
