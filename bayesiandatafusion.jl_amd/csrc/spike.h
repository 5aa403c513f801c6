// spike.h -- the spike-and-slab prior of an entity's rows: what the row kernel (k_rows_ss.hip), the
// hyper step (k_spike_hyper.hip) and the router (rows_plan.hip) share.
//
//   u_id = s_id w_id,  s_id ~ Bernoulli(pi_d),  w_id ~ N(0, 1 / tau_d),  pi_d ~ Beta(incl_a, incl_b),  tau_d ~ Gamma(shape, rate)
//
// spike_state: 4 D doubles in device memory, component d at
//   [d] pi_d    [D + d] tau_d    [2 D + d] logit pi_d    [3 D + d] log tau_d
// The row kernel reads tau (through the prior image of diag(tau)), logit pi and log tau; pi is kept for the result.
#pragma once
#include "rows.h"
#include "wave_linalg.h"
#include "c_layout_chol.h"

#define BDF_SPIKE_PI(D, d) (d)
#define BDF_SPIKE_TAU(D, d) ((D) + (d))
#define BDF_SPIKE_LOGIT(D, d) (2 * (D) + (d))
#define BDF_SPIKE_LOGTAU(D, d) (3 * (D) + (d))
// rows per partial of the hyper step's counts and sums of squares: fixed, so that the order of the sums does not depend on the grid
#define BDF_SPIKE_ROWS_PER_BLOCK 256
#define BDF_SPIKE_MAX_BLOCKS ((int64_t)0x7fffffff)      // one workgroup per partial: what a grid's x dimension takes

// doubles of LDS a wave of k_rows_ss needs: one panel of 16 columns of P, DP rows of 17 (an odd stride: lane e reads row e)
template <int DP>
struct SpikeGeo { static constexpr int LD = 17; static constexpr int WAVE_LDS = DP * LD; };

namespace {

// ---- the finish of k_rows_ss: the D-step coordinate sweep over (s_d, w_d) of one row ---------------------------------------
// In: acc / bv, the row's P = diag(tau) + sum alpha sum omega w w' and c in the accumulator layout (index-reversed: element e is
// component D-1-e; the padding e >= D is the identity with c = 0); z and uu, in lane e < D the normal and the uniform of
// component D-1-e.
// P leaves the accumulator layout one block column (16 columns, DP rows) at a time through the wave's LDS: afterwards lane e
// holds row e of the symmetric P in registers (Prow[c] = P_ec = P_ce), its own c_e, u_e and P_ee.  What does not change during the
// sweep is made once, in every lane for its own component: 1 / P_ee, z / sqrt(P_ee) and logit pi + (log tau - log P_ee) / 2.
// g = c - P u is formed by DP column updates (u_c broadcast by v_readlane).  Step d (e = D-1-d, the unrolled loop's constant)
// is evaluated by every lane on its own values -- only lane e's are meaningful --, then delta = u_e(new) - u_e(old) is read
// from lane e and g -= delta Prow[e] (a compile-time register): no LDS traffic and no reduction inside the sweep.
template <int DP>
__device__ __forceinline__ void spike_finish(const SampleArgs &a, d4 (&acc)[Geo<DP>::NB], double (&bv)[Geo<DP>::DB], const double z,
                                             const double uu, const int64_t row, const int lane, double *pan)
{
    using GG = Geo<DP>;
    constexpr int DB = GG::DB, LD = SpikeGeo<DP>::LD;
    const int D = a.D, j = lane & 15, h = lane >> 4;
    const int el = lane < DP ? lane : 0;              // (DP < 64: the lanes past DP repeat lane 0's reads and write nothing)
    double Prow[DP];
    double lam = 1.0;
    static_for<DB>([&](auto Jc_) {
        constexpr int Jc = decltype(Jc_)::value;
        wave_sync();                                  // the previous panel has been read
#pragma unroll
        for (int I = 0; I < DB; I++) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                // block (I, Jc) holds rows 16 I + h + 4 r of the panel's column j; above the diagonal block the mirror image
                // of block (Jc, I): its element (16 Jc + h + 4 r, 16 I + j) is row 16 I + j of the panel's column h + 4 r
                if (I >= Jc) pan[(16 * I + h + 4 * r) * LD + j] = acc[GG::blk(I, Jc)][r];
                else pan[(16 * I + j) * LD + h + 4 * r] = acc[GG::blk(Jc, I)][r];
            }
        }
        wave_sync();
#pragma unroll
        for (int c = 0; c < 16; c++) Prow[16 * Jc + c] = pan[el * LD + c];
        const double dg = pan[el * LD + (el & 15)];
        lam = ((el >> 4) == Jc) ? dg : lam;
    });
    double ce = 0.0;
#pragma unroll
    for (int J = 0; J < DB; J++) ce = ((el >> 4) == J) ? bv[J] : ce;

    const bool mine = lane < D;
    const int d = mine ? D - 1 - lane : 0;
    double u = mine ? a.u_current[row * D + d] : 0.0;
    const double logit = a.spike_state[BDF_SPIKE_LOGIT(D, d)], logtau = a.spike_state[BDF_SPIKE_LOGTAU(D, d)];
    // a diagonal entry that is not positive and finite: the flag a bad pivot sets
    if (mine && !(lam > 0.0 && lam < __builtin_inf())) atomicOr_system(a.flag, 1);
    const double rl = 1.0 / lam;
    const double zs = z / sqrt(lam);
    const double base = logit + 0.5 * (logtau - log(lam));

    double g = ce;
    static_for<DP>([&](auto c_) {
        constexpr int c = decltype(c_)::value;
        g = fma(-readlane_f64(u, c), Prow[c], g);
    });
    static_for<DP>([&](auto k_) {
        constexpr int e = DP - 1 - decltype(k_)::value;          // component d = D-1-e: d ascending
        if (e < D) {                                             // (wave-uniform)
            const double m = fma(lam, u, g) * rl;                // (c_d - sum_{k != d} P_dk u_k) / P_dd
            const double lo = fma(0.5 * lam * m, m, base);
            const bool s = uu < 1.0 / (1.0 + exp(-lo));
            const double un = s ? m + zs : 0.0;
            const double delta = readlane_f64(un - u, e);
            g = fma(-delta, Prow[e], g);
            u = (lane == e) ? un : u;
        }
    });
    if (mine) a.out[row * D + d] = u;
}

}  // namespace
