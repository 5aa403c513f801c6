// k_rows_ss.hip -- the row kernel of the spike-and-slab prior.
//
// The conditional of a row is no longer Gaussian, so of K1 (k_sample_rows.hip) only the first half applies: the work
// decomposition (one wave per item; a row of several items publishes partials to the slab and the wave that completes it
// finishes it), the gathers and the f64-MFMA accumulation of P_i and c_i -- k1_accumulate.h, shared, with Lambda = diag(tau)
// and mu = 0 as the prior.  The finish is spike.h's D-step coordinate sweep over (s_d, w_d) with w_d integrated out of the
// inclusion odds, in place of the factorisation and the two solves.  Every term takes the general gather (the variant
// BDF_K1_GENERAL_KERNEL forces on K1), weighted when a term carries observation weights.  The kernel polls nothing.
#include "k1_accumulate.h"

namespace {

// waves per SIMD: after the transpose a lane holds a row of P (2 DP registers) beside the sweep's few values; before it, the
// accumulators.  The bounds below keep every variant free of scratch (tests/test_spike_host.py reads the build's resource usage):
// at D > 32 the transpose needs about 286 registers, 30 more than two waves per SIMD leave a wave, so that variant is built for one
// and keeps the excess in accumulation registers.
template <int DP>
struct SsWaves { static constexpr int value = DP == 64 ? 1 : (DP == 32 ? 4 : 6); };

template <int DP, bool WEIGHTED>
__global__ __launch_bounds__(64 * Geo<DP>::WPB, SsWaves<DP>::value)
void k_rows_ss(SampleArgs a, PlanDev p)
{
    constexpr int WPB = Geo<DP>::WPB;
    constexpr int WLDS = SpikeGeo<DP>::WAVE_LDS;
    __shared__ __attribute__((aligned(16))) double lds[WPB * WLDS];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t w = (int64_t)blockIdx.x * WPB + wave;
    if (w < (int64_t)p.n_split + p.n_direct)
        process_item<DP, false, false, false, WEIGHTED, true>(a, p, p.order[w], lane, lds + wave * WLDS);
}

template <int DP>
int launch(bdf_ctx *ctx, const SampleArgs &a, const PlanDev &p, hipEvent_t e0, hipEvent_t e1)
{
    constexpr int WPB = Geo<DP>::WPB;
    bool weighted = false;
    for (int r = 0; r < a.n_terms; r++) weighted = weighted || a.t[r].weight != nullptr;
    const int64_t waves = (int64_t)p.n_split + p.n_direct;
    const dim3 grid((unsigned)((waves + WPB - 1) / WPB)), block(64 * WPB);
    auto kern = weighted ? k_rows_ss<DP, true> : k_rows_ss<DP, false>;
    hipExtLaunchKernelGGL(kern, grid, block, 0, ctx->stream, e0, e1, 0, a, p);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}

}  // namespace

int bdf_ss_launch(bdf_ctx *ctx, const SampleArgs &a, const PlanDev &p, hipEvent_t e0, hipEvent_t e1)
{
    const int DP = bdf_rows_dp(a.D);
    if (DP == 16) return launch<16>(ctx, a, p, e0, e1);
    if (DP == 32) return launch<32>(ctx, a, p, e0, e1);
    return launch<64>(ctx, a, p, e0, e1);
}
