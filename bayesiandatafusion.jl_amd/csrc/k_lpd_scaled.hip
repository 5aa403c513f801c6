// k_lpd_scaled.hip -- bdf_pairs_lpd_update for pairs with a precision scale (bdf_pairs_set_precision_scale): a
// cell is scored with alpha tau[its id in one mode], as a Gaussian measurement and as the mass of an interval alike.  The body is
// k_lpd's (lpd_body.h) with SCALED set: one 8-byte gather and one multiplication in the lane that owns the pair.  A unit of its
// own, so that k_lpd.hip compiles to what it was.
//
// No LDS beyond the statistics' reduction, no scratch, plain vector stores.
#include "lpd_body.h"

namespace {

template <int NM, int VEC, int NC>
__global__ __launch_bounds__(256, (VEC == 4 && NM * NC >= 8) ? 2 : 3) void k_lpd_scaled(LpdArgs a)
{
    lpd_body<NM, VEC, NC, true>(a);
}

}  // namespace

int bdf_lpd_launch_scaled(bdf_ctx *ctx, int n_modes, int D, int nblocks, const void *args, size_t args_bytes, double *stats_out)
{
    BDF_REQUIRE(args && args_bytes == sizeof(LpdArgs), BDF_ERR_ARG, "bdf_lpd_launch_scaled: the two units disagree on the launch arguments");
    LpdArgs a = *(const LpdArgs *)args;
    return launch_reduced(ctx, nblocks, a.rec.partial, stats_out, [&] { BDF_BY_SHAPE(k_lpd_scaled, n_modes, D, nblocks, ctx->stream, a); });
}
