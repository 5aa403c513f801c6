// k_gather_image.hip -- K1c's gather image of a sample that something other than a K1c launch wrote: the initial state, a state put
// back (bdf_gibbs_warm_device, bdf_gibbs_set_recorded), a sample the host wrote, the rows of another row kernel.
//
// The image is a second, lane-ordered copy of an entity's sample at D = 32, read only by K1c's gathers (k_rows_col.hip,
// col_gather4).  Lane j of a lane row gathers, of every observation's factor row, v0_j = element 31 - j and v1_j = element 15 - j,
// and col_rank1u (dpp_rows32.h) derives from them x_j = (j >= 8 ? v0_j : v1_j) and y_j = (j >= 8 ? v1_j : v0 of lane j ^ 8):
//   tier 1, the pair image   row i, lane j: [v0_j, v1_j]             at doubles 32 i + 2 j        (the default)
//   tier 2, the full image   row i, lane j: [v0_j, v1_j, x_j, y_j]   at doubles 64 i + 4 j        (bdf_ctx_set_gather_image(ctx, 2))
// A K1c launch that gathers from an image leaves the image of its own rows (its producer stores); this kernel makes the same bytes
// from the natural rows.
#include "rows.h"

namespace {

__global__ __launch_bounds__(256) void k_gather_image(const double *__restrict__ sample, double *__restrict__ image, int64_t M, int tier)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= M * 16) return;
    const int64_t i = t >> 4;
    const int j = (int)(t & 15);
    const double *r = sample + i * 32;
    const double v0 = r[31 - j], v1 = r[15 - j];
    if (tier == 2) {
        const bool h = j >= 8;
        double *d = image + i * 64 + j * 4;
        d[0] = v0; d[1] = v1;
        d[2] = h ? v0 : v1;
        d[3] = h ? v1 : r[31 - (j ^ 8)];
    } else {
        double *d = image + i * 32 + j * 2;
        d[0] = v0; d[1] = v1;
    }
}

}  // namespace

int bdf_gather_image_pack_launch(bdf_ctx *ctx, const double *sample, int64_t M, int tier, double *image)
{
    BDF_REQUIRE(ctx && sample && image && M >= 0 && (tier == 1 || tier == 2), BDF_ERR_ARG, "bdf_gather_image_pack: bad argument");
    if (M == 0) return BDF_OK;
    BDF_REQUIRE(M <= bdf_col_image_max_rows(), BDF_ERR_ARG, "bdf_gather_image_pack: %lld rows (at most %lld)", (long long)M, (long long)bdf_col_image_max_rows());
    const unsigned blocks = (unsigned)((M * 16 + 255) / 256);
    hipLaunchKernelGGL(k_gather_image, dim3(blocks), dim3(256), 0, ctx->stream, sample, image, M, tier);
    BDF_HIP(hipGetLastError());
    return BDF_OK;
}
