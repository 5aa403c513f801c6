// pair_gather.h -- the gather that the kernels of k_probit.hip and k_censored.hip share: the dot products of 8 consecutive pairs
// by a group of 8 lanes, as k_predict.hip's general kernel forms them, and the choice of a kernel variant by the shape.
// File-local in every unit that includes it.
#pragma once
#include "bdf_common.h"

namespace {

// the dot products of the 8 consecutive pairs p0 .. p0 + 7 of a group of 8 lanes; my[k]: the id in mode k of pair p0 + sub.
// Returns, in lane sub, the dot product of pair p0 + sub.  VEC = 4: D a multiple of 4, NC 32-byte pieces of a row per lane
// (D <= 32: one, D <= 64: two); VEC = 1: any D, a lane takes elements sub, sub + 8, ...
template <int NM, int VEC, int NC>
__device__ __forceinline__ double group_dots(const double *const (&fac)[BDF_MAX_MODES], int D, int64_t n, int64_t p0, int sub,
                                             const int32_t (&my)[NM])
{
    constexpr int BATCH = (VEC == 1) ? 2 : (NC * NM <= 3 ? 4 : 2);
    double keep = 0.0;
#pragma unroll
    for (int u0 = 0; u0 < 8; u0 += BATCH) {
        if (p0 + u0 >= n) break;                       // group-uniform
        double s[BATCH];
        if constexpr (VEC == 4) {
            double4 f[BATCH][NM][NC];
#pragma unroll
            for (int u = 0; u < BATCH; u++)
#pragma unroll
                for (int k = 0; k < NM; k++) {
                    const double *row = fac[k] + (int64_t)__shfl(my[k], u0 + u, 8) * D;
#pragma unroll
                    for (int c = 0; c < NC; c++) {
                        const int e = sub * 4 + 32 * c;
                        f[u][k][c] = e < D ? *(const double4 *)(row + e) : double4{0.0, 0.0, 0.0, 0.0};
                    }
                }
#pragma unroll
            for (int u = 0; u < BATCH; u++) {
                double acc = 0.0;
#pragma unroll
                for (int c = 0; c < NC; c++) {
                    double4 p = f[u][0][c];
#pragma unroll
                    for (int k = 1; k < NM; k++) { p.x *= f[u][k][c].x; p.y *= f[u][k][c].y; p.z *= f[u][k][c].z; p.w *= f[u][k][c].w; }
                    if (sub * 4 + 32 * c < D) acc += (p.x + p.y) + (p.z + p.w);
                }
                s[u] = acc;
            }
        } else {
#pragma unroll
            for (int u = 0; u < BATCH; u++) {
                const double *row[NM];
#pragma unroll
                for (int k = 0; k < NM; k++) row[k] = fac[k] + (int64_t)__shfl(my[k], u0 + u, 8) * D;
                double acc = 0.0;
                for (int e = sub; e < D; e += 8) {
                    double p = 1.0;
#pragma unroll
                    for (int k = 0; k < NM; k++) p *= row[k][e];
                    acc += p;
                }
                s[u] = acc;
            }
        }
#pragma unroll
        for (int u = 0; u < BATCH; u++) {
            double v = s[u];
            v += __shfl_xor(v, 4); v += __shfl_xor(v, 2); v += __shfl_xor(v, 1);
            if (sub == u0 + u) keep = v;
        }
    }
    return keep;
}

// the kernel variant by the number of modes, D % 4 and D <= 32, as launch_predict of k_predict.hip chooses it
#define BDF_BY_SHAPE(KERNEL, n_modes, D, nblocks, stream, args)                                                             \
    do {                                                                                                                     \
        const bool vec__ = ((D) & 3) == 0;                                                                                   \
        const int nc__ = (D) <= 32 ? 1 : 2;                                                                                  \
        if ((n_modes) == 2) {                                                                                                \
            if (!vec__) hipLaunchKernelGGL((KERNEL<2, 1, 1>), dim3(nblocks), dim3(256), 0, stream, args);                    \
            else if (nc__ == 1) hipLaunchKernelGGL((KERNEL<2, 4, 1>), dim3(nblocks), dim3(256), 0, stream, args);            \
            else hipLaunchKernelGGL((KERNEL<2, 4, 2>), dim3(nblocks), dim3(256), 0, stream, args);                           \
        } else if ((n_modes) == 3) {                                                                                         \
            if (!vec__) hipLaunchKernelGGL((KERNEL<3, 1, 1>), dim3(nblocks), dim3(256), 0, stream, args);                    \
            else if (nc__ == 1) hipLaunchKernelGGL((KERNEL<3, 4, 1>), dim3(nblocks), dim3(256), 0, stream, args);            \
            else hipLaunchKernelGGL((KERNEL<3, 4, 2>), dim3(nblocks), dim3(256), 0, stream, args);                           \
        } else {                                                                                                             \
            if (!vec__) hipLaunchKernelGGL((KERNEL<4, 1, 1>), dim3(nblocks), dim3(256), 0, stream, args);                    \
            else if (nc__ == 1) hipLaunchKernelGGL((KERNEL<4, 4, 1>), dim3(nblocks), dim3(256), 0, stream, args);            \
            else hipLaunchKernelGGL((KERNEL<4, 4, 2>), dim3(nblocks), dim3(256), 0, stream, args);                           \
        }                                                                                                                    \
    } while (0)

}  // namespace
