// dpp_rows32.h -- a 32 x 32 (or smaller) symmetric positive-definite system per ROW OF 16 LANES, four systems per wavefront:
// lane j of a lane row holds COLUMNS j and 16 + j of the system in full (A0[i] = entry (i, j), A1[i] = entry (i, 16 + j); entry 32 of
// each: the right-hand side) -- the unfinished part stays symmetric, so the multiplier of a column in step k is the lane's own
// entry of row k: no transposition, no LDS.  The LDL' factorisation with the forward solve riding along as row 32 and the
// backward solve are v_fmac_f64_dpp row_newbcast instructions (lane k % 16 of each lane row is the source of step k).  Used by
// k_rows_col (k_rows_col.hip: K1c, four rows per wave from the first observation on; its accumulation: col_rank1u, the ten unique
// 8 x 8 blocks) and k_rows_lr32 (k_rows_lr.hip: col_rank1, the three 16 x 16 blocks).
#pragma once
#include "dpp_rows16.h"

namespace {

// offset (doubles) in a partial slot / in the prior's image of element (i, 16 s + j) of the reversed system, DP = 32:
// blocks (0,0), (1,0), (1,1) in the accumulator layout -- lane (jj, hh), register r of block (I, J) is element
// (16 I + hh + 4 r, 16 J + jj) at [(blk * 4 + r) * 64 + 16 hh + jj]; the block above the diagonal is read from its mirror image
template <int S, int I>
__device__ __forceinline__ int sys_off(int j)
{
    constexpr int IB = I / 16, ii = I % 16;
    if constexpr (IB >= S) {
        constexpr int blk = IB * (IB + 1) / 2 + S;
        return (blk * 4 + (ii >> 2)) * 64 + 16 * (ii & 3) + j;
    } else {
        return (1 * 4 + (j >> 2)) * 64 + 16 * (j & 3) + ii;       // element (16 + j, i) of block (1, 0)
    }
}

// ---- a rank-1 update v v' of the three stored blocks (0,0), (1,0), (1,1): lane j holds v0 = v_j and v1 = v_(16+j) (k_rows_lr32: an element of
// the two observations a lane streams; k_rows_col's observations take col_rank1u below) ----
template <int DR, int I>
__device__ __forceinline__ void col_rank1(double (&A0)[33], double (&A1)[33], double v0, double v1)
{
    if constexpr (I < 16) {
        if constexpr (I == 0) fm1<0>(A0[0], v0, v0); else fm1_run<I>(A0[I], v0, v0);      // (i, j)      += v_i v_j
        if constexpr (16 + I < DR) {
            fm1_run<I>(A0[16 + I], v1, v0);                                               // (16+i, j)   += v_(16+i) v_j
            fm1_run<I>(A1[16 + I], v1, v1);                                               // (16+i,16+j) += v_(16+i) v_(16+j)
        }
        col_rank1<DR, I + 1>(A0, A1, v0, v1);
    }
}
// ---- the same rank-1 update as the TEN UNIQUE 8 x 8 BLOCKS of the symmetric 32 x 32 (k_rows_col): 40 fmacs where col_rank1 spends 48 --
// its two diagonal 16 x 16 blocks compute (i, j) and (j, i) both.  The 32 elements in four groups of eight (L: lanes 0-7, H: lanes 8-15 of
// v0 | v1), every unordered pair of groups in ONE orientation; a row_newbcast fmac is one element times sixteen, so the eight rows of a
// group meet TWO groups per instruction, and two derived own-vectors put the right pair under them:
//     x = L ? v1 : v0          [v_16..23 | v_8..15]        two v_cndmask_b32
//     y = L ? rot8(v0) : v1    [v_8..15  | v_24..31]       two v_cndmask_b32_dpp row_ror:8 (v_fmac_f64_dpp itself takes no row_ror)
//   A0[i]      += v0[i]   v0     (i, j)            P0: the column's entries as they are
//   A1[i]      += v0[i]   v1     (i, 16+j)         P1: block (0,1) itself (col_rank1 accumulates its mirror image)
//   A0[8+i]    += v0[8+i] x      M1: L (8+i, 16+j) -- A1[8+i]'s L half;  H (8+i, j) -- A0[8+i]'s own H half
//   A1[16+i]   += v1[i]   v1     (16+i, 16+j)      P2
//   A1[24+i]   += v1[8+i] y      M3: L (24+i, 8+j) -- A0[24+i]'s H half, eight lanes to the left;  H (24+i, 16+j) -- A1[24+i]'s own H half
// for i = 0 .. 7; rows DR .. 31 are skipped (P2 from DR < 24, M3 and y at DR <= 24).  Every accumulator sees the fma(acc, a, b) of col_rank1's
// entry with a and b in this or the other order: the same bits.  What the sixty-four natural registers still miss is their mirror image in
// another lane (k_rows_col's re-layout, once per round).
template <int B0, int K0, int N, int I = 0>
__device__ __forceinline__ void col_star(double (&A)[33], double s, double m)
{
    if constexpr (I < N) {
        fm1_run<K0 + I>(A[B0 + I], s, m);
        col_star<B0, K0, N, I + 1>(A, s, m);
    }
}
// hmask: the H lanes of the four lane rows (the DPP form of the select takes its condition from VCC only: a scalar move per observation)
__device__ __forceinline__ double col_own_y(double v0, double v1, uint64_t hmask)
{
    int lo, hi;
    asm("s_mov_b64 vcc, %6\n\t"
        "v_cndmask_b32_dpp %0, %2, %4, vcc row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
        "v_cndmask_b32_dpp %1, %3, %5, vcc row_ror:8 row_mask:0xf bank_mask:0xf"
        : "=&v"(lo), "=v"(hi) : "v"(__double2loint(v0)), "v"(__double2hiint(v0)), "v"(__double2loint(v1)), "v"(__double2hiint(v1)), "s"(hmask) : "vcc");
    return __hiloint2double(hi, lo);
}
template <int DR>
__device__ __forceinline__ void col_rank1u(double (&A0)[33], double (&A1)[33], double v0, double v1, bool h, uint64_t hmask)
{
    fm1<0>(A0[0], v0, v0);
    col_star<1, 1, 7>(A0, v0, v0);
    col_star<0, 0, 8>(A1, v0, v1);
    col_star<16, 0, (DR - 16 < 8 ? DR - 16 : 8)>(A1, v1, v1);
    const double x = h ? v0 : v1;
    col_star<8, 8, 8>(A0, v0, x);
    if constexpr (DR > 24) {
        const double y = col_own_y(v0, v1, hmask);
        col_star<24, 8, DR - 24>(A1, v1, y);
    }
}
// the same with the two own-vectors given: K1c's gather image holds x and y beside v0 and v1 (k_gather_image.hip), made once by whoever
// wrote the row instead of once per observation -- the same fmas with the same operands, no select in the loop
__device__ __forceinline__ void col_rank1u(double (&A0)[33], double (&A1)[33], double v0, double v1, double x, double y)
{
    fm1<0>(A0[0], v0, v0);
    col_star<1, 1, 7>(A0, v0, v0);
    col_star<0, 0, 8>(A1, v0, v1);
    col_star<16, 0, 8>(A1, v1, v1);
    col_star<8, 8, 8>(A0, v0, x);
    col_star<24, 8, 8>(A1, v1, y);
}
// rows I .. DR-1 and the extra row 32 of step k = 16 S + K: A_s[I] -= A[I][k] * A[k][c_s] / d_k
template <int DR, int S, int K, int I, bool FIRST>
__device__ __forceinline__ void fin_elim(double (&A0)[33], double (&A1)[33], double nm0, double nm1)
{
    if constexpr (I <= 32) {
        if constexpr (S == 0) {
            if constexpr (DR > 16) {
                if constexpr (FIRST) fm1<K>(A1[I], A0[I], nm1); else fm1_run<K>(A1[I], A0[I], nm1);
                fm1_self_run<K>(A0[I], nm0);
            } else {
                if constexpr (FIRST) fm1_self<K>(A0[I], nm0); else fm1_self_run<K>(A0[I], nm0);
            }
        } else {
            if constexpr (FIRST) fm1_self<K>(A1[I], nm1); else fm1_self_run<K>(A1[I], nm1);
        }
        fin_elim<DR, S, K, (I + 1 < DR || I == 32) ? I + 1 : 32, false>(A0, A1, nm0, nm1);
    }
}

template <int DR, int k>
__device__ __forceinline__ void fin_factor(double (&A0)[33], double (&A1)[33], double &d0, double &d1, int j)
{
    if constexpr (k < DR) {
        constexpr int S = k / 16, K = k % 16;
        const double dk = row_bcast_f64<K>(S ? A1[k] : A0[k]);
        const double rinv = fast_rcp(dk);
        double nm0 = 0.0, nm1;
        if constexpr (S == 0) {
            d0 = (j == K) ? dk : d0;
            nm0 = (j > K) ? -(A0[k] * rinv) : 0.0;             // finished columns are left alone
            nm1 = -(A1[k] * rinv);
        } else {
            d1 = (j == K) ? dk : d1;
            nm1 = (j > K) ? -(A1[k] * rinv) : 0.0;
        }
        fin_elim<DR, S, K, (k + 1 < DR) ? k + 1 : 32, true>(A0, A1, nm0, nm1);
        fin_factor<DR, k + 1>(A0, A1, d0, d1, j);
    }
}

// y_c -= l_Cc x_C for the columns left of C, C = DR-1 .. 1 (x_C is final in lane C % 16 when its turn comes)
template <int C>
__device__ __forceinline__ void fin_backward(const double (&A0)[33], const double (&A1)[33], double &y0, double &y1, double rd0,
                                             double rd1, int j)
{
    if constexpr (C >= 1) {
        constexpr int S = C / 16, K = C % 16;
        if constexpr (S == 1) {
            fm1<K>(y0, y1, -(A0[C] * rd0));
            if constexpr (K > 0) fm1_self_run<K>(y1, (j < K) ? -(A1[C] * rd1) : 0.0);
        } else {
            fm1_self<K>(y0, (j < K) ? -(A0[C] * rd0) : 0.0);
        }
        fin_backward<C - 1>(A0, A1, y0, y1, rd0, rd1, j);
    }
}

}  // namespace
