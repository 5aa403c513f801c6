// recommend.h -- what the host and the device share of the top-K lists (setRecommend): the order of a list, the
// discount of a list position and the tile of the score sum.  Plain C++ (no HIP types): the same text compiles for the device and
// for a host check.
#pragma once
#include "probit.h"

// k_scores_accum: a workgroup of four waves owns BDF_REC_TN x BDF_REC_TM cells of the sum, a wave BDF_REC_WN x BDF_REC_WM of them:
// 2 x 4 blocks of v_mfma_f64_16x16x4_f64, 64 accumulator registers per lane beside 6 operand doubles per step of four d
#define BDF_REC_TN 64
#define BDF_REC_TM 128
#define BDF_REC_WN 32
#define BDF_REC_WM 64
#define BDF_REC_MAX_K 64
#define BDF_REC_MAX_BATCH 32
// k_topk_rows: the listed columns of a row are marked in LDS, this many columns of the row at a time
#define BDF_REC_WINDOW 65536
// doubles of NaN that bdf_scores_create leaves behind the sum and no kernel writes (bdf_scores_copy reads them: a test's canary)
#define BDF_REC_GUARD 64

// the order of a list: (score_a, item_a) stands before (score_b, item_b) -- the larger score, equal scores by the smaller item id.
// A strict total order on pairs with distinct items and scores that are numbers
BDF_HD inline bool bdf_rec_before(double score_a, int item_a, double score_b, int item_b)
{
    return score_a > score_b || (score_a == score_b && item_a < item_b);
}

// 1 / log2(r + 1), the discount of list position r = 1 .. 64 in DCG, as a table so that the host and the device hold the same bits
BDF_HD inline double bdf_rec_discount(int r)
{
    constexpr double t[BDF_REC_MAX_K] = {
        0x1.0000000000000p+0, 0x1.430939835353ep-1, 0x1.0000000000000p-1, 0x1.b903469050f73p-2,
        0x1.8c23246dc0aa0p-2, 0x1.6cc193acea9b5p-2, 0x1.5555555555555p-2, 0x1.430939835353ep-2,
        0x1.34413509f79ffp-2, 0x1.28009c1dd6454p-2, 0x1.1da3383416064p-2, 0x1.14b94f8d9641fp-2,
        0x1.0cf3ffed2d6acp-2, 0x1.0619dc46d3e15p-2, 0x1.0000000000000p-2, 0x1.f50b57eac5885p-3,
        0x1.eb22cc68aa6e3p-3, 0x1.e21e1180c5dabp-3, 0x1.d9dcd21439834p-3, 0x1.d244c78367a0dp-3,
        0x1.cb40589ac173ep-3, 0x1.c4bd95ba8d72bp-3, 0x1.bead76898f8cep-3, 0x1.b903469050f73p-3,
        0x1.b3b433f2eb070p-3, 0x1.aeb6f759c46fdp-3, 0x1.aa038eb0e3bfep-3, 0x1.a593062b38d8dp-3,
        0x1.a15f4c32b95a3p-3, 0x1.9d630dccc7ddfp-3, 0x1.999999999999ap-3, 0x1.95fec808a6094p-3,
        0x1.928ee7b0b4f23p-3, 0x1.8f46acf8c06e3p-3, 0x1.8c23246dc0aa0p-3, 0x1.8921a744e1aedp-3,
        0x1.863fd1a4a3053p-3, 0x1.837b7a642195ep-3, 0x1.80d2abffdfee9p-3, 0x1.7e439e8fed2b0p-3,
        0x1.7bccb2952736ep-3, 0x1.796c6c7b22305p-3, 0x1.772170b2747aap-3, 0x1.74ea804c2020fp-3,
        0x1.72c67602d3540p-3, 0x1.70b443a1f7c88p-3, 0x1.6eb2efbd2c1adp-3, 0x1.6cc193acea9b5p-3,
        0x1.6adf59c6e689dp-3, 0x1.690b7bca1f15ep-3, 0x1.67454177dda00p-3, 0x1.658bff53d6bf2p-3,
        0x1.63df15867d0dep-3, 0x1.623deedd496bap-3, 0x1.60a7ffe55458ap-3, 0x1.5f1cc61d1c5f1p-3,
        0x1.5d9bc73ac2288p-3, 0x1.5c2490845f2f3p-3, 0x1.5ab6b6386aaa4p-3, 0x1.5951d3046396fp-3,
        0x1.57f587883063fp-3, 0x1.56a179e4d652cp-3, 0x1.5555555555555p-3, 0x1.5410c9d09a12cp-3,
    };
    return t[r - 1];
}

// the score of a cell from its sum over the draws: this expression, on the host and on the device
BDF_HD inline double bdf_rec_score(double sum, double draws, double mean_value) { return sum / draws + mean_value; }
