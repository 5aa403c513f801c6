// vb.h -- what bdf_vb.hip (host preparation, C ABI) and k_vb.hip (kernels) share: variational BPMF (src/macau_vb.jl).
#pragma once
#include "bdf_common.h"

// A row of a VB model on the device is one RECORD of rs doubles: its second moment Euu as a packed upper triangle (element
// (i, j), i <= j, at j (j + 1) / 2 + i; T = D (D + 1) / 2 doubles), then its mean mu (D doubles), then zeros up to a whole
// number of 128-byte lines.  The row update gathers the records of a row's neighbours and needs nothing else of them.
__host__ __device__ inline int vb_tri(int D) { return D * (D + 1) / 2; }
__host__ __device__ inline int vb_record(int D) { return (vb_tri(D) + D + 15) / 16 * 16; }

struct VBRowArgs {
    int D, T, RS, PW;              // T = vb_tri(D), RS = vb_record(D), PW = T + D + 1 (partial sums per block)
    int64_t N;                     // rows of the entity updated
    const int32_t *order;          // N: rows by descending number of neighbours (block b takes positions b G .. b G + G - 1)
    const int64_t *rowptr;         // N + 1
    const int32_t *colidx;         // the neighbours (0-based rows of the other entity), ascending within a row
    const double *vals;            // their values, centred and duplicates summed (the reference's sparse(...))
    const double *rec_other;       // the other entity's records (read)
    double *rec_out;               // this entity's records (written)
    double *mu_out;                // this entity's means again, D x N (for the prediction kernels)
    const double *pack;            // A = nu_N W_N (D x D column-major), then b = A mu_N (D)
    double alpha;
    double *partial;               // per block: sum of the block's packed Euu (T), of its mu (D), of |mu|^2 (1)
    int *flag;
};

struct VBPriorArgs {
    int D, T, PW;
    int64_t nblocks;               // blocks of the row launch whose partial sums are reduced
    const double *partial;
    double *slices;                // VB_SLICES x PW
    double nu_N, b_N, b_0;
    const double *mu0, *Winv0;     // D, D x D
    double *W_N, *mu_N, *pack;     // outputs: D x D, D, pack as VBRowArgs::pack
    double *normsq;                // 1 double: |mu_u|^2 of the entity
    int *flag;
};
#define VB_SLICES 32

int vb_row_blocks(int D, int64_t N);      // blocks (and partial rows) of a row launch
int vb_launch_rows(hipStream_t s, const VBRowArgs &a);
int vb_launch_prior(hipStream_t s, const VBPriorArgs &a);
