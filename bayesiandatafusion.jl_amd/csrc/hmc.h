// hmc.h -- what bdf_hmc.hip (host preparation, C ABI) and k_hmc.hip (kernels) share: Hamiltonian Monte Carlo BPMF
// (src/macau_hmc.jl).
#pragma once
#include "bdf_common.h"

// Per-block partial sums of a leapfrog launch (HMC_PW doubles per block, fixed order):
#define HMC_MSQ     0    // |momentum|^2 of the entity after the launch
#define HMC_USQ     1    // |sample|^2 after the launch
#define HMC_KIN_S   2    // sum (r^2 G + log G) at the start point (HMC_DRAW launches)
#define HMC_PRI_S   3    // sum u'(Lambda u / 2 - Lambda mu) at the start point
#define HMC_DAT_S   4    // sum over the observations of (u.v - val)^2 at the start point (HMC_DATA launches)
#define HMC_KIN_F   5    // the same three at the final point (HMC_FINAL launches)
#define HMC_PRI_F   6
#define HMC_DAT_F   7
#define HMC_USQ_S   8    // |sample|^2 at the start point
#define HMC_PW      9

// launch flags
#define HMC_DRAW    1    // first launch of the entity in the iteration: draw the momentum, keep the start copy, start energies
#define HMC_FINAL   2    // last launch of the entity: final energies
#define HMC_DATA    4    // the rows are U's: the launch also sums the data term (over every observation)

// The iteration record (doubles) the accept kernel writes; then the momentum log from HMC_REC_LOG on: sqrt(HMC_MSQ) of every
// launch of the iteration, in launch order (U0, V1, U1, ..., VL, UL).
#define HMC_REC_I        0
#define HMC_REC_EPS      1
#define HMC_REC_L        2
#define HMC_REC_KIN_S    3
#define HMC_REC_KIN_F    4
#define HMC_REC_POT_S    5
#define HMC_REC_POT_F    6
#define HMC_REC_DH       7
#define HMC_REC_ACCEPT   8
#define HMC_REC_EPS_NEW  9
#define HMC_REC_L_NEW    10
#define HMC_REC_NORM_U   11
#define HMC_REC_NORM_V   12
#define HMC_REC_UNIFORM  13
#define HMC_REC_LOG      16

// the flag bit a non-finite energy raises (bdf_ctx_sync reports it)
#define HMC_FLAG_ENERGY  32

struct HMCLeapArgs {
    int D, L_inner, flags;
    uint32_t tag;                  // entity tag of the momentum stream: 0 (U) or 1 (V)
    int64_t N;                     // rows of the entity
    const int32_t *order;          // N: rows by descending number of neighbours
    const int64_t *rowptr;         // N + 1
    const int32_t *colidx;         // the neighbours (0-based rows of the other entity), ascending within a row
    const double *vals;            // the centred values, duplicates summed (the reference's sparse(...))
    const double *cs;              // per entry: multiplicity c and the sum of the squared centred values (2 doubles)
    const double *other;           // the other entity's sample, N_other x D row-major (fixed during the launch)
    double *sample, *mom, *start;  // this entity's sample, momentum (N x D row-major) and start copy
    const double *G;               // D: the diagonal mass (the same for every row: repmat(diag(Lambda), 1, N))
    const double *mu, *Lambda;     // D, D x D
    double alpha, eps;
    uint64_t seed;
    uint32_t sweep;
    double *partial;               // per block: HMC_PW doubles
};

struct HMCAcceptArgs {
    const double *partial;         // the iteration's launches one after another (launch s of entity s % 2 at slot_offset(s))
    int64_t nb[2];                 // blocks of a U and of a V launch
    int L;
    double eps, alpha;
    uint64_t seed;
    uint32_t sweep;
    double *rec;                   // the iteration record
    int *flag;
};

struct HMCRestoreArgs {
    int64_t n[2];                  // N_u D, N_v D
    double *sample[2];
    const double *start[2];
    const double *rec;
};

struct HMCPredictArgs {
    int D;
    int64_t n;
    const int32_t *ids;            // two planes of n, 0-based
    const double *values;
    const double *U, *V;
    double mean, lo, hi;           // lo > hi: no clamping
    int copy;                      // update_yhat_post!: 1 copies, 0 keeps the running mean of count samples
    double count;
    double *avg;
    double *partial;               // per block: sum (y - yhat)^2, sum (y - clamp(avg))^2
};

int64_t hmc_row_blocks(int D, int64_t N);
int hmc_launch_leap(hipStream_t s, const HMCLeapArgs &a);
int hmc_launch_accept(hipStream_t s, const HMCAcceptArgs &a);
int hmc_launch_restore(hipStream_t s, const HMCRestoreArgs &a);
int64_t hmc_predict_blocks(int64_t n);
int hmc_launch_predict(hipStream_t s, const HMCPredictArgs &a);
