// acquire.h -- what the host and the device share of the acquisition lists (setAcquire): the rules, the score
// of a cell from its moments over the draws and the tile of the moment planes.  Plain C++ (no HIP types): the same text compiles
// for the device and for a host check.
#pragma once
#include "recommend.h"

// k_acquire_accum: a workgroup of four waves owns BDF_ACQ_TN x BDF_ACQ_TM cells of the planes, a wave BDF_ACQ_WN x BDF_ACQ_WM of
// them: 2 x 2 blocks of v_mfma_f64_16x16x4_f64.  Per lane the product and the three planes are 4 x 16 doubles = 128 registers
// beside 4 operand doubles per step of four d: half of k_scores_accum's wave tile, so that mean, M2 and psum fit beside the product
#define BDF_ACQ_TN 64
#define BDF_ACQ_TM 64
#define BDF_ACQ_WN 32
#define BDF_ACQ_WM 32

// the rules of a list
#define BDF_ACQ_UCB 0      // m + kappa sd
#define BDF_ACQ_SD 1       // sd
#define BDF_ACQ_PROB 2     // the posterior probability that a measurement exceeds the threshold
// the planes bdf_acquire_copy addresses
#define BDF_ACQ_MEAN 0     // the running mean of u.v over the draws
#define BDF_ACQ_M2 1       // the running sum of squared deviations from it (Welford)
#define BDF_ACQ_PSUM 2     // the sum over the draws of Phi(sqrt(alpha_b) (u.v + mean_value - threshold))
#define BDF_ACQ_SCORE 3    // what the last bdf_acquire_topk ranked

// one draw's product p into a cell's moments; n: the count of draws with this one (1, 2, ...)
BDF_HD inline void bdf_acq_fold(double p, double n, double &mean, double &M2)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double delta = p - mean;
    mean += delta / n;
    M2 += delta * (p - mean);
}

// the term of one draw in psum: Phi(sqrt(alpha) (p + mean_value - threshold)), the noise integrated out of [measurement > threshold]
BDF_HD inline double bdf_acq_prob(double p, double root_alpha, double mean_value, double threshold)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return bdf_phi(root_alpha * (p + mean_value - threshold));
}

// the sample standard deviation of u.v over n draws, NaN with fewer than two
BDF_HD inline double bdf_acq_sd(double M2, double n) { return n >= 2.0 ? sqrt(M2 / (n - 1.0)) : __builtin_nan(""); }

// the acquisition score of a cell from its moments over n draws: this expression, on the host and on the device.  NaN (no
// candidate) with fewer than two draws for ucb and sd, with none for prob_above.  kappa sd is rounded before m is added
BDF_HD inline double bdf_acq_score(int rule, double mean, double M2, double psum, double n, double kappa, double mean_value)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (rule == BDF_ACQ_PROB) return n >= 1.0 ? psum / n : __builtin_nan("");
    const double sd = bdf_acq_sd(M2, n);
    if (rule == BDF_ACQ_SD) return sd;
    const double m = mean + mean_value;
    const double spread = kappa * sd;
    return spread + m;
}
