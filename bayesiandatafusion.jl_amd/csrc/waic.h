// waic.h -- the per-cell running state of WAIC on the training cells and the step that folds one posterior
// draw's log-likelihood into it.  Plain C++ on lpd.h's attributes: the same text compiles for the device (k_waic.hip) and for a
// host check (tests/test_waic_host.py).
#pragma once
#include "lpd.h"

#define BDF_WAIC_HIGH 0.4          // a cell whose V exceeds this is counted: WAIC is known to be unreliable for it

// the streaming log-sum-exp (M the largest l so far, A = sum exp(l - M)) exactly as k_lpd keeps it, and Welford's mean and M2 of l
struct bdf_waic_cell {
    double M, A, mu, M2;
};

// the first posterior draw
BDF_HD_FORCE inline void bdf_waic_start(double l, bdf_waic_cell &c)
{
    c.M = l; c.A = 1.0; c.mu = l; c.M2 = 0.0;
}

// l is the draws-th draw (draws >= 2, log_draws its logarithm): folds it in and gives lppd = M + log A - log(draws) and
// V = M2 / (draws - 1).  Equal draws leave d = 0 and so V = 0 exactly.
BDF_HD_FORCE inline void bdf_waic_fold(double l, double draws, double log_draws, bdf_waic_cell &c, double &lppd, double &V)
{
    const double Mn = fmax(c.M, l);
    c.A = c.A * exp(c.M - Mn) + exp(l - Mn);
    c.M = Mn;
    lppd = Mn + log(c.A) - log_draws;
    const double d = l - c.mu;
    c.mu += d / draws;
    c.M2 += d * (l - c.mu);
    V = c.M2 / (draws - 1.0);
}
