// newrows.h -- predictions for rows that were not in training (setNewRows / setNewTest): the per-cell running
// state and the step that folds one posterior draw into it.  Given one draw (mu, Lambda, beta, V, alpha) the factor of a new row with
// features f is u* ~ N(uhat, Lambda^-1), uhat = mu + beta' f, and it is integrated out of the cell (i*, j) in closed form:
//   identity link:  y | draw ~ N(m, q_j + 1 / alpha),          m = mean + uhat . v_j,   q_j = v_j' Lambda^-1 v_j
//   probit link:    P(y = 1 | draw) = Phi(m / sqrt(1 + q_j))   (the latent's unit noise and the new row's Gaussian add)
// Plain C++ on lpd.h's attributes: the same text compiles for the device (k_newrows.hip) and for a host check.
#pragma once
#include "lpd.h"

#define BDF_NEWROWS_TILE 64        // rows of V a workgroup of bdf_newrows_quad's kernel takes: four waves, 16 rows each
#define BDF_NEWROWS_STATS 8        // doubles of bdf_newrows_update's stats_out
#define BDF_NEWROWS_PLANES 5       // planes of n doubles of the running state: mean, M2, sum q, M, A

// Welford's (mean, M2) of the prediction p, the running sum of q, and the streaming log-sum-exp (M, A) of the log-likelihood
struct bdf_newrows_cell {
    double mean, M2, sq, M, A;
};

// this draw's prediction and, for a cell with a value, its log-likelihood (l is left alone without one)
BDF_HD_FORCE inline double bdf_newrows_predict(int link, double m, double q) { return link == 1 ? bdf_phi(m / sqrt(1.0 + q)) : m; }

BDF_HD_FORCE inline double bdf_newrows_loglik(int link, double y, double m, double q, double alpha)
{
    if (link == 1) return bdf_lpd_probit(y, m / sqrt(1.0 + q));
    return bdf_lpd_gauss(y, m, 1.0 / (q + 1.0 / alpha));
}

// the first posterior draw; scored: the cell has a value and the log-likelihood l is kept
BDF_HD_FORCE inline void bdf_newrows_start(double p, double q, bool scored, double l, bdf_newrows_cell &c)
{
    c.mean = p; c.M2 = 0.0; c.sq = q;
    c.M = scored ? l : 0.0; c.A = scored ? 1.0 : 0.0;
}

// (p, q, l) is the draws-th draw (draws >= 2): folds it in; returns lpd = M + log A - log(draws) of a scored cell (else l unchanged)
BDF_HD_FORCE inline double bdf_newrows_fold(double p, double q, bool scored, double l, double draws, double log_draws, bdf_newrows_cell &c)
{
    const double d = p - c.mean;
    c.mean += d / draws;
    c.M2 += d * (p - c.mean);
    c.sq += q;
    if (!scored) return l;
    const double Mn = fmax(c.M, l);
    c.A = c.A * exp(c.M - Mn) + exp(l - Mn);
    c.M = Mn;
    return Mn + log(c.A) - log_draws;
}

// the posterior sd of the cell's noise-free value (identity link: the spread of m over the draws plus the mean of q) or of its
// probability (probit); NaN below two draws
BDF_HD_FORCE inline double bdf_newrows_stdev(int link, double M2, double sq, double draws)
{
    if (draws < 2.0) return NAN;
    return sqrt(M2 / (draws - 1.0) + (link == 1 ? 0.0 : sq / draws));
}

// ---- one cell's step of one draw --------------------------------------------------------------------------------------------------
// What bdf_newrows_update and bdf_newrows_update_cells share: the first gathers (m, q) of a cold row from uhat, V and q_j, the second
// reads them from per-cell planes (a new row conditioned on cells of its own: k_foldin.hip).  From there on
// the two are this one text.
struct bdf_newrows_draw {
    int link, phase, score;        // phase 0: statistics only, 1: start the running state, 2: fold into it
    double draws, log_draws;       // phase 2: the draws the state holds after this one, and their logarithm
    double clamp_lo, clamp_hi, cut;
};

struct bdf_newrows_planes {
    double *mean, *M2, *sq, *M, *A;        // the running state, storage order
};

BDF_HD_FORCE inline double bdf_newrows_clamp(double x, double lo, double hi)
{
    if (lo > hi) return x;
    return x < lo ? lo : (x > hi ? hi : x);
}

// the cell stored at pm, with value y (NaN: predicted, left out of every scalar): the link, the fold into the state and the cell's
// eight statistics into st (zero on entry)
BDF_HD_FORCE inline void bdf_newrows_step(const bdf_newrows_draw &w, const bdf_newrows_planes &pl, long long pm, double y, double m, double q,
                                          double alpha, double (&st)[BDF_NEWROWS_STATS])
{
    const bool has = y == y;
    const bool scored = has && w.score != 0;
    const double p = bdf_newrows_predict(w.link, m, q);
    double l = 0.0;
    if (scored) l = bdf_newrows_loglik(w.link, y, m, q, alpha);
    double avg = p, lpd = l;
    if (w.phase >= 1) {
        bdf_newrows_cell c;
        if (w.phase == 1) bdf_newrows_start(p, q, scored, l, c);
        else {
            c.mean = pl.mean[pm]; c.M2 = pl.M2[pm]; c.sq = pl.sq[pm]; c.M = pl.M[pm]; c.A = pl.A[pm];
            lpd = bdf_newrows_fold(p, q, scored, l, w.draws, w.log_draws, c);
        }
        pl.mean[pm] = c.mean; pl.M2[pm] = c.M2; pl.sq[pm] = c.sq; pl.M[pm] = c.M; pl.A[pm] = c.A;
        avg = c.mean;
    }
    if (has) {
        const double ea = y - bdf_newrows_clamp(avg, w.clamp_lo, w.clamp_hi), ep = y - bdf_newrows_clamp(p, w.clamp_lo, w.clamp_hi);
        const bool label = y < w.cut;
        st[0] = ea * ea; st[1] = ep * ep;
        st[2] = (label == (avg < w.cut)) ? 1.0 : 0.0;
        st[3] = (label == (p < w.cut)) ? 1.0 : 0.0;
        st[4] = 1.0;
        if (scored) { st[5] = lpd; st[6] = l; }
    }
}
