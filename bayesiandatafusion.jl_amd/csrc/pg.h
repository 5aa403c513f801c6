// pg.h -- the scalar maps and the sampler of the Polya-Gamma noise models (Polson, Scott & Windle 2013): a cell
// with psi = udot + mean and likelihood (e^psi)^a / (1 + e^psi)^b is, given omega ~ PG(b, psi), a Gaussian pseudo-observation
// kappa / omega of psi with precision omega, kappa = a - b / 2.  Logit (model 1): b = 1, kappa = y - 1/2; negative-binomial counts
// with fixed dispersion r (model 2): b = y + r, kappa = (y - r) / 2.
//
// Plain C++ (no HIP types): the same text compiles for the device and for a host check.  The sampler is a template over the source
// of its random numbers, a cursor R with
//   double uniform();                    one block: its first double
//   double expo();                       one block: -log of its first double
//   void   expo2(double &E, double &F);  one block: -log of its first and of its second double
//   double normal();                     one block: sqrt(-2 log first) cos(2 pi second)
// so that the device (k_pg.hip: Philox blocks pair = 0, 1, 2, ... of the observation's stream) and a host program draw the same
// numbers.  Every loop is bounded (BDF_PG_TRIES); what it returns at the bound is said where it stands.
#pragma once
#include "lpd.h"

#define BDF_PG_T 0.64                 // Devroye's switch point between the two series of the J* density
#define BDF_PG_SUM_MAX 170.0          // b above it: the moment-matched normal (an approximation), as BayesLogit's hybrid sampler
#define BDF_PG_TRIES 256              // proposals per draw, and candidates per truncated inverse-Gaussian variate
#define BDF_PG_TERMS 64               // partial sums of the alternating series per proposal
#define BDF_PG_SERIES_BELOW 0.25      // |c| below it: the moments by their series
#define BDF_PG_PI 3.14159265358979323846

// ---- the models' maps --------------------------------------------------------------------------------------------------------------
// (the values are the caller's contract -- 0/1, or integers >= 0; b is held at 1 so that a stored value outside it, which only
// the bare C ABI lets through, still gives a finite, positive omega)
BDF_HD inline double bdf_pg_b(int model, double y, double r) { return model == 1 ? 1.0 : fmax(y + r, 1.0); }
BDF_HD inline double bdf_pg_kappa(int model, double y, double r) { return model == 1 ? y - 0.5 : 0.5 * (y - r); }
// what the row kernels take as the observation's base: y - base = kappa / omega - mean, the pseudo-observation of udot
BDF_HD inline double bdf_pg_linear(double mean, double y, double kappa, double omega) { return mean + (y - kappa / omega); }

// the logistic link, stable on both sides
BDF_HD inline double bdf_pg_logistic(double psi)
{
    if (psi >= 0.0) return 1.0 / (1.0 + exp(-psi));
    const double e = exp(psi);
    return e / (1.0 + e);
}
// the mean of the counts, r e^psi (finite: the exponent is held at 700)
BDF_HD inline double bdf_pg_count_mean(double psi, double r) { return r * exp(fmin(psi, 700.0)); }

// ---- the first two moments of PG(b, c), a = |c| ------------------------------------------------------------------------------------
// m = b / (2a) tanh(a / 2), v = b / (4 a^3) (sinh a - a) sech^2(a / 2); with e = e^-a: tanh(a / 2) = (1 - e) / (1 + e) and
// (sinh a - a) sech^2(a / 2) = 2 (1 - e^2 - 2 a e) / (1 + e)^2, which overflow nowhere.  Below BDF_PG_SERIES_BELOW, where
// 1 - e^2 - 2 a e cancels like a^3 / 3, tanh(x) / x (x = a / 2) and (sinh a - a) / a^3 = sum a^2k / (2k + 3)! by their series (the
// first terms left out are below 1e-17 of the sums).  At a = 0: m = b / 4, v = b / 24.
BDF_HD inline void bdf_pg_moments(double b, double a, double &m, double &v)
{
    const double e = exp(-a), d = (1.0 + e) * (1.0 + e);
    if (a < BDF_PG_SERIES_BELOW) {
        const double x2 = 0.25 * a * a, a2 = a * a;
        const double T = 1.0 + x2 * (-1.0 / 3.0 + x2 * (2.0 / 15.0 + x2 * (-17.0 / 315.0 + x2 * (62.0 / 2835.0 + x2 * (-1382.0 / 155925.0 +
                         x2 * (21844.0 / 6081075.0 + x2 * (-929569.0 / 638512875.0)))))));
        const double G = 1.0 / 6.0 + a2 * (1.0 / 120.0 + a2 * (1.0 / 5040.0 + a2 * (1.0 / 362880.0 + a2 * (1.0 / 39916800.0 +
                         a2 * (1.0 / 6227020800.0 + a2 * (1.0 / 1307674368000.0))))));
        m = 0.25 * b * T;
        v = b * G * e / d;                                 // b / 4 G sech^2(a / 2), sech^2(a / 2) = 4 e / (1 + e)^2
        return;
    }
    m = b / (2.0 * a) * ((1.0 - e) / (1.0 + e));
    v = b / (2.0 * a * a * a) * (((1.0 - e) * (1.0 + e) - 2.0 * a * e) / d);
}

// ---- J*(1, z) by Devroye's method ----------------------------------------------------------------------------------------------------
// the coefficients of the alternating series of the density, on either side of t
BDF_HD_FORCE inline double bdf_pg_coef(int n, double x)
{
    const double h = n + 0.5, k = BDF_PG_PI * h;
    if (x <= BDF_PG_T) {
        const double w = 2.0 / (BDF_PG_PI * x);
        return k * (w * sqrt(w)) * exp(-2.0 * h * h / x);
    }
    return k * exp(-0.5 * k * k * x);
}

// what a draw at tilt z shares between its b variates: K and the masses p (the exponential tail beyond t) and q (the truncated
// inverse Gaussian below it) of the proposal.  e^2z is never formed on its own: the left tail's log Phi takes it.
struct bdf_pg_tilt {
    double z, K, p, q;
};

BDF_HD_FORCE inline bdf_pg_tilt bdf_pg_tilt_of(double z)
{
    const double t = BDF_PG_T, st = 0.8;                   // sqrt(t)
    bdf_pg_tilt w;
    w.z = z;
    w.K = BDF_PG_PI * BDF_PG_PI / 8.0 + 0.5 * z * z;
    w.p = BDF_PG_PI / (2.0 * w.K) * exp(-w.K * t);
    w.q = 2.0 * exp(-z) * (bdf_phi((t * z - 1.0) / st) + exp(2.0 * z + bdf_log_phi(-(t * z + 1.0) / st)));
    return w;
}

// X ~ J*(1, z).  A proposal: with probability p / (p + q) -- decided as u (p + q) < p, so that an underflowed p or q gives no 0/0 --
// X = t + E / K; else X ~ IG(1 / z, 1) truncated to (0, t]: for 1 / z > t candidates t / (1 + t E)^2 with E^2 <= 2 E' / t, accepted
// with probability e^(-z^2 X / 2); else candidates of the inverse Gaussian itself until one is at most t.  Then the alternating
// series decides.  At the bound of the candidates the last one stands (held at t); after BDF_PG_TERMS partial sums a proposal is
// accepted; after BDF_PG_TRIES refused proposals the last one is returned.
template <class R>
BDF_HD_FORCE inline double bdf_pg_jstar(const bdf_pg_tilt &w, R &rng)
{
    const double t = BDF_PG_T, z = w.z;
    double X = t;
    for (int prop = 0; prop < BDF_PG_TRIES; prop++) {
        const double u = rng.uniform();
        if (u * (w.p + w.q) < w.p) {
            X = t + rng.expo() / w.K;
        } else if (t * z < 1.0) {
            for (int c = 0; c < BDF_PG_TRIES; c++) {
                double E, F;
                rng.expo2(E, F);
                if (E * E > 2.0 * F / t) continue;
                const double g = 1.0 + t * E;
                X = t / (g * g);
                if (rng.uniform() <= exp(-0.5 * z * z * X)) break;
            }
        } else {
            const double mu = 1.0 / z;
            for (int c = 0; c < BDF_PG_TRIES; c++) {
                const double N = rng.normal(), Y = N * N;
                X = mu + 0.5 * mu * mu * Y - 0.5 * mu * sqrt(4.0 * mu * Y + (mu * Y) * (mu * Y));
                if (rng.uniform() > mu / (mu + X)) X = mu * mu / X;
                if (X <= t) break;
            }
            X = fmin(X, t);
        }
        double S = bdf_pg_coef(0, X);
        const double y = rng.uniform() * S;
        bool accept = true;
        for (int n = 1; n < BDF_PG_TERMS; n++) {
            if (n & 1) {
                S -= bdf_pg_coef(n, X);
                if (y <= S) break;
            } else {
                S += bdf_pg_coef(n, X);
                if (y > S) { accept = false; break; }
            }
        }
        if (accept) return X;
    }
    return X;
}

// omega ~ PG(b, c), b a positive integer held in a double.  b <= 170: the sum of b variates J*(1, |c| / 2) / 4, exact.  Above: the
// normal with PG(b, c)'s mean and variance (one normal), an approximation.  Finite and strictly positive for every finite c.
template <class R>
BDF_HD_FORCE inline double bdf_pg_omega(double b, double c, R &rng)
{
    const double a = fabs(c);
    if (b > BDF_PG_SUM_MAX) {
        double m, v;
        bdf_pg_moments(b, a, m, v);
        return fmax(m + sqrt(v) * rng.normal(), DBL_MIN);
    }
    const bdf_pg_tilt w = bdf_pg_tilt_of(0.5 * a);
    double s = 0.0;
    const int nb = (int)b;
    for (int i = 0; i < nb; i++) s += bdf_pg_jstar(w, rng);
    return fmax(0.25 * s, DBL_MIN);
}
