// nonneg.h -- the scalar map of the non-negative prior of an entity's rows: from a uniform to one
// coordinate of a row, a normal truncated to [0, inf).  Plain C++ (no HIP types) on the inverse normal CDF of probit.h: the same
// text compiles for the device and for a host check.
#pragma once
#include "probit.h"

#define BDF_NONNEG_TAIL (-37.0)        // t = m sqrt(lambda) below which Phi(t) is about to leave the double range (it does at -37.5)

// u ~ N(m, 1 / lambda) truncated to u >= 0, by inversion from U in (0, 1].  With s = sqrt(lambda) and t = m s, x = (u - m) s is a
// standard normal truncated to x > -t.
// t >= -37: the two branches of bdf_censored_z at bound 0 (either argument of Phi^-1 is at most 1/2), with Phi(t) and Phi(-t)
// from ONE erfc: q = erfc(|t| / sqrt 2) / 2 <= 1/2 is the smaller of the two, and 1 - q the other, exact to rounding.
// t < -37: the leading term of the tail, P(x > a + e | x > a) ~ exp(-a e - e^2 / 2) with a = -t, solved for e without the
// cancellation: y = sqrt(t^2 - 2 log U), e = -2 log U / (y - t); within 1 / t^2 relative of the exact excess over the bound.
// The result is finite and >= 0 whatever the rounding; U = 1 gives the bound's side of the law's support.
BDF_HD inline double bdf_nonneg(double m, double lambda, double U)
{
    const double s = sqrt(lambda), t = m * s;
    if (t < BDF_NONNEG_TAIL) {
        const double L = -2.0 * log(U);
        const double y = sqrt(t * t + L);
        return fmax(L / ((y - t) * s), 0.0);
    }
    const double q = 0.5 * erfc(fabs(t) / 1.4142135623730951);
    const double Pt = t >= 0.0 ? 1.0 - q : q, Pmt = t >= 0.0 ? q : 1.0 - q;      // Phi(t), Phi(-t)
    const double lo = Pmt + U * Pt;
    const double x = lo < 0.5 ? bdf_phi_inv(fmax(lo, DBL_MIN)) : -bdf_phi_inv(fmax((1.0 - U) * Pt, DBL_MIN));
    return fmax(m + x / s, 0.0);
}
