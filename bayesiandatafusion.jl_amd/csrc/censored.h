// censored.h -- the scalar map of the censored (Tobit) noise model: from a uniform to the latent value of
// one observation that is a bound, not a measurement.  Plain C++ (no HIP types) on the normal CDF and its inverse of probit.h:
// the same text compiles for the device and for a host check.
#pragma once
#include "probit.h"

// z ~ N(m, 1 / alpha) truncated to z >= y (c = +1, right-censored) or z <= y (c = -1, left-censored), by inversion from u in
// (0, 1]; c = 0: the measurement itself.  With s = c, ra = sqrt(alpha) and t = s (m - y) ra, x = s (z - m) ra is a standard
// normal truncated to x > -t: the two branches of bdf_probit_z, for the same reason (either argument of Phi^-1 is at most 1/2).
// The last line keeps the draw on the bound's side whatever the rounding: for t < -37.5, where Phi(t) underflows, it returns a
// draw at or near the bound (the exact law there lies within about 1 / (37 ra) of it).
BDF_HD inline double bdf_censored_z(double m, double y, int c, double alpha, double u)
{
    if (c == 0) return y;
    const double s = c > 0 ? 1.0 : -1.0, ra = sqrt(alpha), t = s * (m - y) * ra;
    const double Pt = bdf_phi(t);
    const double lo = bdf_phi(-t) + u * Pt;
    const double x = lo < 0.5 ? bdf_phi_inv(fmax(lo, DBL_MIN)) : -bdf_phi_inv(fmax((1.0 - u) * Pt, DBL_MIN));
    const double z = m + s * x / ra;
    return y + s * fmax(s * (z - y), 0.0);
}
