// interval.h -- the scalar map of the interval-censored noise model: from a uniform to the latent value of
// one observation that is known only to lie between two bounds.  Plain C++ (no HIP types) on the normal CDF and its inverse of
// probit.h: the same text compiles for the device and for a host check.
#pragma once
#include "probit.h"

// z ~ N(m, 1 / alpha) truncated to [lo, hi] (lo < hi, either may be infinite), by inversion from u in (0, 1]; lo == hi: the
// measurement y itself.  With ra = sqrt(alpha), a = (lo - m) ra and b = (hi - m) ra, x = (z - m) ra is a standard normal
// truncated to [a, b].  An interval that lies more above 0 than below it (a + b > 0; false for the NaN of (-inf, +inf)) is
// reflected, (a, b, v, v', s) = (-b, -a, 1 - u, u, -1) for (a, b, u, 1 - u, +1), so that both Phi(a) and Phi(b) are taken in the
// lower tail, where they and their difference w are relatively accurate (in the upper tail Phi(b) - Phi(a) cancels to nothing
// beyond 8 standard deviations).  p = Phi(a) + v w is the CDF value of x; below the median x = Phi^-1(p), above it
// 1 - p = Phi(-b) + v' w is formed without the cancellation and x = -Phi^-1(1 - p): either argument of Phi^-1 is at most 1/2, as
// in bdf_probit_z.  v' is the complement of v taken from u itself, never 1 - (1 - u): 1 - u is rounded by up to 2^-54 when
// u < 1/2, which is harmless where it is used (there it is at least 1/2) but would be an error of 2^-54 w / phi(x) standard
// deviations in the far tail of a wide reflected interval (1e-5 at [-7.9, 8.1]).  x increases with u whether reflected or not.
// The last line keeps the draw inside the bounds whatever the rounding: with both bounds beyond 37.5 standard deviations on one
// side of m, where Phi underflows, it returns the nearer bound (the exact law there lies within about 1 / (37 ra) of it).
BDF_HD inline double bdf_interval_z(double m, double y, double lo, double hi, double alpha, double u)
{
    if (lo == hi) return y;
    const double ra = sqrt(alpha);
    double a = (lo - m) * ra, b = (hi - m) * ra, v = u, vc = 1.0 - u, s = 1.0;
    if (a + b > 0.0) {
        const double t = a;
        a = -b; b = -t; v = vc; vc = u; s = -1.0;
    }
    const double Pa = bdf_phi(a), w = bdf_phi(b) - Pa, p = Pa + v * w;
    const double x = p < 0.5 ? bdf_phi_inv(fmax(p, DBL_MIN)) : -bdf_phi_inv(fmax(bdf_phi(-b) + vc * w, DBL_MIN));
    return fmin(fmax(m + s * x / ra, lo), hi);
}
