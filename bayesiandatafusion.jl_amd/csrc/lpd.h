// lpd.h -- the scalar maps of the held-out log predictive density: the log-likelihood of one test cell
// given the rows of one posterior draw, for each kind of record the noise models know -- a measurement (Gaussian density), a 0/1
// value (probit) and a value known only to lie between two bounds (the mass of the interval).  Plain C++ (no HIP types) on the
// normal CDF of probit.h: the same text compiles for the device and for a host check.
#pragma once
#include "probit.h"
// (forced: left to its own judgement the device compiler calls the interval's map out of line, which costs the kernel a stack)
#define BDF_HD_FORCE BDF_HD __attribute__((always_inline))

// log of the series 1 - 1/x^2 + 3/x^4 - 15/x^6 + ... + 2027025/x^16 of the normal tail's asymptotic expansion (eight terms behind
// the 1; the first one left out is 3.4e7 / x^18: 2e-21 at |x| = 37)
BDF_HD_FORCE inline double bdf_log_tail_series(double x)
{
    const double r = 1.0 / (x * x);
    return log1p(r * (-1.0 + r * (3.0 + r * (-15.0 + r * (105.0 + r * (-945.0 + r * (10395.0 + r * (-135135.0 + r * 2027025.0))))))));
}

// log Phi(x).  Above 0 through the upper tail, log1p(-Phi(-x)); below, log(Phi(x)) while Phi is a normal double, and from 37
// standard deviations down the asymptotic form -x^2/2 - log(-x) - log(2 pi)/2 + log(series): Phi itself is denormal beyond -37.5
// and zero beyond -38.5, where its logarithm would lose every digit and then be -inf.
BDF_HD_FORCE inline double bdf_log_phi(double x)
{
    if (x >= 0.0) return log1p(-bdf_phi(-x));
    if (x > -37.0) return log(bdf_phi(x));
    return -0.5 * x * x - log(-x) - 0.91893853320467274178 + bdf_log_tail_series(x);
}

// a measurement y of N(m, 1 / alpha): the log density
BDF_HD_FORCE inline double bdf_lpd_gauss(double y, double m, double alpha)
{
    const double e = y - m;
    return 0.5 * log(alpha / 6.283185307179586476925286766559) - 0.5 * alpha * (e * e);
}

// a 0/1 value of the probit model: log P(y | m) = log Phi(+-m)
BDF_HD_FORCE inline double bdf_lpd_probit(double y, double m) { return bdf_log_phi(y > 0.5 ? m : -m); }

// a value of N(m, 1 / alpha) known to lie in [lo, hi] (lo < hi, either may be infinite): log(Phi(b) - Phi(a)) with
// a = (lo - m) sqrt(alpha), b = (hi - m) sqrt(alpha).  Reflected as bdf_interval_z reflects (a + b > 0, false for the NaN of
// (-inf, +inf)) so that both CDF values are lower-tail ones, where their difference is relatively accurate.  While Phi(b) is a
// normal double the difference is formed directly; below that from the logarithms, log Phi(b) + log(1 - exp(La - Lb)), where both
// are on the asymptotic branch and La - Lb = (b - a)(a + b)/2 - log(a / b) + (series(a) - series(b)) is formed WITHOUT the
// cancellation of two logarithms of size x^2 / 2 (1,200 at 49 standard deviations, which would leave 1e-8 of a narrow interval).
// Finite wherever a < b as doubles; 0 for (-inf, +inf).
BDF_HD_FORCE inline double bdf_lpd_mass(double m, double lo, double hi, double alpha)
{
    const double ra = sqrt(alpha);
    double a = (lo - m) * ra, b = (hi - m) * ra;
    if (a + b > 0.0) {
        const double t = a;
        a = -b; b = -t;
    }
    if (b > -37.0) return log(bdf_phi(b) - bdf_phi(a));
    const double Lb = bdf_log_phi(b);
    if (a == -INFINITY) return Lb;
    const double d = 0.5 * (b - a) * (a + b) - log(a / b) + (bdf_log_tail_series(a) - bdf_log_tail_series(b));
    return Lb + log(-expm1(d));
}

// the log-likelihood of a record by its kind: the probit map when the pairs carry the probit link, else the interval's mass where
// the bounds differ, else the Gaussian density at the stored value (lo == hi: a measurement)
BDF_HD_FORCE inline double bdf_lpd_record(int link, double y, double m, double lo, double hi, double alpha)
{
    if (link == 1) return bdf_lpd_probit(y, m);
    if (lo != hi) return bdf_lpd_mass(m, lo, hi, alpha);
    return bdf_lpd_gauss(y, m, alpha);
}
