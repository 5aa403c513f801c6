// probit.h -- the scalar maps of the probit noise model: the normal CDF, its inverse and the map from a
// uniform to the truncated-normal latent of one 0/1 observation.  Plain C++ (no HIP types): the same text compiles for the
// device and for a host check.
#pragma once
#include <cfloat>
#include <cmath>
#if defined(__HIPCC__)
#define BDF_HD __host__ __device__
#else
#define BDF_HD
#endif

// the standard normal CDF, Phi(x) = erfc(-x / sqrt 2) / 2
BDF_HD inline double bdf_phi(double x) { return 0.5 * erfc(-x / 1.4142135623730951); }

// the inverse normal CDF for p in (0, 1): Wichura's algorithm AS 241 (PPND16; Appl. Statist. 37 (1988) 477-484), about 1e-16
// relative -- three rational functions of degree 7, in q = p - 1/2 in the centre and in sqrt(-log(min(p, 1 - p))) in the tails
// (valid to p ~ 1e-316: every normal double)
BDF_HD inline double bdf_phi_inv(double p)
{
    const double q = p - 0.5;
    if (fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        const double num = (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r +
                                4.5921953931549871457e+4) * r + 1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r +
                             1.3314166789178437745e+2) * r + 3.3871328727963666080);
        const double den = (((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r +
                                2.1213794301586595867e+4) * r + 5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r +
                             4.2313330701600911252e+1) * r + 1.0);
        return q * num / den;
    }
    double r = sqrt(-log(q < 0.0 ? p : 1.0 - p));
    double x;
    if (r <= 5.0) {
        r -= 1.6;
        const double num = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r +
                                1.27045825245236838258) * r + 3.64784832476320460504) * r + 5.76949722146069140550) * r +
                             4.63033784615654529590) * r + 1.42343711074968357734);
        const double den = (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r +
                                1.48103976427480074590e-1) * r + 6.89767334985100004550e-1) * r + 1.67638483018380384940) * r +
                             2.05319162663775882187) * r + 1.0);
        x = num / den;
    } else {
        r -= 5.0;
        const double num = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r +
                                2.65321895265761230930e-2) * r + 2.96560571828504891230e-1) * r + 1.78482653991729133580) * r +
                             5.46378491116411436990) * r + 6.65790464350110377720);
        const double den = (((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r +
                                7.86869131145613259100e-4) * r + 1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r +
                             5.99832206555887937690e-1) * r + 1.0);
        x = num / den;
    }
    return q < 0.0 ? -x : x;
}

// z ~ N(m, 1) truncated to z > 0 (y = 1) or z < 0 (y = 0), by inversion from u in (0, 1).  With s = +-1 the side, t = s m:
// s (z - m) = x is N(0, 1) truncated to x > -t, CDF value lo = Phi(-t) + u Phi(t).  Below the median x = Phi^-1(lo); above it
// 1 - lo = (1 - u) Phi(t) is formed WITHOUT the cancellation and x = -Phi^-1(1 - lo): either argument of Phi^-1 is at most 1/2,
// where a relative error eps of the argument moves x by eps p / phi(x) <= eps.  (The one-branch form Phi^-1 of u Phi(t) counted
// from the far tail loses eps / phi(t) near the boundary.)  The result is finite and strictly on y's side of 0.
BDF_HD inline double bdf_probit_z(double m, double y, double u)
{
    const double s = y > 0.5 ? 1.0 : -1.0, t = s * m;
    const double Pt = bdf_phi(t);
    const double lo = bdf_phi(-t) + u * Pt;
    const double x = lo < 0.5 ? bdf_phi_inv(fmax(lo, DBL_MIN)) : -bdf_phi_inv(fmax((1.0 - u) * Pt, DBL_MIN));
    const double z = m + s * x;
    return s * fmax(s * z, DBL_MIN);
}
