// robust.h -- the scalar maps of the robust (Student-t) noise model: from the gamma variate of one
// observation to its precision weight, and the term it adds to the weighted sum of squares.  Plain C++ (no HIP types): the same
// text compiles for the device and for a host check.
#pragma once
#include "probit.h"

// omega | e ~ Gamma((nu + 1) / 2, rate (nu + alpha e^2) / 2) from G ~ Gamma((nu + 1) / 2, 1).  Finite and positive for finite e:
// G > 0 (Marsaglia-Tsang returns d v with v > 0) and the denominator is at least nu >= 1.
BDF_HD inline double bdf_robust_omega(double G, double nu, double alpha, double e) { return 2.0 * G / (nu + alpha * (e * e)); }

// the observation's term of sum omega e^2
BDF_HD inline double bdf_robust_term(double omega, double e) { return omega * (e * e); }
