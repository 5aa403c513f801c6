// background.h -- the scalar maps of a relation with background cells: every cell that is not listed
// observes a background value with precision alpha c0.  Plain C++ (no HIP types): the same text compiles for the device and for a
// host check.
#pragma once
#include "probit.h"

// the precision the rows of a relation with unit weights read: a listed cell counts with alpha (1 - c0) beside the Gram term
BDF_HD inline double bdf_bg_alpha_rows(double alpha, double c0) { return alpha * (1.0 - c0); }

// a listed cell's term of the sum of c e^2 over all cells: its own omega e^2, less what the closed form below counts for it as
// a background cell; e = y - mean - psi, rb = background value - mean, psi = u.v
BDF_HD inline double bdf_bg_term(double omega, double e, double c0, double rb, double psi)
{
    const double d = rb - psi;
    return omega * (e * e) - c0 * (d * d);
}

// c0 sum over ALL cells of (rb - psi)^2 = c0 [N M rb^2 - 2 rb (sum U).(sum V) + <U U', V V'>]
BDF_HD inline double bdf_bg_all_cells(double c0, double cells, double rb, double dot_sums, double dot_grams)
{
    return c0 * ((cells * (rb * rb) - 2.0 * rb * dot_sums) + dot_grams);
}
