// dense.h -- the scalar maps of a dense two-mode relation (setDense): every one of its N x M cells is
// observed, so its part of every row's conditional is the Gram matrix of the other entity's rows, which all rows share, and one
// row of the product C = R V.  Plain C++ (no HIP types): the same text compiles for the device and for a host check.
#pragma once
#include "probit.h"

// sum over ALL cells of (r_ij - u_i.v_j)^2 = sum r^2 - 2 sum_i u_i.C_i + <U'U, V'V>, C = R V of the current (U, V)
BDF_HD inline double bdf_dense_all_cells(double sum_r2, double dot_uc, double dot_grams)
{
    return (sum_r2 - 2.0 * dot_uc) + dot_grams;
}

// a hole's draw: r = u.v + z / sqrt(alpha), z standard normal
BDF_HD inline double bdf_dense_hole(double psi, double z, double alpha) { return psi + z / sqrt(alpha); }
