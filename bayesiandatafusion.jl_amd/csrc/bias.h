// bias.h -- the scalar maps of a relation's row and column biases: a cell whose id in a biased mode m is j
// is shifted by b^m_j, b^m_j ~ N(0, 1 / lambda_m) a priori, lambda_m ~ Gamma(shape_m, rate_m).  From the sum of a row's residuals
// and its normal to b^m_j, and from the gamma variate and the sum of squares to lambda_m.  Plain C++ (no HIP types): the same
// text compiles for the device and for a host check.
//
// The summation order of S_j = sum of r_k over the n_j cells of row j, entries 0 .. n_j - 1 in the order of the mode's CSR
// (k_bias.hip, k_bias_rows), r_k = bdf_bias_resid(e_k, the other biased modes' biases of the cell in rising mode order).  A group
// of W lanes takes the row; lane l adds entries l, l + W, l + 2 W, ... in that order, starting from 0.0, and the W lane sums are
// added by a butterfly, v += the value of lane (l xor off), off = W / 2, W / 4, ..., 1:
//   W = 8  (nnz <= 32 N):  ((p0 + p4) + (p2 + p6)) + ((p1 + p5) + (p3 + p7))
//   W = 64 (nnz  > 32 N):  the same tree one level deeper per doubling: at the leaves p_l + p_(l + 32), then pairs 16 apart, 8, 4,
//                          2 and last 1 apart
// (every lane ends with the same bits: each level adds the same two numbers in both lanes of a pair, and + commutes).  A row
// without cells has S_j = 0.0 and draws from its prior.
// sum_j (b^m_j)^2: the rows of a workgroup of 256 lanes (256 / W rows, taken in the relation's degree order, bdf_relation_order)
// hold b^2 in the group's first lane, the other lanes 0.0; the wave's 64 values by the butterfly off = 32 .. 1, the four wave
// sums as (w0 + w1) + (w2 + w3); then one workgroup adds the workgroups' sums: lane t adds sums t, t + 256, ... in that order,
// and the 256 lane sums are added the same way.
#pragma once
#include "probit.h"

// what a cell's residual e_k = y_k - (udot_k + mean) leaves once another biased mode's current bias is taken off
BDF_HD inline double bdf_bias_resid(double r, double other_bias) { return r - other_bias; }

// b^m_j | rest ~ N(alpha S_j / prec_j, 1 / prec_j), prec_j = lambda_m + alpha n_j, from the standard normal z
BDF_HD inline double bdf_bias_prec(double lambda, double alpha, long long n_j) { return lambda + alpha * (double)n_j; }
BDF_HD inline double bdf_bias_row(double S, long long n_j, double alpha, double lambda, double z)
{
    const double prec = bdf_bias_prec(lambda, alpha, n_j);
    return alpha * S / prec + z / sqrt(prec);
}

// lambda_m | b ~ Gamma(shape + N / 2, rate + sum b^2 / 2) from G ~ Gamma(shape + N / 2, 1)
BDF_HD inline double bdf_bias_lambda_shape(double shape, long long N) { return shape + 0.5 * (double)N; }
BDF_HD inline double bdf_bias_lambda(double G, double rate, double sum_b2) { return G / (rate + 0.5 * sum_b2); }
