// entity_noise.h -- the scalar maps of the per-row noise model: a cell whose id in the noise entity's mode is
// j is observed with precision alpha tau_j, tau_j ~ Gamma(shape, rate) a priori.  From the gamma variate of row j and the sum of
// its cells' squared residuals to tau_j, and the term the row adds to sum_j tau_j S_j.  Plain C++ (no HIP types): the same text
// compiles for the device and for a host check.
//
// The summation order of S_j = sum of e^2 over the n_j cells of row j, entries 0 .. n_j - 1 in the order of the mode's CSR
// (k_entity_noise.hip, launch 2).  A group of W lanes takes the row; lane l adds entries l, l + W, l + 2 W, ... in that order,
// starting from 0.0, and the W lane sums are added by a butterfly, v += the value of lane (l xor off), off = W / 2, W / 4, ..., 1:
//   W = 8  (nnz / N <= 32):  ((p0 + p4) + (p2 + p6)) + ((p1 + p5) + (p3 + p7))
//   W = 64 (nnz / N  > 32):  the same tree one level deeper per doubling: at the leaves p_l + p_(l + 32), then pairs 16 apart,
//                            8, 4, 2 and last 1 apart
// (every lane ends with the same bits: each level adds the same two numbers in both lanes of a pair, and + commutes).  A row
// without cells has S_j = 0.0.
// sum_j tau_j S_j: the rows of a workgroup of 256 lanes (256 / W rows, taken in the relation's degree order, bdf_relation_order)
// hold their term in the group's first lane, the other lanes 0.0; the wave's 64 values by the butterfly off = 32 .. 1, the four
// wave sums as (w0 + w1) + (w2 + w3); then one workgroup adds the workgroups' sums: lane t adds sums t, t + 256, ... in that
// order, and the 256 lane sums are added the same way.
#pragma once
#include "probit.h"

// tau_j | U, V, alpha ~ Gamma(shape + n_j / 2, rate + alpha S_j / 2) from G ~ Gamma(shape + n_j / 2, 1).  Finite and positive:
// G > 0, rate > 0 and S_j >= 0.
BDF_HD inline double bdf_entity_noise_shape(double shape, long long n_j) { return shape + 0.5 * (double)n_j; }
BDF_HD inline double bdf_entity_noise_tau(double G, double rate, double alpha, double S) { return G / (rate + 0.5 * (alpha * S)); }

// the row's term of sum_j tau_j S_j
BDF_HD inline double bdf_entity_noise_term(double tau, double S) { return tau * S; }
