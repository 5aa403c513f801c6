// ordinal.h -- the scalar maps of the ordinal probit model's cutpoint step.  A relation with levels 1 .. K
// has the edge table e_0 = -inf < e_1 = 1.5 < ... < e_{K-1} = K - 1/2 < e_K = +inf; e_1 and e_{K-1} are fixed, the K - 3 edges
// between them are sampled.  The step works on the K - 2 gaps g_k = e_{k+1} - e_k (k = 1 .. K-2), whose sum R = e_{K-1} - e_1 is
// fixed, through the additive log-ratio coordinates theta_k = log(g_k / g_{K-2}), k = 1 .. K-3.
// Plain C++ (no HIP types, no local arrays: a kernel that calls these keeps no stack): the same text compiles for the device and
// for a host check.
#pragma once
#include "probit.h"

#define BDF_ORD_MIN_K 4
#define BDF_ORD_MAX_K 16
#define BDF_ORD_MIN_GAP 1e-6      // a proposal with a gap at or below this is refused: equal edges read as "a measurement"

// theta_k of the edge table e (K + 1 doubles), k = 1 .. K-3
BDF_HD inline double bdf_ordinal_theta(int K, const double *e, int k)
{
    return log((e[k + 1] - e[k]) / (e[K - 1] - e[K - 2]));
}

// The random-walk proposal: theta'_k = theta_k + sigma eps[k - 1], w = (exp theta'_1, ..., exp theta'_{K-3}, 1), g' = R w / sum w,
// out_k = e_1 + g'_1 + ... + g'_{k-1} for the interior edges; out_0, out_1, out_{K-1}, out_K are e's.  *jac: the log Jacobian
// term of the acceptance ratio, sum_k log g'_k - sum_k log g_k over all K - 2 gaps (the density of a uniform law on the ordered
// edges, in theta, is prod g_k up to a constant).  Returns whether every g' exceeds BDF_ORD_MIN_GAP (false for a NaN as well).
BDF_HD inline bool bdf_ordinal_propose(int K, const double *e, double sigma, const double *eps, double *out, double *jac)
{
    const double R = e[K - 1] - e[1];
    double sw = 0.0;
    for (int k = 1; k <= K - 3; k++) sw += exp(bdf_ordinal_theta(K, e, k) + sigma * eps[k - 1]);
    sw += 1.0;
    bool ok = true;
    double acc = e[1], lj = 0.0;
    out[0] = e[0]; out[1] = e[1];
    for (int k = 1; k <= K - 2; k++) {
        const double w = k <= K - 3 ? exp(bdf_ordinal_theta(K, e, k) + sigma * eps[k - 1]) : 1.0;
        const double g = R * w / sw;
        ok = ok && (g > BDF_ORD_MIN_GAP);
        lj += log(g) - log(e[k + 1] - e[k]);
        acc += g;
        if (k <= K - 3) out[k + 1] = acc;
    }
    out[K - 1] = e[K - 1]; out[K] = e[K];
    *jac = lj;
    return ok;
}

// the step size after the i-th step (i >= 1) of the burn-in: log sigma += (accepted - 0.3) / sqrt(i), sigma kept in [1e-8, 10]
BDF_HD inline double bdf_ordinal_adapt(double sigma, bool accepted, double i)
{
    const double s = exp(log(sigma) + ((accepted ? 1.0 : 0.0) - 0.3) / sqrt(i));
    return s < 1e-8 ? 1e-8 : (s > 10.0 ? 10.0 : s);
}
