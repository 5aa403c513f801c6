"""AUC_ROC (src/ROC.jl:1-11) restated as the device computes it (csrc/k_auc.hip): an order-preserving 64-bit key per score,
a stable sort of the keys, and the exact pair count C = (sum of the positives' sorted positions) - P (P - 1) / 2, so that
AUC = C / (P Nn).  The GPU tests hold bdf_auc_roc / bdf_pairs_auc to these integers exactly."""
import numpy as np

SIGN = np.uint64(1 << 63)
NAN_KEY = np.uint64(0xFFF0000000000001)          # one above +inf's key: NaNs sort last and tie among themselves


def keys(scores):
    """negatives ~bits, the rest bits | 1 << 63; -0.0 folded into +0.0; every NaN NAN_KEY"""
    x = np.ascontiguousarray(scores, dtype=np.float64).reshape(-1)
    b = x.view(np.uint64).copy()
    b[x == 0.0] = 0
    k = np.where((b & SIGN) != 0, ~b, b | SIGN)
    k[np.isnan(x)] = NAN_KEY
    return k


def order(scores):
    """the stable ranking of the scores: argsort of the keys, ties in the caller's order"""
    return np.argsort(keys(scores), kind="stable")


def counts(labels, scores, perm=None):
    """(C, P, Nn) as Python ints.  perm: the ranking to use (default: order(scores))"""
    lab = np.asarray(labels, dtype=bool).reshape(-1)
    if perm is None:
        perm = order(scores)
    pos = np.nonzero(lab[perm])[0].astype(np.int64)
    P = len(pos)
    Nn = len(lab) - P
    C = int(pos.sum(dtype=np.int64)) - P * (P - 1) // 2
    return C, P, Nn


def auc(labels, scores):
    C, P, Nn = counts(labels, scores)
    if P == 0 or Nn == 0:
        return float("nan")
    return C / (P * Nn)


def brute_force_count(labels, scores):
    """O(n^2): pairs (negative j, positive i) with j ranked before i -- a smaller key, or an equal key and a smaller index"""
    lab = np.asarray(labels, dtype=bool).reshape(-1)
    k = keys(scores)
    C = 0
    for i in np.nonzero(lab)[0]:
        for j in np.nonzero(~lab)[0]:
            if k[j] < k[i] or (k[j] == k[i] and j < i):
                C += 1
    return C


def cases(rng):
    """(name, labels, scores): the tie rules and edge cases every implementation is held to"""
    out = []
    n = 1000
    lab = rng.random(n) < 0.4
    out.append(("random", lab, rng.standard_normal(n)))
    out.append(("three_values", lab, np.round(rng.random(n) * 2.0)))
    out.append(("all_equal", lab, np.full(n, 3.25)))
    z = np.where(rng.random(n) < 0.5, 0.0, -0.0)
    z[rng.random(n) < 0.3] = 1.0
    out.append(("signed_zeros", lab, z))
    s = rng.standard_normal(n)
    s[rng.random(n) < 0.1] = np.inf
    s[rng.random(n) < 0.1] = -np.inf
    out.append(("infinities", lab, s))
    s = rng.standard_normal(n)
    s[rng.random(n) < 0.05] = np.nan
    s[:3] = [np.nan, -np.nan, np.inf]
    out.append(("nans", lab, s))
    out.append(("n1", np.array([True]), np.array([0.5])))
    out.append(("one_class", np.zeros(n, dtype=bool), rng.standard_normal(n)))
    return out
