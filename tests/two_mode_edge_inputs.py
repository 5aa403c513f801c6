"""Inputs of tests/test_gpu_vb_edges.py and tests/test_gpu_hmc_edges.py, built on the host: two-mode training sets whose user rows
have prescribed degrees (vb_restatement.make_case gives every row about the same one), the cases both files run, and the HMC
restatement's run of every HMC case, computed once.  Nothing here touches the device: tests/test_two_mode_edge_inputs_host.py checks
without a GPU that every case has the degrees, block counts, duplicates and accept / reject sequence its GPU test relies on.

"Degree" is the number of a row's neighbours after duplicates are summed, as sparse_data and two_mode_build count it.  A "pass"
is what one trip of a kernel's neighbour loop takes of a row: 4 waves x U neighbours in k_vb_rows, NG groups x 4 in k_hmc_leap."""
import functools

import numpy as np


def padded(D):
    """DP: the tile a dimension is padded to"""
    return 16 if D <= 16 else 32 if D <= 32 else 64


def vb_rows_per_block(D):
    """G of k_vb_rows"""
    return 64 // padded(D)


def vb_row_blocks(D, N):
    """blocks of a k_vb_rows launch (vb_row_blocks in k_vb.hip)"""
    G = vb_rows_per_block(D)
    return (N + G - 1) // G


def vb_pass(D):
    """neighbours per trip of k_vb_rows' gather loop: four waves, U = 4 in flight (2 at DP = 64)"""
    return 4 * (2 if padded(D) == 64 else 4)


def hmc_groups(D):
    """NG of k_hmc_leap: lane groups that deal a row's neighbours among them"""
    return 256 // padded(D)


def hmc_pass(D):
    """neighbours per trip of k_hmc_leap's loop: NG groups, four in flight"""
    return 4 * hmc_groups(D)


def make_edge_case(Nu, Nv, degrees, seed, ntest, pass_size=16):
    """ratings from a planted rank-3 model, clipped to [1, 5], in which user row i has degrees[i] distinct items (0 allowed).  The
    last item has no observations.  Every row longer than pass_size lists two of its (u, v) pairs twice: its last neighbour in
    ascending item order and its first neighbour of the second pass (one pair where they coincide).  The rows come in a shuffled
    order; the test pairs are drawn over all users and items.  Returns vb_restatement.make_case's tuple (uid, vid, values,
    test_uid, test_vid, test_values), ids 1-based."""
    degrees = np.asarray(degrees, dtype=np.int64)
    assert len(degrees) == Nu and degrees.min() >= 0 and degrees.max() <= Nv - 1 and degrees.sum() >= 1
    rng = np.random.default_rng(seed)
    Pu, Pv = rng.standard_normal((Nu, 3)), rng.standard_normal((Nv, 3))
    uid, vid = [], []
    for u, d in enumerate(degrees):
        items = np.sort(rng.choice(Nv - 1, d, replace=False)) + 1
        extra = sorted({int(items[pass_size]), int(items[-1])}) if d > pass_size else []
        uid += [u + 1] * (d + len(extra))
        vid += list(items) + extra
    uid, vid = np.array(uid, dtype=np.int64), np.array(vid, dtype=np.int64)
    perm = rng.permutation(len(uid))
    uid, vid = uid[perm], vid[perm]
    vals = np.clip(3.0 + np.sum(Pu[uid - 1] * Pv[vid - 1], axis=1) + 0.3 * rng.standard_normal(len(uid)), 1.0, 5.0)
    tu, tv = rng.integers(1, Nu + 1, ntest), rng.integers(1, Nv + 1, ntest)
    tval = np.clip(3.0 + np.sum(Pu[tu - 1] * Pv[tv - 1], axis=1) + 0.3 * rng.standard_normal(ntest), 1.0, 5.0)
    return uid, vid, vals, tu, tv, tval


def transpose(case):
    """the same observations with users and items swapped"""
    uid, vid, vals, tu, tv, tval = case
    return vid, uid, vals, tv, tu, tval


def degrees_of(case, Nu, Nv):
    """(degrees of the Nu users, degrees of the Nv items) after duplicates are summed"""
    uid, vid = case[0], case[1]
    pairs = np.unique((uid - 1) * Nv + (vid - 1))
    return np.bincount(pairs // Nv, minlength=Nu), np.bincount(pairs % Nv, minlength=Nv)


def duplicate_positions(case, Nu, Nv):
    """{user row (0-based): positions, in the row's ascending item order, of the neighbours listed more than once}"""
    uid, vid = case[0], case[1]
    pairs, cnt = np.unique((uid - 1) * Nv + (vid - 1), return_counts=True)
    out = {}
    for u in np.unique(pairs[cnt > 1] // Nv):
        mine = pairs // Nv == u
        out[int(u)] = [int(p) for p in np.nonzero(cnt[mine] > 1)[0]]
    return out


def launch_order(deg):
    """rows by descending degree, ties in row order (rows_by_degree in bdf_common.h): position k holds row launch_order(deg)[k]"""
    return np.argsort(-np.asarray(deg), kind="stable")


def spread(ladder, Nu, filler=7):
    """Nu degrees: the ladder's, apart from each other among filler rows, so that neighbours in row order differ"""
    assert len(ladder) <= Nu
    deg = np.full(Nu, filler, dtype=np.int64)
    deg[np.linspace(0, Nu - 1, len(ladder)).astype(int)] = ladder
    return deg


# ---- VB (tests/test_gpu_vb_edges.py) -----------------------------------------------------------------------------------------------
VB_LADDER_D = (16, 17, 32, 33, 63)
VB_LADDER_NU = 23                          # no multiple of G = 4 or 2: the last block has live and dead groups
VB_LADDER_CLAMPED_D = 33
VB_LADDER_TRANSPOSED_D = 17


def vb_ladder_degrees(D, Nv):
    P = vb_pass(D)
    return [0, 1, 2, 3, 4, 5, P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1, 4 * P + 1, Nv - 1]


def vb_ladder_shape(D):
    """(Nu, Nv): Nv - 1 above 4 P + 1, the longest rung"""
    return VB_LADDER_NU, 4 * vb_pass(D) + 5


@functools.lru_cache(maxsize=None)
def vb_ladder_case(D, transposed=False):
    """-> case, Nu, Nv (of the case as returned: swapped when transposed)"""
    Nu, Nv = vb_ladder_shape(D)
    case = make_edge_case(Nu, Nv, spread(vb_ladder_degrees(D, Nv), Nu), seed=100 + D, ntest=60, pass_size=vb_pass(D))
    return (transpose(case), Nv, Nu) if transposed else (case, Nu, Nv)


# rows fewer than, equal to and one more than a workgroup's G: (D, Nu, degrees); Nv = 9.  The cases of one user have one
# observation: every observed item's mean is its centred value times one and the same vector, and the centred values sum to zero,
# so with more observations V's mu_N is rounding noise around 0 and no reference for anything (the restatement's two evaluation
# orders then differ by 0.26 of max |mu_N|); with one observation every mean is exactly zero and Euu, W_N are what is compared.
VB_TAIL_NV = 9
VB_TAIL_CASES = [(4, 1, (1,)), (4, 2, (3, 1)), (4, 3, (8, 2, 1)), (4, 5, (8, 1, 4, 2, 5)), (20, 1, (1,)), (20, 3, (2, 8, 1))]


@functools.lru_cache(maxsize=None)
def vb_tail_case(D, Nu):
    deg = next(d for D_, Nu_, d in VB_TAIL_CASES if (D_, Nu_) == (D, Nu))
    return make_edge_case(Nu, VB_TAIL_NV, deg, seed=200 + 10 * D + Nu, ntest=12, pass_size=vb_pass(D))


# block counts of the U launch around VB_SLICES = 32: (D, Nu, Nv)
VB_SLICES = 32
VB_SLICE_CASES = [(33, 31, 65), (33, 32, 65), (33, 33, 65), (8, 4 * 33 + 1, 40)]


@functools.lru_cache(maxsize=None)
def vb_slice_case(D, Nu, Nv):
    deg = np.resize(np.array([3, 9, 1, 12, 6, 2, 10]), Nu)
    return make_edge_case(Nu, Nv, deg, seed=300 + D + Nu, ntest=50, pass_size=vb_pass(D))


# ---- HMC (tests/test_gpu_hmc_edges.py) ---------------------------------------------------------------------------------------------
HMC_NU, HMC_NV = 70, 140                   # above 64 and no multiple of it: k_hmc_accept's block loop has a second and a third trip
HMC_LADDER_EPS = {16: 0.01, 17: 0.005, 32: 0.005, 33: 0.002, 63: 0.002}
HMC_LADDER_TRANSPOSED_D = 16
HMC_LADDER_KW = dict(burnin=2, psamples=3, L=3, L_inner=1, prior_freq=2, clamp=(1.0, 5.0))
HMC_LADDER_NTEST = 257


def hmc_ladder_degrees(D, Nv):
    NG, P = hmc_groups(D), hmc_pass(D)
    return [0, 1, 2, NG - 1, NG, NG + 1, P - 1, P, P + 1, 2 * P + 1, Nv - 1]


@functools.lru_cache(maxsize=None)
def hmc_ladder_case(D, transposed=False, ntest=HMC_LADDER_NTEST):
    """-> case, Nu, Nv (swapped when transposed)"""
    Nu, Nv = HMC_NU, HMC_NV
    case = make_edge_case(Nu, Nv, spread(hmc_ladder_degrees(D, Nv), Nu), seed=400 + D, ntest=ntest, pass_size=hmc_pass(D))
    return (transpose(case), Nv, Nu) if transposed else (case, Nu, Nv)


HMC_SMALL_D = 17                           # the (L, L_inner) cases: a small ladder, 20 x 40
HMC_L_CASES = [(1, 1), (1, 3), (2, 2), (2, 3)]
HMC_SMALL_SHAPE = (20, 40)
HMC_PREDICT_NTEST = 600                    # three blocks of k_hmc_predict, the last with 88 pairs

ADAPT_SHAPE = (50, 40)
ADAPT_D, ADAPT_SEED = 5, 4


@functools.lru_cache(maxsize=None)
def hmc_small_case():
    Nu, Nv = HMC_SMALL_SHAPE
    D = HMC_SMALL_D
    NG, P = hmc_groups(D), hmc_pass(D)
    deg = spread([0, 1, 2, NG - 1, NG, NG + 1, P - 1, P, P + 1, Nv - 1], Nu)
    return make_edge_case(Nu, Nv, deg, seed=417, ntest=50, pass_size=P)


@functools.lru_cache(maxsize=None)
def adapt_case():
    import vb_restatement as R
    return R.make_case(*ADAPT_SHAPE, 600, seed=8, ntest=300)


def hmc_scenarios():
    """name -> (case, Nu, Nv, D, seed, keywords of hmc_restatement.run): every run of tests/test_gpu_hmc_edges.py that is compared
    with the restatement"""
    s = {}
    for D in HMC_LADDER_EPS:
        s["ladder-%d" % D] = (*hmc_ladder_case(D), D, D, dict(HMC_LADDER_KW, eps=HMC_LADDER_EPS[D]))
    D = HMC_LADDER_TRANSPOSED_D
    s["ladder-%d-transposed" % D] = (*hmc_ladder_case(D, True), D, D, dict(HMC_LADDER_KW, eps=HMC_LADDER_EPS[D]))
    for L, Li in HMC_L_CASES:
        s["steps-%d-%d" % (L, Li)] = (hmc_small_case(), *HMC_SMALL_SHAPE, HMC_SMALL_D, 10 * L + Li,
                                      dict(burnin=2, psamples=2, L=L, L_inner=Li, prior_freq=2, eps=0.004, clamp=(1.0, 5.0)))
    s["predict"] = (*hmc_ladder_case(16, False, HMC_PREDICT_NTEST), 16, 5,
                    dict(burnin=2, psamples=4, L=2, L_inner=1, prior_freq=3, eps=0.01, clamp=()))
    s["adapt-then-onward"] = (adapt_case(), *ADAPT_SHAPE, ADAPT_D, ADAPT_SEED,
                              dict(burnin=3, psamples=3, L=3, L_inner=1, prior_freq=2, eps=0.2, clamp=(1.0, 5.0)))
    s["adapt-five-times"] = (adapt_case(), *ADAPT_SHAPE, ADAPT_D, ADAPT_SEED,
                             dict(burnin=3, psamples=3, L=2, L_inner=1, prior_freq=2, eps=0.1, clamp=(1.0, 5.0)))
    for name, tr in (("restore", False), ("restore-transposed", True)):
        s[name] = (*hmc_ladder_case(16, tr), 16, 9, dict(burnin=3, psamples=0, L=2, L_inner=1, prior_freq=1000, eps=1e-3, clamp=(),
                                                         phases={3: (RESTORE_EPS, 2)}))
    return s


RESTORE_EPS = 0.3                          # the third iteration of the restore cases: dH < -6


@functools.lru_cache(maxsize=None)
def hmc_expected(name):
    """hmc_restatement.run of a scenario, row by row; shared by the host check and the GPU test, which leave it unchanged"""
    import hmc_restatement as H
    case, Nu, Nv, D, seed, kw = hmc_scenarios()[name]
    return H.run(*case, Nu, Nv, D, 2.0, seed, vectorised=False, **kw)


def metropolis_margins(exp):
    """per iteration with dH < 0: |uniform - exp(dH)| / max(uniform, exp(dH)) (None where dH >= 0: accepted whatever the uniform)"""
    import math
    out = []
    for r in exp["records"]:
        if r["dH"] >= 0:
            out.append(None)
            continue
        a, u = math.exp(r["dH"]), r["uniform"]
        out.append(abs(u - a) / max(u, a))
    return out
