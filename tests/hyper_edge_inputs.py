"""The cases of tests/test_gpu_hyper_edges.py and tests/test_gpu_hyper_chain_edges.py, each named after the edge of the hyperprior
kernels (K6) it sits on, and their inputs, built on the host.  Nothing here touches the device: tests/test_hyper_edge_inputs_host.py
pins every case to the partition its name promises and holds the inputs to the conditions the GPU tests' bounds rest on."""
import functools

import numpy as np

import hyper_restatement as R

# the widths' edges: 16-, 32- and 64-wide instances of the kernels, and the smallest D
WIDTHS_D = (1, 2, 15, 16, 17, 31, 32, 33, 48, 63, 64)

# ---- sums: N -> (the edge, workgroups, chunks per workgroup, rows of the last workgroup) on the unfused partition --------------------
SUMS_ROWS = {
    1: ("one row: one lane row of a 4-row step", 1, 1, 1),
    3: ("three of a step's four lane rows", 1, 1, 3),
    4: ("one full 4-row step", 1, 1, 4),
    5: ("one step and a row: the second wave's first lane row", 1, 1, 5),
    127: ("a chunk less one row", 1, 1, 127),
    128: ("one full chunk", 1, 1, 128),
    129: ("a chunk and a row: two partials", 2, 1, 1),
    1920: ("15 partials: the last of the final sum's 16 chains stays empty", 15, 1, 128),
    2048: ("16 partials: one term in every chain", 16, 1, 128),
    2049: ("17 partials: two terms in chain 0", 17, 1, 1),
    4097: ("33 partials: three terms in chain 0", 33, 1, 1),
}
# above 2048 x 128 rows a workgroup takes several chunks: (D, N, with uhat) -> the same
SUMS_LARGE = {
    (32, 262_145, False): ("32-wide paired loop, two chunks; the last workgroup has one row", 1025, 2, 1),
    (17, 524_417, True): ("32-wide paired loop, three chunks: the lone tail chunk", 1366, 3, 257),
    (33, 262_145, False): ("64-wide unpaired loop, two chunks", 1025, 2, 1),
}

# ---- the random part: (D, N, nu); D D + D crosses 64 entries between 7 and 8 and 256 between 15 and 16 ------------------------------
DRAWS_CASES = [(D, N, nu) for D in (1, 7, 8, 15, 16, 64)
               for N, nu in ((5, D + 3.0), (0, float(D)), (129, D + 2.5))]      # nu = D at N = 0: the last row's shape is 1/2, below 1

# ---- the draw: every width at N = 0 (the prior alone), 5 (fewer rows than most D) and 129 -------------------------------------------
DRAW_ROWS = (0, 5, 129)
MEAN_REF_D = (2, 17, 33, 64)              # BDF_HYPER_MEAN=reference: the second factorisation on a padded matrix, at N = 129
B0 = 2.0
ORACLE_TOL = 1e-12                         # what the inputs must let the double-precision oracle reach against the restatement
COND_MAX = 1e3
DEVICE_MARGIN = 1000.0                     # the device's bound: this many times the oracle's own distance E_D

# ---- the one-launch chain as the sweep runs it: (name, D, rows of u, rows of v, features on u, BDF_NO_POLL) -> per entity the
# chain's (workgroups, chunks per workgroup, rows of the last workgroup) ---------------------------------------------------------------
CHAIN_CASES = {
    "cap14_16wide": ((15, 1792, 1793, False, False), ((14, 1, 128), (8, 2, 1))),
    "cap13_16wide": ((16, 1664, 1665, False, False), ((13, 1, 128), (7, 2, 129))),
    "cap10_fused_head": ((32, 1280, 1281, False, False), ((10, 1, 128), (6, 2, 1))),
    "cap10_generic_head": ((33, 1280, 1281, False, False), ((10, 1, 128), (6, 2, 1))),
    "cap8": ((64, 1024, 1025, False, False), ((8, 1, 128), (5, 2, 1))),
    "largest_fused_32": ((32, 16384, 300, False, False), ((10, 13, 1408), (3, 1, 44))),
    "largest_fused_64": ((64, 16384, 300, False, False), ((8, 16, 2048), (3, 1, 44))),
    "one_past_the_limit": ((32, 16385, 300, False, False), ((129, 1, 1), (3, 1, 44))),
    "with_uhat": ((17, 1665, 300, True, False), ((7, 2, 129), (3, 1, 44))),
    "no_poll": ((32, 1280, 1281, False, True), ((10, 1, 128), (6, 2, 1))),
}
CHAIN_CELLS = 4000
CHAIN_FEATURES = 5


def seed_of(D, N):
    """the seed of the case (D, N), written down: 7000 + 131 D + N mod 1000 (no two cases of this file share one)"""
    return 7000 + 131 * D + N % 1000


def sums_inputs(D, N, with_uhat):
    """-> S (N x D) = 0.7 N(0,1) + a shift per column, uhat = 0.1 N(0,1) or None"""
    rng = np.random.default_rng(seed_of(D, N))
    S = rng.standard_normal((N, D)) * 0.7 + rng.standard_normal(D)
    uh = rng.standard_normal((N, D)) * 0.1 if with_uhat else None
    return S, uh


def draw_inputs(D, N):
    """-> S, mu0 = 0.1 N(0,1), Tinv = Q Q' / D + I, b0 = 2, nu = D + 3"""
    rng = np.random.default_rng(seed_of(D, N) + 500_000)
    S = rng.standard_normal((N, D)) * 0.7 + rng.standard_normal(D)
    mu0 = rng.standard_normal(D) * 0.1
    Q = rng.standard_normal((D, D))
    return S, mu0, Q @ Q.T / D + np.eye(D), B0, D + 3.0


def rel_distance(got, want, floor=0.0):
    """max |got - want| relative to the largest entry of want (and to at least `floor`: 1 for a mean)"""
    want = np.asarray(want, dtype=R.LD)
    scale = max(float(np.abs(want).max()) if want.size else 0.0, floor)
    return float(np.abs(np.asarray(got, dtype=R.LD) - want).max() / scale) if want.size else 0.0


def restated_draw(sumU, UUt, N, mu0, b0, Tinv, nu, rand, mean_map="factor"):
    """the whole update from given sums and a given random part (k_hyper_draws' layout) -> {mu_N, W, Lambda, mu, beta_N, nu_N, ...}"""
    D = len(mu0)
    mu_N, beta_N, nu_N, W = R.params(sumU, UUt, N, mu0, b0, Tinv, nu)
    mu, Lam, mid = R.draw(W, mu_N, beta_N, rand[:D * D].reshape(D, D), rand[D * D:], mean_map)
    return dict(mu_N=mu_N, W=W, Lambda=Lam, mu=mu, beta_N=beta_N, nu_N=nu_N, **mid)


ORACLE_SWEEP, ORACLE_TAG, ORACLE_SEED = 12, 5, 1234


@functools.lru_cache(maxsize=None)
def oracle_distances(D, N):
    """how far the double-precision oracle (hyper_params, hyper_draw) lies from the restatement on the case (D, N): the distances of
    mu_N, W, Lambda and mu (both mean maps) as the GPU tests measure them, and cond(W)"""
    from oracle import oracle as O
    S, mu0, Tinv, b0, nu = draw_inputs(D, N)
    sumU, UUt, _, _ = R.sums(S)
    rand = R.draws(D, nu + N, ORACLE_SEED, ORACLE_SWEEP, ORACLE_TAG)
    mu_N, beta_N, T_N, nu_N = O.hyper_params(S, mu0, b0, Tinv, nu)
    out = {}
    for mm in ("factor", "reference"):
        want = restated_draw(sumU, UUt, N, mu0, b0, Tinv, nu, rand, mm)
        mu, Lam = O.hyper_draw(mu_N, beta_N, T_N, nu_N, ORACLE_SEED, ORACLE_SWEEP, ORACLE_TAG, mean_map=mm)
        out["mu_" + mm] = rel_distance(mu, want["mu"], 1.0)
        out["Lambda"] = max(out.get("Lambda", 0.0), rel_distance(Lam, want["Lambda"]))
    out["mu_N"] = rel_distance(mu_N, want["mu_N"], 1.0)
    out["W"] = rel_distance(np.linalg.inv(T_N), want["W"])
    out["cond_W"] = float(np.linalg.cond(want["W"].astype(np.float64)))
    assert beta_N == float(want["beta_N"]) and nu_N == float(want["nu_N"])
    return out


@functools.lru_cache(maxsize=None)
def E(D):
    """E_D: the largest distance of the oracle from the restatement over D's draw cases -- what a correct double-precision
    implementation in the reference's order of operations reaches on these inputs.  The device is held to DEVICE_MARGIN E_D."""
    return max(v for N in DRAW_ROWS for k, v in oracle_distances(D, N).items() if k != "cond_W")


def device_bound(D):
    return DEVICE_MARGIN * E(D)
