"""Inputs of tests/test_gpu_feature_edges.py, built on the host: the sparse matrix with the row lengths the sparse kernels branch on,
the panelled 40,003 x 40,000 matrix, the well-conditioned solve problems and the float64 statements the device results are compared
with.  Nothing here touches the device: tests/test_feature_edge_inputs_host.py checks the row-length histograms, the condition
numbers and the two shortcuts (cond_AtA, direct_solve) against their literal numpy forms without a GPU."""
import functools

import numpy as np

# row lengths (stored entries per row) the sparse kernels branch on: an empty row; the 4-entry unrolling of k_spmm_rm and its
# remainder loop (1, 4, 15, 17, 33); the 16-entry chunk of k_spmm_rm16's index prefetch, exactly full, one over, two chunks, two + 1
EDGE_ROW_LENGTHS = (0, 1, 4, 15, 16, 17, 32, 33)
EDGE_SHAPE = (67, 53)                     # neither a multiple of 8, 16 or 32
EDGE_DUPLICATE_ROWS = (0, 2, 5)           # rows whose second entry repeats the first one's column: duplicates are summed

PANEL_SHAPE = (40_003, 40_000)            # 2,500 full row blocks of sixteen and one of three; four 12,288-wide panels both ways
PANEL_WIDTH = 12_288                      # BDF_SPMM_PANEL_ROWS
PANEL_PER_ROW, PANEL_DENSE_PER_ROW = 24, 40


def edge_row_lengths():
    m = EDGE_SHAPE[0]
    lens = np.resize(np.array([33, 0, 16, 1, 17, 4, 32, 15]), m)      # neighbours differ: a wave's four rows end at different chunks
    lens[-1] = 17
    return lens


@functools.lru_cache(maxsize=None)
def edge_sparse():
    """-> rows, cols, vals (0-based COO in a shuffled order, three duplicated entries), the dense matrix with the values and the
    dense matrix of the binary operator (every stored entry counts 1)"""
    m, n = EDGE_SHAPE
    rng = np.random.default_rng(67053)
    lens = edge_row_lengths()
    rows = np.repeat(np.arange(m), lens)
    cols = []
    for i in range(m):
        c = np.sort(rng.choice(n, lens[i], replace=False))
        if i in EDGE_DUPLICATE_ROWS:
            c[1] = c[0]
        cols.append(c)
    cols = np.concatenate(cols)
    vals = rng.standard_normal(len(rows))
    perm = rng.permutation(len(rows))
    rows, cols, vals = rows[perm], cols[perm], vals[perm]
    A, Abin = np.zeros((m, n)), np.zeros((m, n))
    np.add.at(A, (rows, cols), vals)
    np.add.at(Abin, (rows, cols), 1.0)
    for a in (rows, cols, vals, A, Abin):
        a.setflags(write=False)
    return rows, cols, vals, A, Abin


@functools.lru_cache(maxsize=None)
def panel_sparse():
    """-> rows, cols (0-based, sorted by row then column: the library panels only rows in column order), the rows' lengths, the
    empty rows and the rows with PANEL_DENSE_PER_ROW entries inside ONE panel (-> their panel)"""
    m, n = PANEL_SHAPE
    rng = np.random.default_rng(40003)
    pick = rng.choice(m - 3, 200, replace=False)
    empty = np.sort(np.append(pick[:100], 0))                        # the first row among them
    dense = np.sort(np.append(pick[100:], m - 1))                    # the last row (in the partial row block) among them
    stride = n // PANEL_PER_ROW
    cols = np.arange(PANEL_PER_ROW) * stride + rng.integers(0, stride, (m, PANEL_PER_ROW))      # one per stratum: distinct, in order
    per_row = [None] * m
    panel_of = {}
    for q, i in enumerate(dense):
        p = q % 4
        lo = p * PANEL_WIDTH
        w = (min(n, lo + PANEL_WIDTH) - lo) // PANEL_DENSE_PER_ROW
        per_row[i] = lo + np.arange(PANEL_DENSE_PER_ROW) * w + rng.integers(0, w, PANEL_DENSE_PER_ROW)
        panel_of[int(i)] = p
    lens = np.full(m, PANEL_PER_ROW)
    lens[empty] = 0
    lens[dense] = PANEL_DENSE_PER_ROW
    keep = np.ones(m, dtype=bool)
    keep[empty] = False
    keep[dense] = False
    parts = []
    plain = iter(cols[keep])
    for i in range(m):
        if lens[i] == 0:
            continue
        parts.append(per_row[i] if lens[i] == PANEL_DENSE_PER_ROW else next(plain))
    cols = np.concatenate(parts).astype(np.int64)
    rows = np.repeat(np.arange(m), lens)
    for a in (rows, cols, lens):
        a.setflags(write=False)
    return rows, cols, lens, empty, panel_of


def panel_values():
    return np.random.default_rng(24).standard_normal(len(panel_sparse()[0]))


def dense_features(rows, numF, seed):
    """rows x numF standard normals / sqrt(rows): F'F has its spectrum around 1 (Marchenko-Pastur: within (1 +- sqrt(numF / rows))^2)"""
    return np.random.default_rng(seed).standard_normal((rows, numF)) / np.sqrt(rows)


def sparse_features(rows, numF, per, seed, binary=False):
    """rows x numF, `per` entries per row in distinct columns, N(0, 1 / per) (or 1 / sqrt(per) for a pattern-only check): F F' is near I"""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    r = np.repeat(np.arange(rows), per)
    stride = numF // per
    c = (np.arange(per) * stride + rng.integers(0, stride, (rows, per))).ravel()
    v = np.ones(len(r)) if binary else rng.standard_normal(len(r)) / np.sqrt(per)
    return r, c, v, sp.csr_matrix((v, (r, c)), shape=(rows, numF))


def solve_inputs(N, D, seed):
    """sample (N x D), mu, Lambda = M M' / D + I"""
    rng = np.random.default_rng(seed)
    sample = rng.standard_normal((N, D))
    mu = rng.standard_normal(D) * 0.1
    M = rng.standard_normal((D, D))
    return sample, mu, M @ M.T / D + np.eye(D)


def _dense(A):
    return A.toarray() if hasattr(A, "toarray") else np.asarray(A)


def cond_AtA(A, lb):
    """np.linalg.cond(A.T @ A + lb I) from the singular values of A: (s_max^2 + lb) / (s_min^2 + lb), s_min = 0 when A has fewer
    rows than columns -- the same number without the numF x numF decomposition"""
    A = _dense(A)
    s = np.linalg.svd(A, compute_uv=False)
    smin = s[-1] if A.shape[0] >= A.shape[1] else 0.0
    return (s[0] ** 2 + lb) / (smin ** 2 + lb)


WOODBURY_ABOVE = 3000


def direct_solve(A, lb, rhs):
    """np.linalg.solve(A.T @ A + lb I, rhs) in float64.  Above WOODBURY_ABOVE columns (the 8,200-feature cases, whose 8,200 x 8,200
    system is a minute of host time) the same solution through the rows x rows system:
    (A'A + lb I)^-1 = (I - A'(A A' + lb I)^-1 A) / lb"""
    A = _dense(A)
    n = A.shape[1]
    if n <= WOODBURY_ABOVE:
        return np.linalg.solve(A.T @ A + lb * np.eye(n), rhs)
    return (rhs - A.T @ np.linalg.solve(A @ A.T + lb * np.eye(A.shape[0]), A @ rhs)) / lb


# ---- the cases (shared with the host check of their condition numbers) -------------------------------------------------------------
# direct solves through bdf_sample_beta(use_ff=True): (numF, D, no_eig)
DIRECT_ROWS = 300
DIRECT_CASES = [
    (1, 1, False), (15, 33, False), (16, 17, False),                       # k_solve_small<16>
    (17, 1, False), (31, 17, False), (31, 16, False), (32, 64, False),    # k_solve_small<32>
    (33, 1, False), (63, 17, False), (64, 64, False),                      # k_solve_small<64>
    (65, 1, False), (130, 17, False), (640, 33, False),                    # feat_eig_solve
    (641, 1, False), (704, 64, False), (705, 17, False),                   # bdf_chol_solve, natively
    (65, 1, True), (128, 17, True), (129, 33, True),                       # bdf_chol_solve under BDF_NO_EIG
]
REL_NUMF = [16, 17, 32, 33, 64, 65]

# CG solves through bdf_sample_beta(use_ff=False), dense F: (rows, numF, D)
CG_DENSE_CASES = [
    (300, 512, 64), (300, 513, 1), (300, 1024, 33), (300, 1025, 33), (300, 2048, 1), (300, 2049, 17),
    (600, 512, 33), (600, 513, 64), (1030, 1024, 1),
]
# sparse F: (rows, numF, D, kind)
CG_SPARSE_CASES = [(300, 2600, 33, "csr"), (300, 8200, 2, "csr"), (300, 8200, 33, "bin")]
CG_SPARSE_PER = 40

# the one-launch solve: (N, numF, D)
RESIDENT_CASES = [(200, 128, 8), (200, 129, 5), (700, 512, 32)]
RESIDENT_REFUSED = (200, 128, 9)
RESIDENT_LB = 0.6


def lb_of(numF, D):
    """lambda_beta in 0.5 .. 2.5, another one per case"""
    return 0.5 + ((7 * numF + 3 * D) % 21) / 10.0
