"""The Normal-Wishart hyperprior update (K6: csrc/k_hyper.hip, csrc/hyper_job.h) restated in numpy.longdouble, in this project's words:
the sums of an entity's rows, the parameters of the conditional Normal-Wishart, the draw from it with the random part supplied (both
maps from the mean's normals), the random part itself from the oracle's stream functions, the prior pack the draw leaves for the row
sampler, and the partition of the rows into workgroups.  numpy.linalg does not take long double: the factorisation, the triangular
inverse and the products are written out (one numpy call per row or column; D <= 64).  Nothing here touches the device, and nothing
is imported from the library: tests/test_hyper_edge_inputs_host.py holds this file against the double-precision oracle."""
import numpy as np

from oracle import oracle as O

LD = np.longdouble
HS_ROWS = 128                       # rows per chunk: 8 steps of 4 rows on each of a workgroup's 4 waves
UNFUSED_WORKGROUPS = 2048           # the sums on their own: one chunk per workgroup up to here, then whole chunks more
CHAIN_ROWS = 16384                  # the one-launch chain is taken up to this many rows
CHAIN_SLOTS = 16                    # nominal resident workgroups of the chain: the last one, the draws', the partial sums'


# ---- the sums ---------------------------------------------------------------------------------------------------------------------
def sums(S, uhat=None, block=4096):
    """U = S - uhat in double (one rounding per element, as the kernel forms it), then sum_k u_k and sum_k u_k u_k' in long double,
    in row blocks.  -> sumU, UUt (long double), and the bound on a double-precision sum in ANY order, per element:
    N 2^-52 sum_k |u_ki| and N 2^-52 sum_k |u_ki u_kj| (double: the bound needs no more digits than it has)"""
    S = np.asarray(S, dtype=np.float64)
    N, D = S.shape
    sumU, UUt = np.zeros(D, LD), np.zeros((D, D), LD)
    aU, aUU = np.zeros(D), np.zeros((D, D))
    for r0 in range(0, N, block):
        U = S[r0:r0 + block] if uhat is None else S[r0:r0 + block] - np.asarray(uhat[r0:r0 + block], dtype=np.float64)
        Ul = U.astype(LD)
        sumU += Ul.sum(0)
        UUt += Ul.T @ Ul
        Ua = np.abs(U)
        aU += Ua.sum(0)
        aUU += Ua.T @ Ua
    eps = N * 2.0 ** -52
    return sumU, UUt, eps * aU, eps * aUU


# ---- long-double linear algebra, written out ------------------------------------------------------------------------------------------
def chol_lower(M):
    """L lower with L L' = M (M symmetric positive definite)"""
    M = np.asarray(M, dtype=LD)
    n = len(M)
    L = np.zeros((n, n), LD)
    for j in range(n):
        d = M[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0:
            raise np.linalg.LinAlgError(f"pivot {j} is {d}")
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (M[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def lower_inverse(L):
    """inverse of a lower-triangular matrix, row by row: X[i] = (e_i - L[i, :i] X[:i]) / L[i, i]"""
    n = len(L)
    X = np.zeros((n, n), LD)
    for i in range(n):
        X[i, :i] = -(L[i, :i] @ X[:i, :i]) / L[i, i]
        X[i, i] = LD(1) / L[i, i]
    return X


def spd_inverse(M):
    Li = lower_inverse(chol_lower(M))
    return Li.T @ Li


def solve_upper(Ut, z):
    """x with Ut x = z, Ut upper triangular: backward substitution"""
    n = len(z)
    x = np.zeros(n, LD)
    for i in range(n - 1, -1, -1):
        x[i] = (z[i] - Ut[i, i + 1:] @ x[i + 1:]) / Ut[i, i]
    return x


# ---- ConditionalNormalWishart and the draw ---------------------------------------------------------------------------------------------
def params(sumU, UUt, N, mu0, b0, Tinv, nu):
    """-> mu_N, beta_N, nu_N, W = Tinv + UU' + b0 mu0 mu0' - beta_N mu_N mu_N'  (= inv(T_N))"""
    sumU, UUt, mu0, Tinv = (np.asarray(a, dtype=LD) for a in (sumU, UUt, mu0, Tinv))
    beta_N, nu_N = LD(b0) + LD(N), LD(nu) + LD(N)
    mu_N = (LD(b0) * mu0 + sumU) / beta_N
    W = Tinv + UUt + LD(b0) * np.outer(mu0, mu0) - beta_N * np.outer(mu_N, mu_N)
    return mu_N, beta_N, nu_N, W


def draw(W, mu_N, beta_N, A, z, mean_map="factor"):
    """T_N = inv(W), L_T = chol(T_N) lower, Z = L_T A, Lambda = Z Z'; the mean through the factor Z (mu_N + Z^-T z / sqrt(beta_N), the
    library's default) or by the reference's map (mu_N + chol(inv(Lambda) / beta_N)' z, chol upper: BDF_HYPER_MEAN=reference).
    -> mu, Lambda, and the intermediates {T_N, L_T, Z} for locating a lost digit"""
    W, mu_N, A, z = (np.asarray(a, dtype=LD) for a in (W, mu_N, A, z))
    beta_N = LD(beta_N)
    T_N = spd_inverse(W)
    L_T = chol_lower(T_N)
    Z = L_T @ np.tril(A)
    Lam = Z @ Z.T
    if mean_map == "factor":
        mu = mu_N + solve_upper(Z.T, z) / np.sqrt(beta_N)
    elif mean_map == "reference":
        mu = mu_N + chol_lower(spd_inverse(Lam) / beta_N) @ z
    else:
        raise ValueError(mean_map)
    return mu, Lam, {"T_N": T_N, "L_T": L_T, "Z": Z, "pivots": np.diag(chol_lower(W)) ** 2}


def draws(D, nu_N, seed, sweep, tag):
    """the data-independent part, k_hyper_draws' layout: the Bartlett matrix row-major (A_aa = sqrt(2 gamma(row a, shape (nu_N - a) / 2)),
    A_ac = normal(P_NW_NORMAL, row a, entry c) for c < a, zero above the diagonal), then the D normals of the mean
    (P_NW_MEAN, row 0)"""
    out = np.zeros(D * D + D)
    for a in range(D):
        out[a * D:a * D + a] = O.normals(seed, sweep, O.P_NW_NORMAL, tag, a, D)[:a]
        out[a * D + a] = np.sqrt(2.0 * O.gamma(seed, sweep, tag, a, 0.5 * (float(nu_N) - a)))
    out[D * D:] = O.normals(seed, sweep, O.P_NW_MEAN, tag, 0, D)
    return out


# ---- the prior pack ---------------------------------------------------------------------------------------------------------------------
def width(D):
    return 16 if D <= 16 else (32 if D <= 32 else 64)


def pack_doubles(D):
    DB = width(D) // 16
    return D + DB * (DB + 1) // 2 * 4 * 64


def reversed_padded(Lambda, D):
    """Lambda in index-reversed coordinates on the width's square, identity on the padding"""
    DP = width(D)
    Lt = np.eye(DP, dtype=np.asarray(Lambda).dtype)
    Lt[:D, :D] = np.asarray(Lambda)[::-1, ::-1]
    return Lt


def _image_index(D):
    """(row, column) of the reversed matrix behind every element of the image: element (b 4 + r) 64 + lane of block b = (I, J <= I),
    the lower block-triangle in row order, is [16 I + (lane >> 4) + 4 r][16 J + (lane & 15)]"""
    DB = width(D) // 16
    lane = np.arange(64)
    rows, cols = [], []
    for I in range(DB):
        for J in range(I + 1):
            for r in range(4):
                rows.append(16 * I + (lane >> 4) + 4 * r)
                cols.append(16 * J + (lane & 15))
    return np.concatenate(rows), np.concatenate(cols)


def pack_image(Lambda, mu, D):
    """bdf_prior_pack_doubles(D) doubles: Lambda mu, then the accumulator-layout image of the reversed Lambda"""
    Lambda, mu = np.asarray(Lambda), np.asarray(mu)
    rows, cols = _image_index(D)
    Lt = reversed_padded(Lambda.astype(np.float64), D)
    return np.concatenate([(Lambda.astype(LD) @ mu.astype(LD)).astype(np.float64), Lt[rows, cols]])


def unpack_image(pack, D):
    """-> the first D doubles, and the width's square with the image's elements in place (its strict upper BLOCK triangle, which the
    image does not hold, mirrored from the lower one)"""
    DP = width(D)
    rows, cols = _image_index(D)
    Lt = np.full((DP, DP), np.nan)
    Lt[rows, cols] = pack[D:]
    up = np.isnan(Lt)
    Lt[up] = Lt.T[up]
    return pack[:D], Lt


# ---- the partition of an entity's rows into workgroups --------------------------------------------------------------------------------
def max_partials(D):
    """the chain's cap on the number of partial sums: of CHAIN_SLOTS nominal workgroups one is the draw's and ceil((D^2 + D) / 256) make the
    random part; between 8 and 16"""
    return max(8, min(16, CHAIN_SLOTS - 1 - (D * D + D + 255) // 256))


def _partition(N, cap):
    chunks = max(1, -(-N // HS_ROWS))
    per = -(-chunks // cap)                                  # chunks per workgroup
    rpb = HS_ROWS * per
    nblocks = max(1, -(-N // rpb))
    return nblocks, per, N - (nblocks - 1) * rpb


def unfused_partition(N):
    """-> workgroups, chunks per workgroup, rows of the last workgroup, of bdf_hyper_sums on its own"""
    return _partition(N, UNFUSED_WORKGROUPS)


def chain_partition(D, N):
    """the same when the sweep asks for the one-launch chain: at most max_partials(D) workgroups up to CHAIN_ROWS rows, the unfused
    partition above"""
    return _partition(N, max_partials(D)) if N <= CHAIN_ROWS else unfused_partition(N)
