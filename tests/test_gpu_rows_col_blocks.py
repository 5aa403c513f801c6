"""K1c (k_rows_col.hip) accumulates the ten unique 8 x 8 blocks of S~ (40 fmacs per observation) and rebuilds the full columns once
per round: the sampled rows must keep THE BITS of the kernel that accumulated the three 16 x 16 blocks (48 fmacs).  Every accumulator
sees the same fma(acc, a, b) over the same observations -- only a and b trade places -- so the tolerance is 0.

The reference is tests/golden/rows_col_blocks.npz: bdf_sample_rows of the parent build (48 fmacs) on the inputs below, recorded by
`python tests/test_gpu_rows_col_blocks.py --record` on an MI355X.  K1c has no dump of the row system (bdf_row_system goes through the
wave-per-row kernel), so every case is recorded twice as samples, under two sweeps: two draws of the normals on the same system.

Cases, pieces of at most 16 observations (bdf_ctx_set_col_rows): D in 17, 20, 24, 28, 32 (every DR instantiation and FULL) x ids + values
and the coded variant x shared and per-row prior means; rows of 0, 1, 7, 8, 9, 15, 16, 17, 32, 33, 64, 65 observations (whole rows, two
and four pieces on one wave), 130 and 700 (rows that span waves: 3 and 11 parts through the slab, the last-arriving part sums them) and
five random lengths: 19 rows, no multiple of four.  One case at the default piece (128) with a row of 2,000 observations.
"""
import hashlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rows_col_blocks.npz")
HEAD = [0, 1, 7, 8, 9, 15, 16, 17, 32, 33, 64, 65, 130, 700]
DIMS = [19, 60]
SWEEPS = (6, 9)
CASES = [(D, coded, per_row) for D in (17, 20, 24, 28, 32) for coded in (False, True) for per_row in (False, True)]


def _inputs(seed, D, dims, head, hi, coded):
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, hi, dims[0])
    deg[:len(head)] = head
    rows = np.repeat(np.arange(1, dims[0] + 1), deg)
    ids = np.stack([rows, rng.integers(1, dims[1] + 1, len(rows))], axis=1).astype(np.int64)
    vals = rng.integers(1, 6, len(rows)).astype(np.float64) if coded else rng.random(len(rows)) * 4 + 1
    fac = rng.standard_normal((dims[1], D)) * 0.5
    A = rng.standard_normal((D, D))
    Lam = A @ A.T / D + np.eye(D)
    mu = rng.standard_normal(D)
    mu_rows = rng.standard_normal((dims[0], D))
    return ids, vals, fac, Lam, mu, mu_rows


def _digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()


def _sample(B, ctx, D, dims, inputs, per_row, piece, tag):
    """-> (samples under SWEEPS stacked, digest of the inputs)"""
    from test_gpu_rows import _dev_terms, _run_rows
    ids, vals, fac, Lam, mu, mu_rows = inputs
    N = dims[0]
    dr = B.DeviceRelation(ctx, B.IndexedDF((ids, vals), dims))
    f_t, Lam_t = ctx.tensor(fac), ctx.tensor(Lam)
    mu_t = ctx.tensor(mu_rows if per_row else mu)
    terms = _dev_terms(B, ctx, [(dr, 0, 1.7, float(vals.mean()), [None, f_t], None)])
    out = []
    ctx.set_lowrank(0, 0)
    ctx.set_col_rows(piece)
    try:
        for sweep in SWEEPS:
            ctx.set_sweep(sweep)
            out_t = ctx.zeros(N, D)
            _run_rows(B, ctx, D, N, terms, mu_t, Lam_t, tag, out_t)
            d = ctx.rows_dispatch(tag)
            assert d["col"] == N and d["k1"] == 0, d
            out.append(out_t.cpu().numpy())
        assert ctx.rows_unfinished() == 0
    finally:
        ctx.set_col_rows(-1)
        ctx.set_lowrank(-1, 8192)
    dr.close()
    return np.stack(out), _digest(ids, vals, fac, Lam, mu, mu_rows)


def _key(D, coded, per_row):
    return "D%d_%s_%s" % (D, "coded" if coded else "values", "rowmeans" if per_row else "shared")


def _run_case(B, ctx, D, coded, per_row):
    return _sample(B, ctx, D, DIMS, _inputs(3100 + 2 * D + int(coded), D, DIMS, HEAD, 60, coded), per_row, 16, 5)


def _run_default_piece(B, ctx):
    dims = [7, 300]
    return _sample(B, ctx, 32, dims, _inputs(3200, 32, dims, [2000, 513, 129, 128, 5, 0, 300], 2, True), False, 128, 5)


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _compare(golden, key, got, digest):
    assert np.array_equal(golden[key + "/inputs"], digest), "the generated inputs are not the recorded ones: the fixture does not apply"
    exp = golden[key]
    assert np.isfinite(got).all()
    diff = float(np.max(np.abs(got - exp)))
    print("%s: %d rows x %d sweeps, max |difference| %.3e" % (key, got.shape[1], got.shape[0], diff))
    assert got.shape == exp.shape and np.array_equal(got, exp)
    assert not np.array_equal(got[0], got[1])                # two draws


@pytest.mark.parametrize("D,coded,per_row", CASES)
def test_col_blocks_keep_the_bits(B, ctx, golden, D, coded, per_row):
    got, digest = _run_case(B, ctx, D, coded, per_row)
    _compare(golden, _key(D, coded, per_row), got, digest)


def test_col_blocks_keep_the_bits_at_the_default_piece(B, ctx, golden):
    got, digest = _run_default_piece(B, ctx)
    _compare(golden, "D32_default_piece", got, digest)


def _record():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import bdf_amd as B
    ctx = B.Context(seed=1234)
    out = {}
    for D, coded, per_row in CASES:
        k = _key(D, coded, per_row)
        out[k], out[k + "/inputs"] = _run_case(B, ctx, D, coded, per_row)
    out["D32_default_piece"], out["D32_default_piece/inputs"] = _run_default_piece(B, ctx)
    ctx.close()
    dst = sys.argv[2] if len(sys.argv) > 2 else GOLDEN
    np.savez(dst, **out)
    print("recorded %d arrays, %d bytes -> %s" % (len(out), os.path.getsize(dst), dst))


if __name__ == "__main__" and len(sys.argv) > 1 and sys.argv[1] == "--record":
    _record()
