"""K1c's finish (dpp_rows32.h: fin_factor, fin_backward) selects by the lane's place in its row of sixteen in every step -- the pivot's
lane, the lanes right of it (unfinished columns), the lanes left of it (the backward solve) -- and the compiler is free to keep those
conditions as lane masks in scalar registers from the top of the kernel on (since the round loop went -- r14, DESIGN.md section 4 -- it
keeps some and compares the lane number again for the others).  What a change to the round's fixed parts can break there is a condition at the edge of a lane row (lanes 0 and 15, the step from a lane's
first column to its second) or of the padded columns (D < 32: columns D .. 31 are the identity), in one lane row and not in another:
every lane row of a wave carries a row of its own here, idle lane rows included.  And with one round per wave taken as round w, a
round with idle lane rows, a part that is not its row's last and a round without observations all leave the kernel their own way.

Cases, pieces of at most 16 observations (bdf_ctx_set_col_rows 16): D in 17, 20, 24, 28, 31, 32 (every DR instantiation, FULL, the
gather image's kernel and the plain one at D = 32) x shared and per-row prior means; ONE entity with rows of 0, 1, 15, 16, 17, 33,
64, 65 and 200 observations: an idle lane row, whole rows, two and four pieces on one wave, rows that span waves (two and four
parts through the slab) and a round with fewer than four jobs.

Checks: against the wave-per-row kernel on the same plan input (bdf_ctx_set_col_rows 0) at the 1e-10 of test_gpu_rows_col.py --
the same factorisation of the same matrix in another order of the sums; at tolerance 0 against tests/golden/rows_col_finish_masks.npz,
bdf_sample_rows of the build BEFORE r14 (the round loop, the table of a wave's rounds) on these inputs, recorded by
`python tests/test_gpu_rows_col_finish_masks.py --record` on an MI355X; the not-positive-definite flag stays clear (Context.sync
raises on it).
"""
import hashlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rows_col_finish_masks.npz")
COUNTS = [0, 1, 15, 16, 17, 33, 64, 65, 200]
N_OTHER = 70
TAG = 11
CASES = [(D, per_row) for D in (17, 20, 24, 28, 31, 32) for per_row in (False, True)]


def _inputs(D):
    rng = np.random.default_rng(5100 + D)
    n = len(COUNTS)
    rows = np.repeat(np.arange(1, n + 1), COUNTS)
    ids = np.stack([rows, rng.integers(1, N_OTHER + 1, len(rows))], axis=1).astype(np.int64)
    vals = rng.random(len(rows)) * 4 + 1
    fac = rng.standard_normal((N_OTHER, D)) * 0.5
    A = rng.standard_normal((D, D))
    return ids, vals, fac, A @ A.T / D + np.eye(D), rng.standard_normal(D), rng.standard_normal((n, D))


def _digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()


def _key(D, per_row):
    return "D%d_%s" % (D, "rowmeans" if per_row else "shared")


def _run_case(B, ctx, D, per_row):
    """-> ({"col": K1c's sample, "plain": K1c's without the gather image (D = 32), "k1": the wave-per-row kernel's}, digest of the inputs)"""
    from test_gpu_rows import _dev_terms, _run_rows
    inputs = _inputs(D)
    ids, vals, fac, Lam, mu, mu_rows = inputs
    N, dims = len(COUNTS), [len(COUNTS), N_OTHER]
    dr = B.DeviceRelation(ctx, B.IndexedDF((ids, vals), dims))
    f_t, Lam_t = ctx.tensor(fac), ctx.tensor(Lam)
    mu_t = ctx.tensor(mu_rows if per_row else mu)
    terms = _dev_terms(B, ctx, [(dr, 0, 1.7, float(vals.mean()), [None, f_t], None)])
    got = {}
    ctx.set_lowrank(0, 0)
    # (an iteration number per case: the dispatch counts of a tag start anew with it)
    ctx.set_sweep(40 + CASES.index((D, per_row)))
    try:
        for name, piece, image in (("col", 16, 1), ("plain", 16, 0), ("k1", 0, 1)):
            if name == "plain" and D != 32:
                continue
            ctx.set_col_rows(piece)
            ctx.set_gather_image(image)
            before = ctx.gather_image_stats()["launches"]
            out_t = ctx.zeros(N, D)
            _run_rows(B, ctx, D, N, terms, mu_t, Lam_t, TAG, out_t)      # (its sync raises if the not-positive-definite flag is set)
            d = ctx.rows_dispatch(TAG)
            took_image = ctx.gather_image_stats()["launches"] - before
            if piece:
                assert d["col"] >= N and d["k1"] == 0, d
                assert took_image == (1 if D == 32 and image else 0), (name, took_image)
            else:
                assert d["k1"] == N, d
            got[name] = out_t.cpu().numpy()
        assert ctx.rows_unfinished() == 0
    finally:
        ctx.set_gather_image(1)
        ctx.set_col_rows(-1)
        ctx.set_lowrank(-1, 8192)
    dr.close()
    return got, _digest(*inputs)


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("D,per_row", CASES)
def test_col_finish_masks_keep_the_bits(B, ctx, golden, D, per_row):
    got, digest = _run_case(B, ctx, D, per_row)
    key = _key(D, per_row)
    assert np.array_equal(golden[key + "/inputs"], digest), "the generated inputs are not the recorded ones: the fixture does not apply"
    exp = golden[key]
    for name, x in got.items():
        assert np.isfinite(x).all(), name
        print("%s %s: max |difference| to the recording %.3e, to the wave-per-row kernel %.3e"
              % (key, name, float(np.max(np.abs(x - exp))), float(np.max(np.abs(x - got["k1"])))))
    np.testing.assert_allclose(got["col"], got["k1"], rtol=1e-10, atol=1e-11)
    assert got["col"].shape == exp.shape and np.array_equal(got["col"], exp)
    if D == 32:
        assert np.array_equal(got["plain"], exp)
    assert np.all(got["col"][0] != got["col"][1])               # every row is a draw of its own, the empty one too


def _record():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import bdf_amd as B
    ctx = B.Context(seed=1234)
    out = {}
    for D, per_row in CASES:
        got, digest = _run_case(B, ctx, D, per_row)
        if D == 32:
            assert np.array_equal(got["col"], got["plain"])
        out[_key(D, per_row)], out[_key(D, per_row) + "/inputs"] = got["col"], digest
    ctx.close()
    dst = sys.argv[2] if len(sys.argv) > 2 else GOLDEN
    np.savez(dst, **out)
    print("recorded %d arrays, %d bytes -> %s" % (len(out), os.path.getsize(dst), dst))


if __name__ == "__main__" and len(sys.argv) > 1 and sys.argv[1] == "--record":
    _record()
