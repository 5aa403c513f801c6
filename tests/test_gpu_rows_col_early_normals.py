"""K1c (k_rows_col.hip) draws a round's row normals in its PROLOGUE -- the generator's integer rounds under the first chunk's load, the
transform under the first gathers' -- and carries the lane's two through the accumulation; before, they were drawn after the sums.
The values must be the ones drawn there: the same stream, counter and pair per lane, the same selection.  Where that can go wrong:
lanes and lane rows that are not live (an idle lane row, the lanes without a pair at D < 32), a wave whose normals another wave's
finish must reproduce (a part of a spanning row that is not the last to arrive draws a pair nobody uses; the part that finishes draws
the row's), the padded columns, and a round without observations, which now issues the first gathers too (of padding).

Cases, pieces of at most 16 observations (bdf_ctx_set_col_rows 16): D in 17, 20, 24, 28, 31, 32 (every DR instantiation, FULL, at
D = 32 the gather image's kernel and the plain one) x shared and per-row prior means x ids + values and the coded words.  ONE entity
with rows of 0, 1, 15, 16, 17, 32, 33, 64, 65 and 200 observations: whole rows, two and four pieces on one wave, rows that span waves
in two and four parts, ten rows (no multiple of four: the last round has idle lane rows); and a SECOND entity of six rows, all
empty (a relation without cells): a round without observations, and one with idle lane rows beside it.

Checks: at tolerance 0 against tests/golden/rows_col_early_normals.npz, bdf_sample_rows of the build BEFORE the move (normals after
the sums) on these inputs, recorded by `python tests/test_gpu_rows_col_early_normals.py --record` on an MI355X; against the
wave-per-row kernel on the same plan input (bdf_ctx_set_col_rows 0) at 1e-10; against the oracle at the 1e-8 of
test_gpu_rows_col.py; the not-positive-definite flag stays clear (Context.sync raises on it).
"""
import hashlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rows_col_early_normals.npz")
COUNTS = [0, 1, 15, 16, 17, 32, 33, 64, 65, 200]
N_EMPTY = 6
N_OTHER = 70
TAGS = (11, 12)
ALPHA = 1.7
CASES = [(D, per_row, coded) for D in (17, 20, 24, 28, 31, 32) for per_row in (False, True) for coded in (False, True)]


def _inputs(D, coded):
    rng = np.random.default_rng(7100 + 2 * D + int(coded))
    n = len(COUNTS)
    rows = np.repeat(np.arange(1, n + 1), COUNTS)
    ids = np.stack([rows, rng.integers(1, N_OTHER + 1, len(rows))], axis=1).astype(np.int64)
    vals = rng.integers(1, 6, len(rows)).astype(np.float64) if coded else rng.random(len(rows)) * 4 + 1
    fac = rng.standard_normal((N_OTHER, D)) * 0.5
    A = rng.standard_normal((D, D))
    return (ids, vals, fac, A @ A.T / D + np.eye(D), rng.standard_normal(D), rng.standard_normal((n, D)),
            rng.standard_normal((N_EMPTY, D)))


def _digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()


def _key(D, per_row, coded):
    return "D%d_%s_%s" % (D, "rowmeans" if per_row else "shared", "coded" if coded else "values")


def _entities(D, coded):
    """-> [(ids, vals, dims, mu_rows)] of the two entities, and what they share"""
    ids, vals, fac, Lam, mu, mu_rows, mu_empty = _inputs(D, coded)
    full = (ids, vals, [len(COUNTS), N_OTHER], mu_rows)
    empty = (np.zeros((0, 2), dtype=np.int64), np.zeros(0), [N_EMPTY, N_OTHER], mu_empty)
    return [full, empty], fac, Lam, mu, float(vals.mean())


def _run_case(B, ctx, D, per_row, coded):
    """-> ({"col": K1c's samples of the two entities, one under the other, "plain": K1c's without the gather image (D = 32),
    "k1": the wave-per-row kernel's}, digest of the inputs)"""
    from test_gpu_rows import _dev_terms, _run_rows
    ents, fac, Lam, mu, mean = _entities(D, coded)
    f_t, Lam_t = ctx.tensor(fac), ctx.tensor(Lam)
    got = {}
    ctx.set_lowrank(0, 0)
    # (an iteration number per case: the dispatch counts of a tag start anew with it)
    ctx.set_sweep(60 + CASES.index((D, per_row, coded)))
    rels = []
    try:
        for e, (ids, vals, dims, mu_rows) in enumerate(ents):
            N = dims[0]
            dr = B.DeviceRelation(ctx, B.IndexedDF((ids, vals), dims))
            rels.append(dr)
            mu_t = ctx.tensor(mu_rows if per_row else mu)
            terms = _dev_terms(B, ctx, [(dr, 0, ALPHA, mean, [None, f_t], None)])
            for name, piece, image in (("col", 16, 1), ("plain", 16, 0), ("k1", 0, 1)):
                if name == "plain" and D != 32:
                    continue
                ctx.set_col_rows(piece)
                ctx.set_gather_image(image)
                before = ctx.gather_image_stats()["launches"]
                out_t = ctx.zeros(N, D)
                _run_rows(B, ctx, D, N, terms, mu_t, Lam_t, TAGS[e], out_t)      # (its sync raises if the not-positive-definite flag is set)
                d = ctx.rows_dispatch(TAGS[e])
                took_image = ctx.gather_image_stats()["launches"] - before
                if piece:
                    assert d["col"] >= N and d["k1"] == 0, d
                    assert took_image == (1 if D == 32 and image else 0), (name, took_image)
                else:
                    assert d["k1"] == N, d
                got.setdefault(name, []).append(out_t.cpu().numpy())
        assert ctx.rows_unfinished() == 0
    finally:
        ctx.set_gather_image(1)
        ctx.set_col_rows(-1)
        ctx.set_lowrank(-1, 8192)
        for dr in rels:
            dr.close()
    return {k: np.concatenate(v, axis=0) for k, v in got.items()}, _digest(*_inputs(D, coded))


def _oracle(O, D, per_row, coded):
    """the oracle's samples of the two entities, one under the other, on the streams _run_case's launches draw from"""
    from test_gpu_rows import SEED
    ents, fac, Lam, mu, mean = _entities(D, coded)
    out = []
    for e, (ids, vals, dims, mu_rows) in enumerate(ents):
        t = O.Term(ids, vals, dims, 0, ALPHA, mean, [None, fac])
        out.append(O.sample_rows(D, dims[0], [t], mu_rows if per_row else mu, Lam, SEED, 60 + CASES.index((D, per_row, coded)), TAGS[e]))
    return np.concatenate(out, axis=0)


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("D,per_row,coded", CASES)
def test_col_early_normals_keep_the_bits(B, O, ctx, golden, D, per_row, coded):
    got, digest = _run_case(B, ctx, D, per_row, coded)
    key = _key(D, per_row, coded)
    assert np.array_equal(golden[key + "/inputs"], digest), "the generated inputs are not the recorded ones: the fixture does not apply"
    exp = golden[key]
    ora = _oracle(O, D, per_row, coded)
    for name, x in got.items():
        assert np.isfinite(x).all(), name
        print("%s %s: max |difference| to the recording %.3e, to the wave-per-row kernel %.3e, to the oracle %.3e (relative %.3e)"
              % (key, name, float(np.max(np.abs(x - exp))), float(np.max(np.abs(x - got["k1"]))), float(np.max(np.abs(x - ora))),
                 float(np.max(np.abs(x - ora) / np.maximum(np.abs(ora), 1e-300)))))
    np.testing.assert_allclose(got["col"], got["k1"], rtol=1e-10, atol=1e-11)
    np.testing.assert_allclose(got["col"], ora, rtol=1e-8, atol=1e-9)
    assert got["col"].shape == exp.shape == (len(COUNTS) + N_EMPTY, D) and np.array_equal(got["col"], exp)
    if D == 32:
        assert np.array_equal(got["plain"], exp)
    # every row is a draw of its own: the empty row of the first entity, the rows of the empty one, and the same row number of the two
    rows = got["col"]
    assert np.all(rows[0] != rows[1])
    for i in range(len(COUNTS), len(rows)):
        assert np.all(rows[i] != rows[i - 1]) and np.all(rows[i] != rows[i - len(COUNTS)])


def _record():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import bdf_amd as B
    ctx = B.Context(seed=1234)
    out = {}
    for D, per_row, coded in CASES:
        got, digest = _run_case(B, ctx, D, per_row, coded)
        if D == 32:
            assert np.array_equal(got["col"], got["plain"])
        out[_key(D, per_row, coded)], out[_key(D, per_row, coded) + "/inputs"] = got["col"], digest
    ctx.close()
    dst = sys.argv[2] if len(sys.argv) > 2 else GOLDEN
    np.savez(dst, **out)
    print("recorded %d arrays, %d bytes -> %s" % (len(out), os.path.getsize(dst), dst))


if __name__ == "__main__" and len(sys.argv) > 1 and sys.argv[1] == "--record":
    _record()
