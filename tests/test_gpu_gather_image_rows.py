"""K1c's gather image (k_rows_col.hip, col_gather4; k_gather_image.hip): at D = 32 an observation's factor row is gathered from a
lane-ordered copy of the opposite sample -- a lane's two elements side by side (the pair image), or those and col_rank1u's two
own-vectors (the full image).  Every accumulator sees the
same fma with the same operands in the same order -- only where the operands come from changes -- so the tolerance is 0:

  * bdf_sample_rows with the switch on (bdf_ctx_set_gather_image 1: the pair image, the default; 2: the full image) gives the
    bytes it gives with the switch off;
  * the image a launch leaves of its own rows is the pack kernel's image of those rows, and both are the layout the header of
    k_gather_image.hip states, rebuilt here in numpy.

Cases: pieces of at most 16 observations; rows of 0, 1, 15, 16, 17, 32, 33, 64, 65 observations (whole rows, two and four pieces on
one wave), 100, 250, 300, 560 and 700 (rows that span waves, in parts of at most 64: 2, 4, 5, 9 and 11 slots) and random lengths;
both modes of the relation; ids + values and packed coded values; shared and per-row prior means.  One case at the default piece
with a row of 2,000 observations.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D = 32
HEAD = [0, 1, 15, 16, 17, 32, 33, 64, 65, 100, 250, 300, 560, 700]
N_OWN, N_OTHER = 23, 61                      # no multiple of four rows; 61 rows to gather from
CASES = [(mode0, coded, per_row) for mode0 in (0, 1) for coded in (False, True) for per_row in (False, True)]


def _inputs(seed, mode0, head, n_own, n_other, hi, coded):
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, hi, n_own)
    deg[:len(head)] = head
    own = np.repeat(np.arange(1, n_own + 1), deg)
    other = rng.integers(1, n_other + 1, len(own))
    ids = np.stack([own, other] if mode0 == 0 else [other, own], axis=1).astype(np.int64)
    dims = [n_own, n_other] if mode0 == 0 else [n_other, n_own]
    vals = rng.integers(1, 6, len(own)).astype(np.float64) if coded else rng.random(len(own)) * 4 + 1
    fac = rng.standard_normal((n_other, D)) * 0.5
    A = rng.standard_normal((D, D))
    return ids, dims, vals, fac, A @ A.T / D + np.eye(D), rng.standard_normal(D), rng.standard_normal((n_own, D))


def _image_of(sample, lane_doubles):
    """the layout of k_gather_image.hip's header from the natural rows: [v0, v1(, x, y)] per lane"""
    j = np.arange(16)
    v0, v1 = sample[:, 31 - j], sample[:, 15 - j]
    if lane_doubles == 2:
        return np.stack([v0, v1], axis=2)
    h = (j >= 8)[None, :]
    return np.stack([v0, v1, np.where(h, v0, v1), np.where(h, v1, v0[:, j ^ 8])], axis=2)


def _run(B, ctx, mode0, inputs, per_row, piece, sweep, tag=7):
    """-> {switch: sample} for the switch off, on and on the full image, all under iteration number `sweep` (one per case: the
    dispatch counts of a tag start anew with the number); the images checked on the way"""
    from test_gpu_rows import _dev_terms, _run_rows
    ids, dims, vals, fac, Lam, mu, mu_rows = inputs
    N = dims[mode0]
    dr = B.DeviceRelation(ctx, B.IndexedDF((ids, vals), dims))
    f_t, Lam_t = ctx.tensor(fac), ctx.tensor(Lam)
    mu_t = ctx.tensor(mu_rows if per_row else mu)
    facs = [None, f_t] if mode0 == 0 else [f_t, None]
    terms = _dev_terms(B, ctx, [(dr, mode0, 1.7, float(vals.mean()), facs, None)])
    got = {}
    ctx.set_lowrank(0, 0)
    ctx.set_col_rows(piece)
    ctx.set_sweep(sweep)
    try:
        for k, (switch, lane_doubles) in enumerate(((0, 0), (1, 2), (2, 4))):
            ctx.set_gather_image(switch)
            before = ctx.gather_image_stats()
            out_t = ctx.zeros(N, D)
            _run_rows(B, ctx, D, N, terms, mu_t, Lam_t, tag, out_t)
            d = ctx.rows_dispatch(tag)
            assert d["col"] == (k + 1) * N and d["k1"] == 0, d          # (the launches of one iteration number add up)
            after = ctx.gather_image_stats()
            took = {k: after[k] - before[k] for k in after}
            got[switch] = out_t.cpu().numpy()
            if switch == 0:
                assert took == {"launches": 0, "packs": 0, "left": 0}, took
                continue
            # a caller that is not the native iteration: the opposite sample's image is packed for the launch, which leaves its own
            assert took == {"launches": 1, "packs": 1, "left": 1}, took
            left = ctx.gather_image_read(out_t, 16 * lane_doubles)
            packed = ctx.gather_image_pack(out_t, 16 * lane_doubles).cpu().numpy()
            assert np.array_equal(left, packed)
            assert np.array_equal(packed, _image_of(got[switch], lane_doubles))
        assert ctx.rows_unfinished() == 0
    finally:
        ctx.set_gather_image(1)
        ctx.set_col_rows(-1)
        ctx.set_lowrank(-1, 8192)
    dr.close()
    return got


def _compare(got):
    assert np.isfinite(got[0]).all() and np.abs(got[0]).max() > 0
    for switch in (1, 2):
        diff = float(np.max(np.abs(got[switch] - got[0])))
        print("switch %d against off: %d rows, max |difference| %.3e" % (switch, got[0].shape[0], diff))
        assert np.array_equal(got[switch], got[0])


@pytest.mark.parametrize("mode0,coded,per_row", CASES)
def test_rows_from_the_gather_image_keep_the_bits(B, ctx, mode0, coded, per_row):
    inputs = _inputs(4100 + 2 * mode0 + int(coded), mode0, HEAD, N_OWN, N_OTHER, 60, coded)
    _compare(_run(B, ctx, mode0, inputs, per_row, 16, 11 + CASES.index((mode0, coded, per_row))))


def test_rows_from_the_gather_image_keep_the_bits_at_the_default_piece(B, ctx):
    inputs = _inputs(4200, 0, [2000, 513, 129, 128, 5, 0, 300], 7, 300, 2, True)
    _compare(_run(B, ctx, 0, inputs, False, 128, 40))


def test_another_dimension_takes_no_image(B, ctx):
    """D = 24 keeps its own gathers: the launch runs, K1c takes every row, and the image counters do not move"""
    from test_gpu_rows import _dev_terms, _run_rows
    rng = np.random.default_rng(4300)
    dims, Dn = [40, 30], 24
    ids = np.stack([rng.integers(1, d + 1, 900) for d in dims], axis=1).astype(np.int64)
    vals = rng.standard_normal(900)
    dr = B.DeviceRelation(ctx, B.IndexedDF((ids, vals), dims))
    f_t, Lam_t, mu_t = ctx.tensor(rng.standard_normal((dims[1], Dn))), ctx.tensor(np.eye(Dn) * 2.0), ctx.tensor(np.zeros(Dn))
    terms = _dev_terms(B, ctx, [(dr, 0, 1.5, 0.0, [None, f_t], None)])
    ctx.set_lowrank(0, 0)
    try:
        before = ctx.gather_image_stats()
        out_t = ctx.zeros(dims[0], Dn)
        _run_rows(B, ctx, Dn, dims[0], terms, mu_t, Lam_t, 8, out_t)
        d = ctx.rows_dispatch(8)
        assert d["col"] == dims[0] and d["k1"] == 0, d
        assert ctx.gather_image_stats() == before
        assert np.isfinite(out_t.cpu().numpy()).all()
    finally:
        ctx.set_lowrank(-1, 8192)
    dr.close()
