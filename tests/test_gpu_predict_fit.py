"""The sweep's prediction update on sorted pairs (k_update_runs.hip) against the general kernel (k_predict) and against a NumPy
evaluation in the kernels' own order of operations.  The order is specified -- per-lane products (x x + y y) + (z z + w w), the
xor 4, 2, 1 sums, pair_finish's formulas, 512 pairs per partial (256 for the general kernel), block_stats' and k_predict_final's
trees -- so the tolerance is 0: equality is the test.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NS = (1, 7, 8, 9, 15, 16, 17, 511, 512, 513, 1031)
MEAN, CLAMP, CUT = 0.4, (2.0, 4.0), 3.0


def _butterfly(v, offs):
    """v[lane] += v[lane ^ off] for every off in turn, over the last axis (every lane ends with the same bits: + commutes)"""
    idx = np.arange(v.shape[-1])
    for off in offs:
        v = v + v[..., idx ^ off]
    return v[..., 0]


def _dots(ids0, facs, D):
    """udot of every pair in the kernels' order: 8 lanes of 4 elements, lanes beyond D / 4 hold 0"""
    a, b = facs[0][ids0[:, 0]], facs[1][ids0[:, 1]]
    pad = np.zeros((a.shape[0], 32))
    pr = pad.copy()
    pr[:, :D] = a * b
    pr = pr.reshape(-1, 8, 4)
    lane = (pr[:, :, 0] + pr[:, :, 1]) + (pr[:, :, 2] + pr[:, :, 3])
    return _butterfly(lane, (4, 2, 1))


def _clamp(x):
    return np.minimum(np.maximum(x, CLAMP[0]), CLAMP[1])


def _stats(terms, per_lane):
    """terms: (n, 4) in STORAGE order; a lane of workgroup b owns `per_lane` pairs, 8 apart in its group's run of 8 per_lane pairs:
    the lane's sum in that order, the wave's butterfly, the workgroup's four waves left to right, then k_predict_final's tree"""
    n = terms.shape[0]
    per_block = 256 * per_lane
    nblocks = (n + per_block - 1) // per_block
    t = np.zeros((nblocks * per_block, 4))
    t[:n] = terms
    ok = np.arange(nblocks * per_block) < n
    t = t.reshape(nblocks, 32, per_lane, 8, 4)             # block, group, q, sub, statistic
    ok = ok.reshape(nblocks, 32, per_lane, 8)
    st = np.zeros((nblocks, 32, 8, 4))
    for q in range(per_lane):
        st = np.where(ok[:, :, q, :, None], st + t[:, :, q], st)
    st = st.reshape(nblocks, 4, 64, 4).transpose(0, 1, 3, 2)          # block, wave, statistic, lane
    w = _butterfly(st, (32, 16, 8, 4, 2, 1))                           # block, wave, statistic
    partial = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]                # block, statistic
    v = np.zeros((256, 4))
    for b in range(nblocks):
        v[b % 256] = v[b % 256] + partial[b]
    w = _butterfly(v.reshape(4, 64, 4).transpose(0, 2, 1), (32, 16, 8, 4, 2, 1))
    return ((w[0] + w[1]) + w[2]) + w[3]


class _Model:
    """pair_finish over three updates, phases 1, 2, 2, in the caller's order"""

    def __init__(self, y):
        self.y, self.avg, self.sq, self.count = y, None, None, 0.0

    def update(self, dot, phase):
        p = dot + MEAN
        if phase == 1:
            self.avg, self.sq, self.count = p.copy(), p * p, 1.0
        else:
            self.avg = (self.count * self.avg + p) / (self.count + 1.0)
            self.sq = self.sq + p * p
            self.count += 1.0
        ea, ep = self.y - _clamp(self.avg), self.y - _clamp(p)
        label = self.y < CUT
        return np.stack([ea * ea, ep * ep, (label == (self.avg < CUT)) * 1.0, (label == (p < CUT)) * 1.0], axis=1)


def _check(B, ctx, ids, y, facs, D, mode):
    n = ids.shape[0]
    ft = [ctx.tensor(f.copy()) for f in facs]
    plain, srt = B.DevicePairs(ctx, ids, y), B.DevicePairs(ctx, ids, y).sort(mode)
    order = np.argsort(ids[:, mode], kind="stable")        # bdf_pairs_sort: stable by the mode's id
    np.testing.assert_array_equal(srt._order, order)
    model = _Model(y)
    f = [x.copy() for x in facs]
    for phase in (1, 2, 2):
        for k in (0, 1):
            ft[k].mul_(0.75)                               # (exact in binary: the host copy follows bit for bit)
            f[k] = f[k] * 0.75
        s_plain = plain.update(D, ft, MEAN, phase, list(CLAMP), CUT).cpu().numpy().copy()
        s_srt = srt.update(D, ft, MEAN, phase, list(CLAMP), CUT).cpu().numpy().copy()
        terms = model.update(_dots(ids - 1, f, D), phase)
        np.testing.assert_array_equal(s_srt, _stats(terms[order], 2), err_msg="sorted statistics n=%d phase=%d" % (n, phase))
        np.testing.assert_array_equal(s_plain, _stats(terms, 1), err_msg="general statistics n=%d phase=%d" % (n, phase))
        a1, q1 = plain.state()
        a2, q2 = srt.state()
        np.testing.assert_array_equal(a2, a1)
        np.testing.assert_array_equal(q2, q1)
        np.testing.assert_array_equal(a2, model.avg)
        np.testing.assert_array_equal(q2, model.sq)
    plain.close(); srt.close()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("D", [4, 20, 32])
def test_sorted_update_equals_the_general_kernel_and_the_model(B, ctx, D, mode):
    rng = np.random.default_rng(100 * D + mode)
    dims = [37, 11]
    facs = [rng.standard_normal((d, D)) * 0.7 for d in dims]
    for n in NS:
        ids = np.stack([rng.integers(1, d + 1, n) for d in dims], axis=1).astype(np.int64)
        y = rng.standard_normal(n) + 3.0
        _check(B, ctx, ids, y, facs, D, mode)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("D", [4, 20, 32])
def test_sorted_update_id_patterns(B, ctx, D, mode):
    """every pair the same sorted id; every pair a different one (the sorted mode's matrix then has a row per pair); an id change
    at each position of a 16-pair run (run r changes id after r pairs; the matrix of 37 rows is the sorted mode's)"""
    rng = np.random.default_rng(7 + 100 * D + mode)
    for n in NS:
        other = rng.integers(1, 12, n)
        for pattern in ("same", "different"):
            rows = 37 if pattern == "same" else max(37, n)
            key = np.full(n, 5) if pattern == "same" else rng.permutation(n) + 1
            ids = np.empty((n, 2), dtype=np.int64)
            ids[:, mode], ids[:, 1 - mode] = key, other
            facs = [None, None]
            facs[mode], facs[1 - mode] = rng.standard_normal((rows, D)) * 0.7, rng.standard_normal((11, D)) * 0.7
            _check(B, ctx, ids, rng.standard_normal(n) + 3.0, facs, D, mode)
    key = np.concatenate([[2 * r - 1] * r + [2 * r] * (16 - r) for r in range(1, 16)])      # sorted already: runs of 16 stay whole
    n = key.size
    ids = np.empty((n, 2), dtype=np.int64)
    ids[:, mode], ids[:, 1 - mode] = key, rng.integers(1, 12, n)
    facs = [None, None]
    facs[mode], facs[1 - mode] = rng.standard_normal((37, D)) * 0.7, rng.standard_normal((11, D)) * 0.7
    _check(B, ctx, ids, rng.standard_normal(n) + 3.0, facs, D, mode)
