"""The sweep's prediction update as single-wave workgroups (k_update_runs.hip): workgroup w takes the pairs that wave w & 3 of the
former 256-lane workgroup w >> 2 took and leaves its four sums per WAVE; k_update_waves_final adds the four waves of a former
workgroup left to right and goes on as k_predict_final does.  Nothing of the order of operations changed, so the reference is
the NumPy model of tests/test_gpu_predict_fit.py as it stands (imported, not copied) and the tolerance is 0 on the running mean,
the sum of squares and all four statistics, through bdf_predict_update, phases 1, 2, 2.  k_predict_runs' raw predictions of the
same sorted pairs (bdf_predict) are held to the model's dot products as well.

Sizes: the edges of a lane group (8 pairs), of a wave (128 pairs: 8 groups of 16), of the former workgroup (512) and of the final
kernel's new level (a former workgroup with one, two, three or four waves that hold pairs); 512 x 256 + 1 pairs for the second
trip of the final kernel's stride loop.  Every size runs twice: with random ids, and with ids whose runs of one sorted-mode id
cross every wave boundary -- srow and cur are per group of 8 lanes, so where a run is cut must not matter.
"""
import functools

import numpy as np
import pytest

from test_gpu_predict_fit import MEAN, _check, _dots

pytestmark = pytest.mark.gpu

WAVE = 128                         # pairs per wave: 8 groups of 8 lanes, 16 pairs each
SIZES = [(n, 32) for n in (0, 1, 7, 8, 9, 127, 128, 129, 511, 512, 513, 1025)] + [(513, 4), (513, 20)]
N_SECOND_TRIP = 512 * 256 + 1


def _crossing_ids(n, mode, rng):
    """pairs already sorted by `mode`: runs of 23 pairs of one id, the first cut to 18 -- a run ends at 18, 41, 64, ..., so that no
    multiple of 128 up to 1,152 is the end of a run and every wave boundary inside the pairs falls INSIDE a run"""
    key = (np.arange(n) + 5) // 23 + 1
    for b in range(WAVE, min(n, 1153), WAVE):
        assert key[b - 1] == key[b], b
    ids = np.empty((n, 2), dtype=np.int64)
    ids[:, mode], ids[:, 1 - mode] = key, rng.integers(1, 12, n)
    return ids, int(key.max()) if n else 1


def _raw(B, ctx, ids, facs, D, mode):
    """k_predict_runs' raw path on the same sorted pairs: the predictions in the caller's order are the model's dot products + mean"""
    if ids.shape[0] == 0:
        return
    srt = B.DevicePairs(ctx, ids, np.zeros(ids.shape[0])).sort(mode)
    raw = srt.predict(D, [ctx.tensor(f.copy()) for f in facs], MEAN).cpu().numpy()
    np.testing.assert_array_equal(raw, _dots(ids - 1, facs, D) + MEAN)
    srt.close()


@functools.lru_cache(maxsize=None)
def _case(n, D):
    rng = np.random.default_rng(1000 * D + n)
    mode = n % 2                                           # both modes over the sizes
    dims = [37, 11]
    rnd = np.stack([rng.integers(1, d + 1, n) for d in dims], axis=1).astype(np.int64).reshape(n, 2)
    rnd_facs = [rng.standard_normal((d, D)) * 0.7 for d in dims]
    cross, rows = _crossing_ids(n, mode, rng)
    cross_facs = [None, None]
    cross_facs[mode], cross_facs[1 - mode] = rng.standard_normal((rows, D)) * 0.7, rng.standard_normal((11, D)) * 0.7
    return mode, (rnd, rng.standard_normal(n) + 3.0, rnd_facs), (cross, rng.standard_normal(n) + 3.0, cross_facs)


@pytest.mark.parametrize("n,D", SIZES)
def test_single_wave_update_equals_the_model(B, ctx, n, D):
    mode, rnd, cross = _case(n, D)
    for ids, y, facs in (rnd, cross):
        _check(B, ctx, ids, y, facs, D, mode)
        _raw(B, ctx, ids, facs, D, mode)


def test_final_kernel_takes_a_second_trip(B, ctx):
    """257 former workgroups = 1,028 waves' sums: partial 256 is added by lane 0 of the final kernel in its second trip, after its
    four waves (of which one holds a pair) were added left to right; the ids' runs cross wave boundaries here too"""
    mode, _, (ids, y, facs) = _case(N_SECOND_TRIP, 32)
    _check(B, ctx, ids, y, facs, 32, mode)
