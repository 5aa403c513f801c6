"""Whole native iterations with K1c's gather image on against off (bdf_ctx_set_gather_image): a 300 x 200 relation of about 6,000
training cells and 2,000 test pairs at D = 32, six iterations with the prediction update.  The image only changes where the row
kernel's operands come from, so every entity's sample, mu and Lambda, the test pairs' running mean and sum of squares and the
reporting statistics are EQUAL -- also when the chain's state is put back between iterations 3 and 4 (bdf_gibbs_warm_device) and
when the host writes one entity's sample there (GibbsEngine.sample_written): both leave an image stale, and the next launch that
gathers it packs it anew.  The counters say that it did, and that every other launch took the image its predecessor left.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N1, N2, D, NNZ, NTEST, SWEEPS = 300, 200, 32, 8000, 2000, 6
CLAMP, CUT = [1.0, 5.0], 2.5


def _chain(B, switch, variant):
    import torch
    rng = np.random.default_rng(5)
    ids = np.stack([rng.integers(1, N1 + 1, NNZ), rng.integers(1, N2 + 1, NNZ)], axis=1)
    U, V = rng.standard_normal((N1, 3)), rng.standard_normal((N2, 3))
    vals = np.clip(3.0 + np.sum(U[ids[:, 0] - 1] * V[ids[:, 1] - 1], axis=1) + 0.1 * rng.standard_normal(NNZ), 1.0, 5.0)
    rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": vals}, "r", [B.Entity("u"), B.Entity("v")], dims=[N1, N2])
    B.assignToTest(rel, np.arange(1, NTEST + 1))
    B.setPrecision(rel, 2.0)
    rd = B.RelationData(rel)
    eng = B.GibbsEngine(rd, D, seed=42)
    assert eng.native
    eng.ctx.set_gather_image(switch)
    test = eng.test_pairs()
    eng.register_test(CLAMP, CUT)
    for i in range(1, SWEEPS + 1):
        if i == 4 and variant == "warm":
            eng.warm_device(3.0)
        if i == 4 and variant == "write":
            eng.sync()
            eng.ent[1].sample.mul_(0.5)
            torch.cuda.synchronize()
            eng.sample_written(1)
        eng.step(i, 1 if i == 1 else 2, CLAMP, CUT)
    eng.sync()
    out = {}
    for j, st in enumerate(eng.ent):
        assert eng.rows_dispatch(j)["col"] == st.N, eng.rows_dispatch(j)
        for k in ("sample", "mu", "Lambda"):
            out["%s%d" % (k, j)] = np.array(st.host(k), dtype=np.float64)
    avg, sq = test.state()
    out["test_pred_mean"], out["test_pred_sumsq"] = np.array(avg), np.array(sq)
    out["test_stats"] = test.stats.cpu().numpy().astype(np.float64)
    stats = eng.ctx.gather_image_stats()
    eng.close()
    return out, stats


@pytest.fixture(scope="module")
def plain_off(B):
    return _chain(B, 0, "plain")


def _equal(a, b):
    assert sorted(a) == sorted(b)
    for k in sorted(a):
        assert np.isfinite(a[k]).all(), k
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (k, float(np.max(np.abs(a[k] - b[k]))))


def test_iterations_with_the_image_keep_the_bits(B, plain_off):
    off, stats_off = plain_off
    on, stats = _chain(B, 1, "plain")
    _equal(on, off)
    assert stats_off == {"launches": 0, "packs": 0, "left": 0}, stats_off
    # the first launch of the chain packs the opposite entity's initial sample; every later one takes the image its predecessor left
    assert stats == {"launches": 2 * SWEEPS, "packs": 1, "left": 2 * SWEEPS}, stats
    assert np.abs(off["sample0"]).max() > 0 and not np.array_equal(off["test_pred_mean"], np.zeros(NTEST))


def test_iterations_with_the_full_image_keep_the_bits(B, plain_off):
    on, stats = _chain(B, 2, "plain")
    _equal(on, plain_off[0])
    assert stats == {"launches": 2 * SWEEPS, "packs": 1, "left": 2 * SWEEPS}, stats


def test_a_state_put_back_makes_the_image_anew(B):
    off, _ = _chain(B, 0, "warm")
    on, stats = _chain(B, 1, "warm")
    _equal(on, off)
    assert stats["packs"] == 2 and stats["launches"] == stats["left"] > 2 * SWEEPS, stats


def test_a_sample_the_host_wrote_makes_the_image_anew(B, plain_off):
    off, _ = _chain(B, 0, "write")
    on, stats = _chain(B, 1, "write")
    _equal(on, off)
    assert not np.array_equal(off["sample0"], plain_off[0]["sample0"])          # (the write took effect)
    assert stats == {"launches": 2 * SWEEPS, "packs": 2, "left": 2 * SWEEPS}, stats
