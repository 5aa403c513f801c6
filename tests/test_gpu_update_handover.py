"""The hand-over of the rows to the sweep's prediction update without an event on the row dispatch (bdf_gibbs_sweep): when the last
entity's launch went out by the done counters, the prediction stream waits for a one-wave gate kernel that polls those counters
on the reserved CUs (k_rows_gate) instead of an event carried by the row launch.  A small BPMF engine whose launches all take K1c
-- every row has more observations than the low-rank sampler takes, so the counter hand-over is what runs, and rows_dispatch says
so -- makes 9 native iterations back to back, three full rotations of the row buffers and more than the host's lag of three
prediction updates, with no host synchronisation between them, and is compared bit for bit with the same chain under a full sync()
after every iteration: every entity's sample, mu and Lambda, the test pairs' running state and the statistics.  The back-to-back
run is made twice.  One case attaches a caller's timing events to every row launch, a path that keeps the event on the dispatch.

Every wait has a time limit: before iteration i the host polls an event of its own behind the prediction update of i - 3 -- the
wait the library makes there itself -- and at the end one event per stream; a hand-over that never completes fails the test.
"""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N1, N2, NNZ, SEED = 300, 200, 6000, 17
ITERS, LAG, LIMIT_S = 9, 3, 30.0
CLAMP, CUT = [1.0, 5.0], 3.0


def _data(ntest):
    """6,000 training ratings, 20 a user and 20 .. 40 a movie (user u rates movies u + 7 k mod 200: no row short enough for the
    low-rank sampler at D = 32, which takes rows of up to 16), and ntest random test pairs behind them"""
    rng = np.random.default_rng(100 + ntest)
    u = np.repeat(np.arange(N1), NNZ // N1)
    m = (u + 7 * np.tile(np.arange(NNZ // N1), N1)) % N2
    assert np.bincount(u, minlength=N1).min() > 16 and np.bincount(m, minlength=N2).min() > 16
    tu, tm = rng.integers(0, N1, ntest), rng.integers(0, N2, ntest)
    U, V = rng.standard_normal((N1, 3)), rng.standard_normal((N2, 3))
    uu, mm = np.concatenate([u, tu]), np.concatenate([m, tm])
    y = np.clip(np.round(3.0 + np.sum(U[uu] * V[mm], axis=1) + 0.3 * rng.standard_normal(uu.size)), 1, 5)
    return uu + 1, mm + 1, y


def _wait(torch, ev, what):
    t0 = time.perf_counter()
    while not ev.query():
        if time.perf_counter() - t0 > LIMIT_S:
            pytest.fail("%s did not complete within %.0f s" % (what, LIMIT_S))


def _run(B, D, ntest, back_to_back, timed=False):
    import torch
    from bdf_amd.engine import GibbsEngine
    u, m, y = _data(ntest)
    rel = B.Relation({"u": u, "v": m, "y": y}, "r", [B.Entity("u"), B.Entity("v")], dims=[N1, N2])
    B.setPrecision(rel, 1.5)
    B.assignToTest(rel, np.arange(NNZ + 1, NNZ + ntest + 1))
    rd = B.RelationData(rel)
    eng = GibbsEngine(rd, D, seed=SEED)
    assert eng.native
    eng.register_test(CLAMP, CUT)
    if timed:
        eng.k1_events, eng.k1_event_every = [], 1          # a caller's timing pair on every row launch: the event stays on the dispatch
    behind = []                                            # an event of the host's own behind every iteration's prediction update
    for i in range(1, ITERS + 1):
        if back_to_back and i > LAG:
            _wait(torch, behind[i - 1 - LAG], "the prediction update of iteration %d" % (i - LAG))
        eng.step(i, 0 if i < 3 else (1 if i == 3 else 2), CLAMP, CUT)
        ev = torch.cuda.Event()
        ev.record(eng.ctx_p.stream)
        behind.append(ev)
        if not back_to_back:
            for ctx, what in ((eng.ctx_p, "prediction"), (eng.ctx_h, "hyperprior"), (eng.ctx, "row")):
                e = torch.cuda.Event()
                e.record(ctx.stream)
                _wait(torch, e, "the %s stream of iteration %d" % (what, i))
            eng.sync()
    for ctx, what in ((eng.ctx_p, "prediction"), (eng.ctx_h, "hyperprior"), (eng.ctx, "row")):
        e = torch.cuda.Event()
        e.record(ctx.stream)
        _wait(torch, e, "the %s stream" % what)
    eng.sync()
    for j in (0, 1):
        d = eng.rows_dispatch(j)
        assert d["col"] == (N1, N2)[j] and d["lowrank"] == 0 and d["small"] == 0 and d["k1"] == 0, d      # K1c alone: the counters' launch
    if timed:
        assert len(eng.k1_events) == 2 * ITERS
    out = []
    for en in rd.entities:
        out += [en.model.sample.copy(), en.model.mu.copy(), en.model.Lambda.copy()]
    out += list(eng.test_pairs().state()) + [eng.test_pairs().stats.cpu().numpy().copy()]
    eng.close()
    return out


def _same(a, b):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        np.testing.assert_array_equal(x, y, err_msg="output %d" % k)


@pytest.mark.parametrize("ntest", [1, 129, 2000])
@pytest.mark.parametrize("D", [32, 20])
def test_back_to_back_iterations_equal_the_synchronised_chain(B, D, ntest):
    ref = _run(B, D, ntest, back_to_back=False)
    assert np.all(np.isfinite(ref[-1])) and ref[-1][1] > 0.0 and np.any(ref[-3] != 0.0)       # (the update ran: statistics and state)
    one = _run(B, D, ntest, back_to_back=True)
    _same(ref, one)
    _same(one, _run(B, D, ntest, back_to_back=True))


def test_a_timed_launch_keeps_its_event_and_the_chain(B):
    """bdf_gibbs_time_rows on every launch: `counter` is false for it, the row dispatch carries the caller's stop event and the
    prediction stream waits for that -- the same chain"""
    ref = _run(B, 32, 129, back_to_back=False)
    _same(ref, _run(B, 32, 129, back_to_back=True, timed=True))
