"""The cost of acquisition lists (setAcquire) at the MovieLens-1M shape (6040 x 3706, D = 32).  Every figure is the
minimum and the maximum over `rounds` (30) runs in which the candidates take turns, so that whatever else the machine does falls on all
of them alike:

    flush      bdf_acquire_flush of 8 buffered draws, per draw, with and without the psum plane, against bdf_scores_flush of the same
               8 draws (the yardstick: one plane, no fold), by device events around the one launch; the bytes each moves per draw
               (planes read and written once per flush, the ring read once) and what they come to over the measured time
    lists      bdf_acquire_topk (the score plane, k_topk_rows on it, the gather) per rule, against bdf_scores_topk (k_topk_rows alone)
    iteration  a whole iteration of MovieLens-1M as implicit data (tools/background_probe.py) by the host clock around `iters` of
               them, with the option (the push behind every iteration, batch 8) and without

One JSON line per figure.

    python tools/acquire_probe.py [--D 32] [--K 10] [--rounds 30] [--iters 48]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

N_ML, M_ML, BATCH = 6040, 3706, 8


def flush_bytes_per_draw(N, M, D, planes, held=BATCH):
    """bytes one flush of `held` draws moves, per draw: every plane read and written once, the ring's factors read once"""
    return (2 * planes * N * M * 8) / held + (N + M) * 4 * ((D + 3) // 4) * 8


def event_us(torch, stream, before, fn):
    before()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def span(xs):
    return {"min": round(float(np.min(xs)), 1), "max": round(float(np.max(xs)), 1), "median": round(float(np.median(xs)), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--D", type=int, default=32)
    ap.add_argument("--K", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--iters", type=int, default=48)
    ap.add_argument("--no-iteration", action="store_true")
    args = ap.parse_args()
    import torch
    import bdf_amd as B
    from bdf_amd.engine import Context, DeviceAcquire, DeviceScores
    D, K, N, M = args.D, args.K, N_ML, M_ML
    ctx = Context()
    rng = np.random.default_rng(0)
    draws = [(ctx.tensor(rng.standard_normal((N, D)) * 0.3), ctx.tensor(rng.standard_normal((M, D)) * 0.3)) for _ in range(BATCH)]
    # rings of 16 slots: 8 pushes do not flush by themselves
    cands = {"acquire_prob": DeviceAcquire(ctx, N, M, D, 2 * BATCH, None, 3.5, 4.0), "acquire": DeviceAcquire(ctx, N, M, D, 2 * BATCH, None, 3.5),
             "scores": DeviceScores(ctx, N, M, D, 2 * BATCH)}
    planes = {"acquire_prob": 3, "acquire": 2, "scores": 1}

    def fill(name):
        c = cands[name]
        c.flush()
        for U, V in draws:
            c.push(U, V, 2.0) if name != "scores" else c.push(U, V)
    for name in cands:                                       # warm-up: code objects, clocks
        for _ in range(3):
            fill(name)
            cands[name].flush()
    ctx.sync()
    per = {name: [] for name in cands}
    for _ in range(args.rounds):
        for name, c in cands.items():
            per[name].append(event_us(torch, ctx.stream, lambda: fill(name), c.flush) / BATCH)
    for name, v in per.items():
        nbytes = flush_bytes_per_draw(N, M, D, planes[name])
        print(json.dumps({"what": "flush_us_per_draw", "model": name, **span(v), "bytes_per_draw": int(nbytes),
                          "TB_per_s_at_min": round(nbytes / (min(v) * 1e-6) / 1e12, 2), "TB_per_s_at_max": round(nbytes / (max(v) * 1e-6) / 1e12, 2)}), flush=True)
    lists = {"ucb": [], "sd": [], "prob_above": [], "scores_topk": []}
    for _ in range(args.rounds):
        for rule in ("ucb", "sd", "prob_above"):
            lists[rule].append(event_us(torch, ctx.stream, lambda: None, lambda: cands["acquire_prob"].topk(K, rule, 1.0)))
        lists["scores_topk"].append(event_us(torch, ctx.stream, lambda: None, lambda: cands["scores"].topk(K, 3.5)))
    for name, v in lists.items():
        print(json.dumps({"what": "lists_us", "model": name, "K": K, **span(v), "bytes_read_back": N * K * (4 + 8 * (4 if name == "prob_above" else 3))}), flush=True)
    for c in cands.values():
        c.close()
    if args.no_iteration:
        return
    from background_probe import implicit_movielens, relation_data
    N, M, ids, test, tv, source = implicit_movielens()
    engines, at, acq = {}, {}, {}
    for name in ("plain", "acquire_b8"):
        rd = relation_data(B, N, M, ids, np.ones(len(ids)), test, tv, 10.0, background=0.1)
        rel = rd.relations[0]
        if name != "plain":
            B.setAcquire(rel, K, rule="prob_above", threshold=0.5, batch=BATCH)
        eng = B.GibbsEngine(rd, D, seed=0)
        eng.register_test((), rel.class_cut)
        for i in range(1, 4):
            eng.step(i, 0, (), rel.class_cut)
        eng.sync()
        eng.warm_device(50.0)
        # (macau()'s Acquire summary builds the planes for a run; the probe builds its own on the engine's row context)
        acq[name] = DeviceAcquire(eng.ctx, N, M, D, BATCH, None, rel.model.mean_value, 0.5) if name != "plain" else None
        engines[name], at[name] = (eng, rel), 4
    per = {name: [] for name in engines}
    for _ in range(args.rounds):
        for name, (eng, rel) in engines.items():
            eng.sync()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(at[name], at[name] + args.iters):
                eng.step(i, 0, (), rel.class_cut)
                if acq[name] is not None:
                    acq[name].push(*eng.factors_of(rel), rel.model.alpha)
            eng.sync()
            torch.cuda.synchronize()
            per[name].append((time.perf_counter() - t0) * 1e6 / args.iters)
            at[name] += args.iters
    for name, v in per.items():
        print(json.dumps({"what": "iteration_us", "model": name, "source": source, "N": N, "M": M, "D": D, **span(v)}), flush=True)
    for e, _ in engines.values():
        e.close()


if __name__ == "__main__":
    main()
