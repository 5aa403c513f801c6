"""The cost of top-K lists (setRecommend) on MovieLens-1M as implicit data, the configuration of
tools/background_probe.py: the ratings of 4 and 5 are the listed cells and all hold 1, setBackground(rel, c0), D = 32, K = 10.
Five engines on the same data take turns, `rounds` times, and the median round is reported beside all of them:

    background        the iteration alone
    recommend_b1/8/32 the iteration and bdf_scores_push behind it, the ring `batch` = 1, 8, 32 draws deep (a full ring: one accumulate launch)
    full_prediction   the iteration and what macau(full_prediction=True) does behind it: bdf_predict_all into a temporary N x M matrix,
                      added to the running one by a torch op

Whole iterations by the host clock around `iters` of them, synchronised at both ends, after the engine's device warm-up.  Then, by
device events around single launches: the accumulate launch with 1, 8 and 32 draws buffered, the push, the top-K launch and the
metrics launch; the bytes read back; and recall@K, NDCG@K and the hit rate after burnin + psamples iterations with and without the
background.  One JSON line per figure.

    python tools/recommend_probe.py [--D 32] [--K 10] [--c0 0.1] [--alpha 10] [--rounds 5] [--iters 96]
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

from background_probe import implicit_movielens, relation_data  # noqa: E402


def event_us(torch, stream, reps, before, fn):
    """the median over `reps` of the device time of fn() alone, `before` (untimed) run in front of each"""
    out = []
    for _ in range(reps):
        before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--D", type=int, default=32)
    ap.add_argument("--K", type=int, default=10)
    ap.add_argument("--c0", type=float, default=0.1)
    ap.add_argument("--alpha", type=float, default=10.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=96)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--burnin", type=int, default=20)
    ap.add_argument("--psamples", type=int, default=20)
    args = ap.parse_args()
    import torch
    import bdf_amd as B
    from bdf_amd.engine import DeviceScores
    D, K, c0 = args.D, args.K, args.c0
    N, M, ids, test, tv, source = implicit_movielens()
    ones = np.ones(len(ids))
    print(json.dumps({"what": "data", "source": source, "N": N, "M": M, "listed": len(ids), "cells": N * M, "test": len(test), "D": D, "K": K,
                      "c0": c0, "alpha": args.alpha, "sum_bytes": N * M * 8, "derived_flush_bytes": 16 * N * M,
                      "derived_flops_per_draw": 2 * D * N * M}), flush=True)
    batches = {"recommend_b1": 1, "recommend_b8": 8, "recommend_b32": 32}
    engines, at, extra, scores = {}, {}, {}, {}
    for name in ["background", *batches, "full_prediction"]:
        rd = relation_data(B, N, M, ids, ones, test, tv, args.alpha, background=c0)
        rel = rd.relations[0]
        if name in batches:
            B.setRecommend(rel, K, batch=batches[name])
        eng = B.GibbsEngine(rd, D, seed=0)
        eng.register_test((), rel.class_cut)
        for i in range(1, 4):
            eng.step(i, 0, (), rel.class_cut)
        eng.sync()
        eng.warm_device(50.0)
        engines[name], at[name] = (eng, rel), 4
        if name in batches:
            # (macau()'s Recommend summary builds the sum for a run; the probe builds its own on the engine's row context)
            scores[name] = DeviceScores(eng.ctx, N, M, D, batches[name])
            extra[name] = lambda eng=eng, rel=rel, sc=scores[name]: sc.push(*eng.factors_of(rel))
        elif name == "full_prediction":
            yhat = torch.zeros((N, M), dtype=torch.float64, device=eng.ctx.device)

            def add(eng=eng, rel=rel, yhat=yhat):
                yhat.add_(eng.pred_all(rel))
            extra[name] = add
        else:
            extra[name] = lambda: None
    per = {name: [] for name in engines}
    for _ in range(args.rounds):
        for name, (eng, rel) in engines.items():
            eng.sync()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(at[name], at[name] + args.iters):
                eng.step(i, 0, (), rel.class_cut)
                extra[name]()
            eng.sync()
            torch.cuda.synchronize()
            per[name].append((time.perf_counter() - t0) * 1e6 / args.iters)
            at[name] += args.iters
    med = {name: float(np.median(v)) for name, v in per.items()}
    for name, v in per.items():
        print(json.dumps({"what": "iteration", "model": name, "us_median": round(med[name], 1), "us_rounds": [round(x, 1) for x in v]}), flush=True)
    print(json.dumps({"what": "iteration_extra_us", **{name: round(med[name] - med["background"], 1) for name in med if name != "background"},
                      "b8_per_round_not_above_full_prediction": [bool(a <= b) for a, b in zip(per["recommend_b8"], per["full_prediction"])]}), flush=True)
    # single launches by device events
    eng, rel = engines["recommend_b32"]
    sc, ctx = scores["recommend_b32"], eng.ctx
    facs = eng.factors_of(rel)
    sc.flush()
    parts = {"what": "launches_us", "push": round(event_us(torch, ctx.stream, args.reps, sc.flush, lambda: sc.push(*facs)), 1)}
    for held in (1, 8, 32):
        def fill(held=held):
            sc.flush()
            for _ in range(held - (1 if held == 32 else 0)):
                sc.push(*facs)
        # (a ring of 32: the 32nd push flushes, so it is timed with its flush and the push's own time taken off)
        if held == 32:
            parts["flush_32_draws"] = round(event_us(torch, ctx.stream, args.reps, fill, lambda: sc.push(*facs)) - parts["push"], 1)
        else:
            parts[f"flush_{held}_draw{'s' if held > 1 else ''}"] = round(event_us(torch, ctx.stream, args.reps, fill, sc.flush), 1)
    got = {}
    parts["topk"] = round(event_us(torch, ctx.stream, args.reps, lambda: None,
                                   lambda: got.__setitem__("lists", sc.topk(K, rel.model.mean_value, rel._dev))), 1)
    pairs = eng.test_pairs()
    sc.metrics(got["lists"][0], K, pairs, rel.class_cut)          # (the first call indexes the relevant cells on the host)
    parts["metrics"] = round(event_us(torch, ctx.stream, args.reps, lambda: None, lambda: sc.metrics(got["lists"][0], K, pairs, rel.class_cut)), 1)
    parts["bytes_read_back"] = N * K * (4 + 8) + 4 * 8
    parts["bytes_read_back_full_prediction"] = N * M * 8
    print(json.dumps(parts), flush=True)
    for e, _ in engines.values():
        e.close()
    # what the lists are worth: recall@K, NDCG@K and hit rate with and without the background
    for name in ("background", "listed"):
        rd = relation_data(B, N, M, ids, ones, test, tv, args.alpha, background=c0 if name == "background" else None)
        B.setRecommend(rd.relations[0], K)
        res = B.macau(rd, num_latent=D, burnin=args.burnin, psamples=args.psamples, verbose=False, seed=0)
        r = res["recommend"]
        print(json.dumps({"what": "held_out", "model": name, "recall": round(r["recall"], 4), "ndcg": round(r["ndcg"], 4), "hit_rate": round(r["hit_rate"], 4),
                          "rows_scored": r["rows_scored"], "AUC": round(float(res["ROC"]), 4), "burnin": args.burnin, "psamples": args.psamples}), flush=True)
        rd._engine.close()


if __name__ == "__main__":
    main()
