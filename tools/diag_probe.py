"""The cost of the convergence diagnostics (setDiagnostics) on MovieLens-1M's 500,000 test pairs (the bench's
split) at D = 32 with 200 draws kept -- a plane of 200 x 500,001 doubles, 800 MB:

- a whole macau() iteration with the push behind it and without, `rounds` blocks of each in turn (min - max over the blocks), by the
  host clock around a block, synchronised at both ends, after the engine's device warm-up; the blocks with the push fill the plane
  with real posterior draws of a Gaussian chain 20 iterations in;
- the push alone beside bdf_predict (the gather alone) and bdf_pairs_lpd_update (phase 2) on the same pairs, device events around
  `reps` launches after `warmup`, the three in turn `rounds` times (min - max);
- bdf_diag_compute on the filled plane, without and with the three columns in turn, `rounds` times (min - max), and what it found.

Reads only the bundled data.  Prints one JSON line per figure.

    python tools/diag_probe.py [--draws 200] [--rounds 5] [--reps 40] [--warmup 10] [--D 32]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from interval_probe import timed  # noqa: E402
from lpd_probe import ratings  # noqa: E402


def span(v):
    return {"min": round(min(v), 1), "max": round(max(v), 1), "each": [round(x, 1) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--D", type=int, default=32)
    args = ap.parse_args()
    import torch
    import bdf_amd as B
    from bdf_amd.engine import DIAG_STATS, DeviceDiag
    D, block = args.D, args.draws // args.rounds
    rd = ratings(B)
    rel = rd.relations[0]
    eng = B.GibbsEngine(rd, D, seed=0)
    eng.register_test((), rel.class_cut)
    for i in range(1, 21):
        eng.step(i, 0, (), rel.class_cut)
    eng.sync()
    eng.warm_device(50.0)
    test = eng.test_pairs()
    mean, alpha = rel.model.mean_value, rel.model.alpha
    diag = DeviceDiag(test.ctx, test.n, 1, block * args.rounds)
    print(json.dumps({"what": "plane", "draws": diag.capacity, "cells": test.n, "scalars": 1, "bytes": diag.capacity * (test.n + 1) * 8}), flush=True)

    # ---- a whole iteration, with the push and without
    it, per = 21, {"plain": [], "diag": []}
    for _ in range(args.rounds):
        for name in ("plain", "diag"):
            eng.sync()
            t0 = time.perf_counter()
            for i in range(it, it + block):
                eng.step(i, 2, (), rel.class_cut)
                if name == "diag":
                    diag.push(test, D, eng.factors_of(rel), mean, alpha)
            eng.sync()
            per[name].append((time.perf_counter() - t0) * 1e6 / block)
            it += block
    for name, v in per.items():
        print(json.dumps({"what": "iteration_" + name, "D": D, "iterations_per_block": block, "us_per_iteration": span(v)}), flush=True)

    # ---- the push alone, beside the gather alone and the lpd update
    ctx, facs = test.ctx, eng.factors_of(rel)
    out = ctx.zeros(test.n)
    test.lpd_update(D, facs, mean, alpha, 1)
    alone = {"predict": [], "lpd_update": [], "push": []}
    for _ in range(args.rounds):
        side = DeviceDiag(ctx, test.n, 1, args.reps + args.warmup)
        from bdf_amd._lib import check, lib
        from bdf_amd.engine import _facs, _ptr
        alone["predict"].append(timed(torch, ctx.stream, args.reps, args.warmup,
                                      lambda: check(lib().bdf_predict(ctx.handle, test.handle, D, _facs(facs), mean, _ptr(out)))))
        alone["lpd_update"].append(timed(torch, ctx.stream, args.reps, args.warmup, lambda: test.lpd_update(D, facs, mean, alpha, 2)))
        alone["push"].append(timed(torch, ctx.stream, args.reps, args.warmup, lambda: side.push(test, D, facs, mean, alpha)))
        side.close()
    for name, v in alone.items():
        print(json.dumps({"what": name + "_alone", "D": D, "pairs": test.n, "us_per_call": span(v)}), flush=True)

    # ---- the end of the run
    took = {False: [], True: []}
    for _ in range(args.rounds):
        for pointwise in (False, True):
            ctx.sync()
            t0 = time.perf_counter()
            stats, cols = diag.compute(1.1, 100.0, pointwise, test._order)
            ctx.sync()
            took[pointwise].append((time.perf_counter() - t0) * 1e6)
    for pointwise, v in took.items():
        print(json.dumps({"what": "compute", "pointwise": pointwise, "draws": diag.capacity, "cells": test.n, "us": span(v)}), flush=True)
    st = stats.cpu().numpy()
    found = dict(zip(DIAG_STATS, (float(x) for x in st)))
    found["sse"] = dict(zip(("rhat", "ess", "mcse"), (float(x) for x in st[len(DIAG_STATS):])))
    print(json.dumps({"what": "found", **found}), flush=True)
    diag.close()
    eng.close()


if __name__ == "__main__":
    main()
