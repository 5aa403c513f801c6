"""The cost of the interval-censored noise model on MovieLens-1M (the bench's 500,000-rating test split, so 500,209 training
pairs) at D = 32, with every rating r taken as the bin [r - 1/2, r + 1/2), open at both ends (setBinned([1.5, 2.5, 3.5, 4.5])):
microseconds of bdf_interval_draw, of bdf_censored_draw with every pair flagged and of bdf_predict on the same pairs (in the
caller's order and stored sorted by movie, as the engine stores them), and of one whole macau() iteration with the bins and
without them on the same data.  Kernels are timed with device events around `reps` launches after `warmup`; iterations by the host
clock around `iters` of them, synchronised at both ends, after the engine's device warm-up.  Reads only the bundled data.  Prints
one JSON line per figure.

    python tools/interval_probe.py [--reps 50] [--warmup 10] [--iters 200] [--D 32]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EDGES = [1.5, 2.5, 3.5, 4.5]


def ratings(B, binned):
    from bdf_amd import datasets
    d = datasets.load_movielens() if os.path.exists(datasets.MOVIELENS_PATH) else datasets.synthetic_movielens_like()
    X = d["X"]
    rel = B.Relation(X, "ratings", [B.Entity("users"), B.Entity("movies")])
    B.assignToTest(rel, datasets.split_test_ids(X.nnz, 500_000, 1))
    B.setPrecision(rel, 1.5)
    if binned:
        B.setBinned(rel, EDGES)
    return B.RelationData(rel)


def timed(torch, stream, reps, warmup, fn):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--D", type=int, default=32)
    args = ap.parse_args()
    import torch
    import bdf_amd as B
    from bdf_amd._lib import check, lib
    from bdf_amd.engine import DevicePairs
    D = args.D
    sweeps = {}
    for name, binned in (("binned", True), ("gaussian", False)):
        rd = ratings(B, binned)
        rel = rd.relations[0]
        eng = B.GibbsEngine(rd, D, seed=0)
        eng.register_test((), rel.class_cut)
        for i in range(1, 21):
            eng.step(i, 0, (), rel.class_cut)
        eng.sync()
        eng.warm_device(50.0)
        t0 = time.perf_counter()
        for i in range(21, 21 + args.iters):
            eng.step(i, 0, (), rel.class_cut)
        eng.sync()
        sweeps[name] = (time.perf_counter() - t0) * 1e6 / args.iters
        disp = [eng.rows_dispatch(j) for j in range(2)]
        print(json.dumps({"what": "sweep_" + name, "D": D, "us_per_iteration": round(sweeps[name], 1), "train_pairs": rel.data.nnz(),
                          "rows_dispatch": disp}), flush=True)
        if binned:
            ctx, facs = eng.ctx, eng.factors_of(rel)
            fp = (C.c_void_p * 2)(*[f.data_ptr() for f in facs])
            ids, vals = np.asarray(rel.data.ids), np.asarray(rel.data.values)
            lin, out = ctx.zeros(len(vals)), ctx.zeros(len(vals))
            mean = rel.model.mean_value
            bins = np.asarray(rel.model.interval)
            exact = np.stack([vals, vals], axis=1)
            flags = ctx.tensor(np.ones(len(vals), dtype=np.int8), dtype=torch.int8)
            ctx.set_sweep(1000)
            for order in ("caller", "sorted_by_movie"):
                pairs = DevicePairs(ctx, ids, vals)
                if order != "caller":
                    pairs.sort(1)
                row = {"what": "draw_vs_predict", "D": D, "pairs": len(vals), "order": order}
                for label, b in (("interval_draw_us", bins), ("interval_draw_none_bounded_us", exact)):
                    bd = ctx.tensor(b)
                    row[label] = round(timed(torch, ctx.stream, args.reps, args.warmup, lambda: check(lib().bdf_interval_draw(
                        ctx.handle, pairs.handle, C.c_void_p(bd.data_ptr()), D, fp, mean, 1.5, None, 1, C.c_void_p(lin.data_ptr()), None))), 2)
                row["censored_draw_all_flagged_us"] = round(timed(torch, ctx.stream, args.reps, args.warmup, lambda: check(lib().bdf_censored_draw(
                    ctx.handle, pairs.handle, C.c_void_p(flags.data_ptr()), D, fp, mean, 1.5, None, 1, C.c_void_p(lin.data_ptr()), None))), 2)
                row["predict_us"] = round(timed(torch, ctx.stream, args.reps, args.warmup, lambda: check(lib().bdf_predict(
                    ctx.handle, pairs.handle, D, fp, mean, C.c_void_p(out.data_ptr())))), 2)
                row["interval_over_censored_draw"] = round(row["interval_draw_us"] / row["censored_draw_all_flagged_us"], 2)
                row["interval_over_predict"] = round(row["interval_draw_us"] / row["predict_us"], 2)
                print(json.dumps(row), flush=True)
                pairs.close()
        eng.close()
    print(json.dumps({"what": "binned_over_gaussian_sweep", "D": D, "ratio": round(sweeps["binned"] / sweeps["gaussian"], 2),
                      "extra_us": round(sweeps["binned"] - sweeps["gaussian"], 1)}), flush=True)


if __name__ == "__main__":
    main()
