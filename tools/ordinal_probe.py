"""The cost of the ordinal noise model's cutpoint step on MovieLens-1M (the bench's 500,000-rating test split, so 500,209 training
pairs; K = 5) at D = 32: microseconds of one whole macau() iteration with setOrdinal, with setOrdinal(sample_edges=False) and with
setBinned([1.5, 2.5, 3.5, 4.5]) on the same data (the last two enqueue the same launches; tools/interval_probe.py prints the same
"sweep_binned" figure on a build without this model), and of bdf_ordinal_step, bdf_interval_draw, bdf_ordinal_bounds and bdf_predict
alone on the training pairs as the engine stores them (sorted by movie).  The step is timed as it runs in a chain -- the edges move
when a proposal is accepted, the bounds are rewritten then -- and once more with a step size of 1e-8, where next to every proposal
is accepted and the bounds are rewritten every time.  Kernels are timed with device events around `reps` launches after `warmup`;
iterations by the host clock around `iters` of them, synchronised at both ends, after the engine's device warm-up.  Reads only the
bundled data.  Prints one JSON line per figure.

    python tools/ordinal_probe.py [--reps 50] [--warmup 10] [--iters 200] [--D 32]
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


def ratings(B, model):
    from bdf_amd import datasets
    d = datasets.load_movielens() if os.path.exists(datasets.MOVIELENS_PATH) else datasets.synthetic_movielens_like()
    X = d["X"]
    rel = B.Relation(X, "ratings", [B.Entity("users"), B.Entity("movies")])
    B.assignToTest(rel, datasets.split_test_ids(X.nnz, 500_000, 1))
    B.setPrecision(rel, 1.5)
    if model == "binned":
        B.setBinned(rel, EDGES)
    else:
        B.setOrdinal(rel, sample_edges=model == "ordinal")
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
    D = args.D
    sweeps = {}
    for model in ("ordinal", "fixed", "binned"):
        rd = ratings(B, model)
        rel = rd.relations[0]
        eng = B.GibbsEngine(rd, D, seed=0)
        eng.ordinal_begin(20, args.iters)
        eng.register_test((), rel.class_cut)
        for i in range(1, 21):
            eng.step(i, 0, (), rel.class_cut)
        eng.sync()
        eng.warm_device(50.0)
        t0 = time.perf_counter()
        for i in range(21, 21 + args.iters):
            eng.step(i, 0, (), rel.class_cut)
        eng.sync()
        sweeps[model] = (time.perf_counter() - t0) * 1e6 / args.iters
        row = {"what": "sweep_" + model, "D": D, "us_per_iteration": round(sweeps[model], 1), "train_pairs": rel.data.nnz()}
        if model == "ordinal":
            got = eng.rel[0].ordinal.read()
            row.update(edges=[round(float(e), 4) for e in got["edges"]], proposals=got["proposals"], accepts=got["accepts"], step=round(got["sigma"], 5))
        print(json.dumps(row), flush=True)
        if model == "ordinal":
            ctx, dr, facs = eng.ctx, eng.rel[0], eng.factors_of(rel)
            fp = (C.c_void_p * 2)(*[f.data_ptr() for f in facs])
            n, mean = rel.data.nnz(), rel.model.mean_value
            lin, out, bd = ctx.zeros(n), ctx.zeros(n), dr.interval.clone()
            ctx.set_sweep(1000)
            row = {"what": "step_vs_draw", "D": D, "pairs": n, "order": "sorted_by_movie"}
            for label, step in (("ordinal_step_us", got["sigma"]), ("ordinal_step_all_accepted_us", 1e-8)):
                o = B.DeviceOrdinal(ctx, 5, step, 0)
                row[label] = round(timed(torch, ctx.stream, args.reps, args.warmup, lambda: o.step(ctx, dr.train, dr.ord_codes, D, facs, mean, 1.5, 1, 0, bd)), 2)
                row[label.replace("_us", "_accepted")] = round(o.read()["accepts"] / (args.reps + args.warmup), 2)
                o.close()
            o = B.DeviceOrdinal(ctx, 5, 0.1, 0)
            row["ordinal_bounds_us"] = round(timed(torch, ctx.stream, args.reps, args.warmup, lambda: o.bounds(ctx, dr.ord_codes, bd)), 2)
            o.close()
            row["interval_draw_us"] = round(timed(torch, ctx.stream, args.reps, args.warmup, lambda: check(lib().bdf_interval_draw(
                ctx.handle, dr.train.handle, C.c_void_p(bd.data_ptr()), D, fp, mean, 1.5, None, 1, C.c_void_p(lin.data_ptr()), None))), 2)
            row["predict_us"] = round(timed(torch, ctx.stream, args.reps, args.warmup, lambda: check(lib().bdf_predict(
                ctx.handle, dr.train.handle, D, fp, mean, C.c_void_p(out.data_ptr())))), 2)
            row["step_over_interval_draw"] = round(row["ordinal_step_us"] / row["interval_draw_us"], 2)
            print(json.dumps(row), flush=True)
        eng.close()
    print(json.dumps({"what": "ordinal_over_fixed_sweep", "D": D, "ratio": round(sweeps["ordinal"] / sweeps["fixed"], 2),
                      "extra_us": round(sweeps["ordinal"] - sweeps["fixed"], 1), "fixed_minus_binned_us": round(sweeps["fixed"] - sweeps["binned"], 1)}), flush=True)


if __name__ == "__main__":
    main()
