"""The cost of the censored (Tobit) noise model on MovieLens-1M (the bench's 500,000-rating test split, so 500,209 training
pairs) at D = 32, with rating 5 right-censored ("at least 5") and rating 1 left-censored ("at most 1"): microseconds of
bdf_censored_draw, of bdf_probit_draw and of bdf_predict on the same pairs (in the caller's order and stored sorted by movie, as
the engine stores them; the probit draw only for its time: on ratings every label is 1), and of one whole macau() iteration with
the flags and without them on the same data.  Kernels are timed with device events around `reps` launches after `warmup`;
iterations by the host clock around `iters` of them, synchronised at both ends, after the engine's device warm-up.  Reads only
the bundled data.  Prints one JSON line per figure.

    python tools/censored_probe.py [--reps 50] [--warmup 10] [--iters 200] [--D 32]
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


def ratings(B, censored):
    from bdf_amd import datasets
    d = datasets.load_movielens() if os.path.exists(datasets.MOVIELENS_PATH) else datasets.synthetic_movielens_like()
    X = d["X"]
    rel = B.Relation(X, "ratings", [B.Entity("users"), B.Entity("movies")])
    B.assignToTest(rel, datasets.split_test_ids(X.nnz, 500_000, 1))
    B.setPrecision(rel, 1.5)
    v = np.asarray(rel.data.values)
    flags = np.where(v >= 5.0, 1, np.where(v <= 1.0, -1, 0)).astype(np.int8)
    if censored:
        B.setCensored(rel, flags)
    return B.RelationData(rel), flags


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
    for name, censored in (("censored", True), ("gaussian", False)):
        rd, flags = ratings(B, censored)
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
                          "censored_share": round(float(np.mean(flags != 0)), 3), "rows_dispatch": disp}), flush=True)
        if censored:
            ctx, facs = eng.ctx, eng.factors_of(rel)
            fp = (C.c_void_p * 2)(*[f.data_ptr() for f in facs])
            ids, vals = np.asarray(rel.data.ids), np.asarray(rel.data.values)
            lin, out = ctx.zeros(len(vals)), ctx.zeros(len(vals))
            mean = rel.model.mean_value
            ctx.set_sweep(1000)
            for order in ("caller", "sorted_by_movie"):
                pairs = DevicePairs(ctx, ids, vals)
                if order != "caller":
                    pairs.sort(1)
                row = {"what": "draw_vs_predict", "D": D, "pairs": len(vals), "order": order}
                for label, c in (("censored_draw_us", flags), ("censored_draw_all_flagged_us", np.ones_like(flags)),
                                 ("censored_draw_none_flagged_us", np.zeros_like(flags))):
                    cd = ctx.tensor(c, dtype=torch.int8)
                    row[label] = round(timed(torch, ctx.stream, args.reps, args.warmup, lambda: check(lib().bdf_censored_draw(
                        ctx.handle, pairs.handle, C.c_void_p(cd.data_ptr()), D, fp, mean, 1.5, None, 1, C.c_void_p(lin.data_ptr()), None))), 2)
                row["probit_draw_us"] = round(timed(torch, ctx.stream, args.reps, args.warmup, lambda: check(lib().bdf_probit_draw(
                    ctx.handle, pairs.handle, D, fp, 0.0, 1, C.c_void_p(lin.data_ptr()), None))), 2)
                row["predict_us"] = round(timed(torch, ctx.stream, args.reps, args.warmup, lambda: check(lib().bdf_predict(
                    ctx.handle, pairs.handle, D, fp, mean, C.c_void_p(out.data_ptr())))), 2)
                row["censored_over_probit_draw"] = round(row["censored_draw_all_flagged_us"] / row["probit_draw_us"], 2)
                print(json.dumps(row), flush=True)
                pairs.close()
        eng.close()
    print(json.dumps({"what": "censored_over_gaussian_sweep", "D": D, "ratio": round(sweeps["censored"] / sweeps["gaussian"], 2),
                      "extra_us": round(sweeps["censored"] - sweeps["gaussian"], 1)}), flush=True)


if __name__ == "__main__":
    main()
