"""The cost of the probit noise model on MovieLens-1M binarised at rating >= 4 (the bench's 500,000-rating test split, so
500,209 training pairs) at D = 32: microseconds of bdf_probit_draw alone and of bdf_predict on the same pairs (both with the
pairs in the caller's order and stored sorted by movie, as the engine stores them), and of one whole macau() iteration with the
probit model and with the Gaussian model on the same 0/1 data.  Kernels are timed with device events around `reps` launches
after `warmup`; iterations by the host clock around `iters` of them, synchronised at both ends, after the engine's device
warm-up.  Reads only the bundled data.  Prints one JSON line per figure.

    python tools/probit_probe.py [--reps 50] [--warmup 10] [--iters 200] [--D 32]
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


def binarised(B, probit):
    from bdf_amd import datasets
    d = datasets.load_movielens() if os.path.exists(datasets.MOVIELENS_PATH) else datasets.synthetic_movielens_like()
    X = d["X"].copy()
    X.data = (X.data >= 4.0).astype(np.float64)          # (explicit zeros stay stored: every rating is an observation)
    rel = B.Relation(X, "liked", [B.Entity("users"), B.Entity("movies")], class_cut=0.5)
    B.assignToTest(rel, datasets.split_test_ids(X.nnz, 500_000, 1))
    if probit:
        B.setProbit(rel)
    else:
        B.setPrecision(rel, 1.5)
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
    for name, probit in (("probit", True), ("gaussian", False)):
        rd = binarised(B, probit)
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
        if probit:
            ctx, facs = eng.ctx, eng.factors_of(rel)
            fp = (C.c_void_p * 2)(*[f.data_ptr() for f in facs])
            ids, vals = np.asarray(rel.data.ids), np.asarray(rel.data.values)
            lin, out = ctx.zeros(len(vals)), ctx.zeros(len(vals))
            ctx.set_sweep(1000)
            for order in ("caller", "sorted_by_movie"):
                pairs = DevicePairs(ctx, ids, vals)
                if order != "caller":
                    pairs.sort(1)
                draw = timed(torch, ctx.stream, args.reps, args.warmup, lambda: check(lib().bdf_probit_draw(
                    ctx.handle, pairs.handle, D, fp, 0.0, 1, C.c_void_p(lin.data_ptr()), None)))
                pred = timed(torch, ctx.stream, args.reps, args.warmup, lambda: check(lib().bdf_predict(
                    ctx.handle, pairs.handle, D, fp, 0.0, C.c_void_p(out.data_ptr()))))
                pairs.set_link(1)
                link = timed(torch, ctx.stream, args.reps, args.warmup, lambda: check(lib().bdf_predict(
                    ctx.handle, pairs.handle, D, fp, 0.0, C.c_void_p(out.data_ptr()))))
                print(json.dumps({"what": "draw_vs_predict", "D": D, "pairs": len(vals), "order": order, "probit_draw_us": round(draw, 2),
                                  "predict_us": round(pred, 2), "predict_link_us": round(link, 2), "draw_over_predict": round(draw / pred, 2)}),
                      flush=True)
                pairs.close()
        eng.close()
    print(json.dumps({"what": "probit_over_gaussian_sweep", "D": D, "ratio": round(sweeps["probit"] / sweeps["gaussian"], 2),
                      "extra_us": round(sweeps["probit"] - sweeps["gaussian"], 1)}), flush=True)


if __name__ == "__main__":
    main()
