"""The cost of the per-row noise model (setEntityNoise) on MovieLens-1M-shaped synthetic data (6,040 x 3,952,
the bench's 500,000-rating test split, so 500,209 training pairs; datasets.synthetic_movielens_like), by default at D = 32:
microseconds of bdf_entity_noise_draw -- its two launches, and with the third that sums tau_j S_j for sample_alpha -- with the
movies (mean degree 127: the 64-wide row pass) and with the users (mean degree 83: 64-wide too) as the noise entity, beside
bdf_predict and a prediction update (bdf_predict_update, phase 0) over the same pairs stored the same way; and of one whole macau()
iteration with setEntityNoise against the same relation under setWeights of all ones, which samples its rows with the same kernel
(k_rows_w) and so isolates the draw.  Kernels are timed with device events around `reps` calls after `warmup`; iterations by the
host clock around `iters` of them, synchronised at both ends, after the engine's device warm-up.  Prints one JSON line per figure.

    python tools/entity_noise_probe.py [--reps 50] [--warmup 10] [--iters 200] [--D 32]
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


def ratings(B, model):
    from bdf_amd import datasets
    X = datasets.synthetic_movielens_like()["X"]
    rel = B.Relation(X, "ratings", [B.Entity("users"), B.Entity("movies")])
    B.assignToTest(rel, datasets.split_test_ids(X.nnz, 500_000, 1))
    B.setPrecision(rel, 1.5)
    if model == "entity_noise":
        B.setEntityNoise(rel, "movies")
    elif model == "unit_weights":
        B.setWeights(rel, np.ones(rel.data.nnz()))
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
    for model in ("entity_noise", "unit_weights", "gaussian"):
        rd = ratings(B, model)
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
        sweeps[model] = (time.perf_counter() - t0) * 1e6 / args.iters
        print(json.dumps({"what": "sweep_" + model, "D": D, "us_per_iteration": round(sweeps[model], 1), "train_pairs": rel.data.nnz(),
                          "rows_dispatch": [eng.rows_dispatch(j) for j in range(2)]}), flush=True)
        if model == "entity_noise":
            ctx, facs = eng.ctx, eng.factors_of(rel)
            fp = (C.c_void_p * 2)(*[f.data_ptr() for f in facs])
            ids, vals = np.asarray(rel.data.ids), np.asarray(rel.data.values)
            n, mean = len(vals), rel.model.mean_value
            om, out, s, stats = ctx.zeros(n), ctx.zeros(n), ctx.zeros(1), ctx.zeros(4)
            ctx.set_sweep(1000)
            pairs = DevicePairs(ctx, ids, vals)
            pairs.sort(1)                                          # as the engine stores the training pairs: sorted by movie
            p = lambda t: C.c_void_p(t.data_ptr())
            for mode, name in ((1, "movies"), (0, "users")):
                N = int(rel.data.dims[mode])
                tau = ctx.zeros(N)
                row = {"what": "draw_vs_predict", "D": D, "pairs": n, "noise_entity": name, "rows": N, "mean_degree": round(n / N, 1),
                       "group_width": 8 if n <= 32 * N else 64}
                row["draw_us"] = round(timed(torch, ctx.stream, args.reps, args.warmup, lambda: check(lib().bdf_entity_noise_draw(
                    ctx.handle, eng.rel[0].handle, mode, pairs.handle, D, fp, mean, 1.5, None, 2.0, 2.0, 1, p(tau), p(om), None))), 2)
                row["draw_with_sum_us"] = round(timed(torch, ctx.stream, args.reps, args.warmup, lambda: check(lib().bdf_entity_noise_draw(
                    ctx.handle, eng.rel[0].handle, mode, pairs.handle, D, fp, mean, 1.5, None, 2.0, 2.0, 1, p(tau), p(om), p(s)))), 2)
                row["predict_us"] = round(timed(torch, ctx.stream, args.reps, args.warmup, lambda: check(lib().bdf_predict(
                    ctx.handle, pairs.handle, D, fp, mean, p(out)))), 2)
                row["predict_update_us"] = round(timed(torch, ctx.stream, args.reps, args.warmup, lambda: check(lib().bdf_predict_update(
                    ctx.handle, pairs.handle, D, fp, mean, 0, 1.0, -1.0, rel.class_cut, p(stats)))), 2)
                row["draw_over_predict_update"] = round(row["draw_us"] / row["predict_update_us"], 2)
                print(json.dumps(row), flush=True)
            pairs.close()
        eng.close()
    print(json.dumps({"what": "entity_noise_over_unit_weights_sweep", "D": D, "ratio": round(sweeps["entity_noise"] / sweeps["unit_weights"], 2),
                      "extra_us": round(sweeps["entity_noise"] - sweeps["unit_weights"], 1),
                      "over_gaussian": round(sweeps["entity_noise"] / sweeps["gaussian"], 2)}), flush=True)


if __name__ == "__main__":
    main()
