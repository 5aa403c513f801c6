"""The cost of the Polya-Gamma draw on MovieLens-shaped synthetic data (6,040 x 3,952, the bench's 500,000-rating test split, so
500,209 training pairs; datasets.synthetic_movielens_like), by default at D = 32: microseconds of bdf_pg_draw for the logit model
(b = 1 in every cell), for counts with mean about 3 (r = 3, b = y + 3: a wave costs its largest b) and, beside them, of
bdf_robust_draw on the same pairs, which does the same gather and draws one gamma variate per cell.  The pairs are stored sorted
by movie, as the engine stores them; the factors are N(0, 1 / sqrt(D)), so that psi = u.v is of order 1.  Kernels are timed with
device events around `reps` launches after `warmup`.  Prints one JSON line per figure.

    python tools/pg_probe.py [--reps 50] [--warmup 10] [--D 32] [--r 3]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    ap.add_argument("--D", type=int, default=32)
    ap.add_argument("--r", type=int, default=3)
    args = ap.parse_args()
    import torch
    import bdf_amd as B
    from bdf_amd import datasets
    from bdf_amd._lib import check, lib
    from bdf_amd.engine import DevicePairs
    D = args.D
    X = datasets.synthetic_movielens_like()["X"]
    rel = B.Relation(X, "ratings", [B.Entity("users"), B.Entity("movies")])
    B.assignToTest(rel, datasets.split_test_ids(X.nnz, 500_000, 1))
    ids = np.asarray(rel.data.ids)
    n = len(ids)
    rng = np.random.default_rng(0)
    ctx = B.Context(seed=0)
    facs = [ctx.tensor(rng.standard_normal((d, D)) / np.sqrt(np.sqrt(D))) for d in rel.data.dims]
    fp = (C.c_void_p * 2)(*[f.data_ptr() for f in facs])
    om, lin = ctx.zeros(n), ctx.zeros(n)
    ctx.set_sweep(1000)
    values = {"logit": (np.asarray(rel.data.values) > 3.5).astype(np.float64), "counts": rng.poisson(3.0, n).astype(np.float64)}
    for name, model, r in (("logit", 1, 0.0), ("counts", 2, float(args.r))):
        pairs = DevicePairs(ctx, ids, values[name])
        pairs.sort(1)
        us = timed(torch, ctx.stream, args.reps, args.warmup, lambda: check(lib().bdf_pg_draw(
            ctx.handle, pairs.handle, D, fp, 0.0, model, r, 1, C.c_void_p(om.data_ptr()), C.c_void_p(lin.data_ptr()))))
        w = om.cpu().numpy()
        print(json.dumps({"what": "pg_draw_" + name, "D": D, "pairs": n, "r": r, "mean_b": float(values[name].mean() + r) if model == 2 else 1.0,
                          "max_b": float(values[name].max() + r) if model == 2 else 1.0, "us": round(us, 2), "mean_omega": float(w.mean())}), flush=True)
        if name == "logit":
            us_r = timed(torch, ctx.stream, args.reps, args.warmup, lambda: check(lib().bdf_robust_draw(
                ctx.handle, pairs.handle, D, fp, 0.0, 1.5, None, 4.0, 1, C.c_void_p(om.data_ptr()), None)))
            print(json.dumps({"what": "robust_draw", "D": D, "pairs": n, "nu": 4.0, "us": round(us_r, 2)}), flush=True)
        pairs.close()
    ctx.close()


if __name__ == "__main__":
    main()
