"""The cost of WAIC on MovieLens-1M's 500,209 training pairs (the bench's split) at D = 32, on the factors of a Gaussian chain 20
iterations in: microseconds of bdf_pairs_waic_update (phase 2, the running state of four doubles per pair read and written) for the
three kinds of record -- every pair a measurement (the Gaussian density), every pair a 0/1 value (the probit link: the rating is at
least 4), every pair a bin record (the rating r as [r - 1/2, r + 1/2), open at both ends) -- beside bdf_pairs_lpd_update with the
same records and bdf_predict, which is the gather alone, on the same pairs in the caller's order and stored sorted by movie; the
end-of-run bdf_pairs_waic with and without the pointwise table; and one whole macau() iteration with the score (its update behind
every iteration) and without.  Kernels are timed with device events around `reps` launches after `warmup`; iterations by the host
clock around `iters` of them, synchronised at both ends, after the engine's device warm-up.  Reads only the bundled data.  Prints one
JSON line per figure.

    python tools/waic_probe.py [--reps 50] [--warmup 10] [--iters 200] [--D 32]
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

from interval_probe import EDGES, timed  # noqa: E402
from lpd_probe import ratings  # noqa: E402


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
    rd = ratings(B)
    rel = rd.relations[0]
    eng = B.GibbsEngine(rd, D, seed=0)
    eng.register_test((), rel.class_cut)
    for i in range(1, 21):
        eng.step(i, 0, (), rel.class_cut)
    eng.sync()
    eng.warm_device(50.0)
    train = eng.train_pairs()
    mean, alpha = rel.model.mean_value, rel.model.alpha
    sweeps, it = {}, 21
    for name, scored in (("plain", False), ("waic", True), ("plain_again", False)):
        if scored:
            train.waic_update(D, eng.factors_of(rel), mean, alpha, 1)
        eng.sync()
        t0 = time.perf_counter()
        for i in range(it, it + args.iters):
            eng.step(i, 0, (), rel.class_cut)
            if scored:
                train.waic_update(D, eng.factors_of(rel), mean, alpha, 2)
        eng.sync()
        sweeps[name] = (time.perf_counter() - t0) * 1e6 / args.iters
        it += args.iters
        print(json.dumps({"what": "iteration_" + name, "D": D, "us_per_iteration": round(sweeps[name], 1), "train_pairs": train.n}), flush=True)
    print(json.dumps({"what": "waic_over_plain_iteration", "D": D,
                      "extra_us": round(sweeps["waic"] - 0.5 * (sweeps["plain"] + sweeps["plain_again"]), 1)}), flush=True)

    ctx, facs = eng.ctx, eng.factors_of(rel)
    fp = (C.c_void_p * 2)(*[f.data_ptr() for f in facs])
    ids, vals = np.asarray(rel.data.ids), np.asarray(rel.data.values, dtype=np.float64)
    full = np.concatenate([[-np.inf], EDGES, [np.inf]])
    j = np.searchsorted(EDGES, vals, side="right")
    bd = ctx.tensor(np.ascontiguousarray(np.stack([full[j], full[j + 1]], axis=1)))
    out, table, stats = ctx.zeros(len(vals)), ctx.zeros((len(vals), 2)), ctx.zeros(4)
    ctx.set_sweep(1000)

    def update(fn, pairs, b):
        return lambda: check(fn(ctx.handle, pairs.handle, b, D, fp, mean, alpha, None, 2, C.c_void_p(stats.data_ptr())))

    for order in ("caller", "sorted_by_movie"):
        row = {"what": "waic_vs_lpd_vs_predict", "D": D, "pairs": len(vals), "order": order}
        for kind, values, link, b in (("gauss", vals, 0, None), ("probit", (vals >= 4.0).astype(np.float64), 1, None),
                                      ("binned", vals, 0, C.c_void_p(bd.data_ptr()))):
            pairs = DevicePairs(ctx, ids, values)
            if order != "caller":
                pairs.sort(1)
            pairs.set_link(link)
            for name, fn in (("waic", lib().bdf_pairs_waic_update), ("lpd", lib().bdf_pairs_lpd_update)):
                check(fn(ctx.handle, pairs.handle, b, D, fp, mean, alpha, None, 1, C.c_void_p(stats.data_ptr())))
                row[f"{name}_{kind}_us"] = round(timed(torch, ctx.stream, args.reps, args.warmup, update(fn, pairs, b)), 2)
            if kind == "binned":
                row["predict_us"] = round(timed(torch, ctx.stream, args.reps, args.warmup, lambda: check(lib().bdf_predict(
                    ctx.handle, pairs.handle, D, fp, mean, C.c_void_p(out.data_ptr())))), 2)
                row["waic_read_us"] = round(timed(torch, ctx.stream, args.reps, args.warmup, lambda: check(lib().bdf_pairs_waic(
                    ctx.handle, pairs.handle, None, C.c_void_p(stats.data_ptr())))), 2)
                row["waic_read_pointwise_us"] = round(timed(torch, ctx.stream, args.reps, args.warmup, lambda: check(lib().bdf_pairs_waic(
                    ctx.handle, pairs.handle, C.c_void_p(table.data_ptr()), C.c_void_p(stats.data_ptr())))), 2)
            pairs.close()
        row["waic_binned_over_lpd_binned"] = round(row["waic_binned_us"] / row["lpd_binned_us"], 2)
        row["waic_binned_over_predict"] = round(row["waic_binned_us"] / row["predict_us"], 2)
        print(json.dumps(row), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
