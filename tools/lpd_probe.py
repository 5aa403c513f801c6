"""The cost of the held-out log predictive density on MovieLens-1M's 500,000 test pairs (the bench's split) at D = 32, on the
factors of a Gaussian chain 20 iterations in: microseconds of bdf_pairs_lpd_update (phase 2, the running state read and written)
for the three kinds of record -- every pair a measurement (the Gaussian density), every pair a 0/1 value (the probit link: the
rating is at least 4), every pair a bin record (the rating r as [r - 1/2, r + 1/2), open at both ends) -- beside bdf_predict, which
is the gather alone, and bdf_interval_draw with the same bounds, on the same pairs in the caller's order and stored sorted by
movie, as the engine stores them; and one whole macau() iteration with the score (its update behind every iteration) and without.
Kernels are timed with device events around `reps` launches after `warmup`; iterations by the host clock around `iters` of them,
synchronised at both ends, after the engine's device warm-up.  Reads only the bundled data.  Prints one JSON line per figure.

    python tools/lpd_probe.py [--reps 50] [--warmup 10] [--iters 200] [--D 32]
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


def ratings(B):
    from bdf_amd import datasets
    d = datasets.load_movielens() if os.path.exists(datasets.MOVIELENS_PATH) else datasets.synthetic_movielens_like()
    X = d["X"]
    rel = B.Relation(X, "ratings", [B.Entity("users"), B.Entity("movies")])
    B.assignToTest(rel, datasets.split_test_ids(X.nnz, 500_000, 1))
    B.setPrecision(rel, 1.5)
    return B.RelationData(rel)


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
    B.setTestBinned(rel, EDGES)
    eng = B.GibbsEngine(rd, D, seed=0)
    eng.register_test((), rel.class_cut)
    for i in range(1, 21):
        eng.step(i, 0, (), rel.class_cut)
    eng.sync()
    eng.warm_device(50.0)
    test = eng.test_pairs()
    bounds = test.ctx.tensor(rel.model.test_interval)
    mean, alpha = rel.model.mean_value, rel.model.alpha
    sweeps, it = {}, 21
    for name, scored in (("plain", False), ("lpd", True), ("plain_again", False)):
        if scored:
            test.lpd_update(D, eng.factors_of(rel), mean, alpha, 1, bounds)
        eng.sync()
        t0 = time.perf_counter()
        for i in range(it, it + args.iters):
            eng.step(i, 0, (), rel.class_cut)
            if scored:
                test.lpd_update(D, eng.factors_of(rel), mean, alpha, 2, bounds)
        eng.sync()
        sweeps[name] = (time.perf_counter() - t0) * 1e6 / args.iters
        it += args.iters
        print(json.dumps({"what": "iteration_" + name, "D": D, "us_per_iteration": round(sweeps[name], 1), "test_pairs": test.n}), flush=True)
    print(json.dumps({"what": "lpd_over_plain_iteration", "D": D,
                      "extra_us": round(sweeps["lpd"] - 0.5 * (sweeps["plain"] + sweeps["plain_again"]), 1)}), flush=True)

    ctx, facs = eng.ctx, eng.factors_of(rel)
    fp = (C.c_void_p * 2)(*[f.data_ptr() for f in facs])
    ids, vals = np.asarray(rel.test_vec.ids), np.asarray(rel.test_vec.values)
    bd = ctx.tensor(rel.model.test_interval)
    out, stats = ctx.zeros(len(vals)), ctx.zeros(4)
    ctx.set_sweep(1000)

    def update(pairs, b):
        return lambda: check(lib().bdf_pairs_lpd_update(ctx.handle, pairs.handle, b, D, fp, mean, alpha, None, 2, C.c_void_p(stats.data_ptr())))

    for order in ("caller", "sorted_by_movie"):
        row = {"what": "lpd_vs_predict", "D": D, "pairs": len(vals), "order": order}
        for label, values, link, b in (("lpd_gauss_us", vals, 0, None), ("lpd_probit_us", (vals >= 4.0).astype(np.float64), 1, None),
                                       ("lpd_binned_us", vals, 0, C.c_void_p(bd.data_ptr()))):
            pairs = DevicePairs(ctx, ids, values)
            if order != "caller":
                pairs.sort(1)
            pairs.set_link(link)
            check(lib().bdf_pairs_lpd_update(ctx.handle, pairs.handle, b, D, fp, mean, alpha, None, 1, C.c_void_p(stats.data_ptr())))
            row[label] = round(timed(torch, ctx.stream, args.reps, args.warmup, update(pairs, b)), 2)
            if label == "lpd_binned_us":
                row["predict_us"] = round(timed(torch, ctx.stream, args.reps, args.warmup, lambda: check(lib().bdf_predict(
                    ctx.handle, pairs.handle, D, fp, mean, C.c_void_p(out.data_ptr())))), 2)
                row["interval_draw_us"] = round(timed(torch, ctx.stream, args.reps, args.warmup, lambda: check(lib().bdf_interval_draw(
                    ctx.handle, pairs.handle, C.c_void_p(bd.data_ptr()), D, fp, mean, alpha, None, 1, C.c_void_p(out.data_ptr()), None))), 2)
            pairs.close()
        row["lpd_binned_over_predict"] = round(row["lpd_binned_us"] / row["predict_us"], 2)
        row["lpd_binned_over_interval_draw"] = round(row["lpd_binned_us"] / row["interval_draw_us"], 2)
        print(json.dumps(row), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
