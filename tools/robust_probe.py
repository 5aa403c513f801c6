"""The cost of the robust (Student-t) noise model and of observation weights on MovieLens-shaped synthetic data (6,040 x 3,952,
the bench's 500,000-rating test split, so 500,209 training pairs; datasets.synthetic_movielens_like), by default at D = 32:
microseconds of bdf_robust_draw with and without the sum for sample_alpha, of bdf_pairs_weighted_sse and of bdf_predict on the
same pairs (in the caller's order and stored sorted by movie, as the engine stores them); of one row launch per entity with
weights (k_rows_w), of the same relation unweighted on the general path (linear_values == mean_value: k_rows' general variant,
what BDF_K1_GENERAL_KERNEL=1 selects for every launch) and as the router sends it by default; and of one whole macau()
iteration with setRobust and without it on the same data.  Kernels are timed with device events around `reps` launches after
`warmup`; iterations by the host clock around `iters` of them, synchronised at both ends, after the engine's device warm-up.
Prints one JSON line per figure.

    python tools/robust_probe.py [--reps 50] [--warmup 10] [--iters 200] [--D 32] [--nu 4]
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


def ratings(B, nu):
    from bdf_amd import datasets
    X = datasets.synthetic_movielens_like()["X"]
    rel = B.Relation(X, "ratings", [B.Entity("users"), B.Entity("movies")])
    B.assignToTest(rel, datasets.split_test_ids(X.nnz, 500_000, 1))
    B.setPrecision(rel, 1.5)
    if nu:
        B.setRobust(rel, nu)
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
    ap.add_argument("--nu", type=float, default=4.0)
    args = ap.parse_args()
    import torch
    import bdf_amd as B
    from bdf_amd._lib import Term, check, lib
    from bdf_amd.engine import DevicePairs
    D = args.D
    sweeps = {}
    for name, nu in (("robust", args.nu), ("gaussian", 0.0)):
        rd = ratings(B, nu)
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
        if nu:
            ctx, facs = eng.ctx, eng.factors_of(rel)
            fp = (C.c_void_p * 2)(*[f.data_ptr() for f in facs])
            ids, vals = np.asarray(rel.data.ids), np.asarray(rel.data.values)
            n = len(vals)
            om, out, s = ctx.zeros(n), ctx.zeros(n), ctx.zeros(1)
            mean = rel.model.mean_value
            ctx.set_sweep(1000)
            for order in ("caller", "sorted_by_movie"):
                pairs = DevicePairs(ctx, ids, vals)
                if order != "caller":
                    pairs.sort(1)
                row = {"what": "draw_vs_predict", "D": D, "pairs": n, "order": order, "nu": nu}
                row["robust_draw_us"] = round(timed(torch, ctx.stream, args.reps, args.warmup, lambda: check(lib().bdf_robust_draw(
                    ctx.handle, pairs.handle, D, fp, mean, 1.5, None, nu, 1, C.c_void_p(om.data_ptr()), None))), 2)
                row["robust_draw_with_sum_us"] = round(timed(torch, ctx.stream, args.reps, args.warmup, lambda: check(lib().bdf_robust_draw(
                    ctx.handle, pairs.handle, D, fp, mean, 1.5, None, nu, 1, C.c_void_p(om.data_ptr()), C.c_void_p(s.data_ptr())))), 2)
                row["weighted_sse_us"] = round(timed(torch, ctx.stream, args.reps, args.warmup, lambda: check(lib().bdf_pairs_weighted_sse(
                    ctx.handle, pairs.handle, D, fp, mean, C.c_void_p(om.data_ptr()), C.c_void_p(s.data_ptr())))), 2)
                row["predict_us"] = round(timed(torch, ctx.stream, args.reps, args.warmup, lambda: check(lib().bdf_predict(
                    ctx.handle, pairs.handle, D, fp, mean, C.c_void_p(out.data_ptr())))), 2)
                row["draw_over_predict"] = round(row["robust_draw_us"] / row["predict_us"], 2)
                print(json.dumps(row), flush=True)
                pairs.close()
            # one row launch per entity: weighted | unweighted on the general path | unweighted as the router sends it
            lin = ctx.tensor(np.full(n, mean))
            for j, en in enumerate(rd.entities):
                st = eng.ent[j]
                nxt = ctx.zeros(st.N, D)
                row = {"what": "row_launch", "D": D, "entity": en.name, "rows": int(st.N), "observations": n}
                for label, w, l in (("weighted_us", om, None), ("general_path_us", None, lin), ("default_path_us", None, None)):
                    t = (Term * 1)()
                    t[0].rel, t[0].mode, t[0].alpha, t[0].mean_value = eng.rel[0].handle, j, 1.5, mean
                    t[0].linear_values = l.data_ptr() if l is not None else None
                    t[0].obs_precision = w.data_ptr() if w is not None else None
                    t[0].factors[1 - j] = eng.ent[1 - j].sample.data_ptr()
                    row[label] = round(timed(torch, ctx.stream, args.reps, args.warmup, lambda: check(lib().bdf_sample_rows(
                        ctx.handle, D, st.N, 1, t, C.c_void_p(st.mu.data_ptr()), 0, C.c_void_p(st.Lambda.data_ptr()), 900 + j, 0, 1,
                        C.c_void_p(nxt.data_ptr()), None))), 2)
                row["weighted_over_general"] = round(row["weighted_us"] / row["general_path_us"], 2)
                print(json.dumps(row), flush=True)
        eng.close()
    print(json.dumps({"what": "robust_over_gaussian_sweep", "D": D, "ratio": round(sweeps["robust"] / sweeps["gaussian"], 2),
                      "extra_us": round(sweeps["robust"] - sweeps["gaussian"], 1)}), flush=True)


if __name__ == "__main__":
    main()
