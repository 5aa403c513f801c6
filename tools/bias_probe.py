"""The cost of row and column biases (setBias) on MovieLens-1M-shaped synthetic data (6,040 x 3,952, the
bench's 500,000-rating test split, so 500,209 training pairs; datasets.synthetic_movielens_like), by default at D = 32, in ONE
process, the variants interleaved, `runs` runs each, reported as min - max.

Calls, timed with device events around one call each after `warmup` calls: bdf_entity_noise_draw without its sum (k_noise_resid and
one row pass: the neighbour the residual launch is held against), bdf_bias_draw with the users, with the movies and with both
entities biased (the residual launch, per biased mode a row and a lambda launch, the base launch), bdf_bias_baseline over the
500,000 test pairs, and bdf_predict over the training pairs.  A single launch cannot be timed through the C ABI: run

    BDF_RESERVE_CUS=0 rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/bias_probe.py --kernels

(BDF_RESERVE_CUS=0: the profiler crashes in its own teardown after a process that used CU-masked streams) for the
per-kernel figures (k_bias_resid beside k_noise_resid on the same pairs, k_bias_rows of both modes, k_bias_lambda,
k_bias_base over the training and over the test pairs): that mode makes `runs` interleaved rounds of the calls and nothing else.

Iterations, by the host clock around `iters` of them, synchronised at both ends, after the engine's device warm-up: the plain
Gaussian model (the lean row kernels) against both entities biased (the general row kernel, which reads a base per cell, plus the
bias step), the two engines alive together and taking turns; and the row launches of both by device events (the engine's own
timers), which separates the move between the row kernels from the bias step.  Prints one JSON line per figure.

    python tools/bias_probe.py [--runs 30] [--warmup 5] [--iters 20] [--D 32] [--kernels]
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


def ratings(B, biased):
    from bdf_amd import datasets
    X = datasets.synthetic_movielens_like()["X"]
    rel = B.Relation(X, "ratings", [B.Entity("users"), B.Entity("movies")])
    B.assignToTest(rel, datasets.split_test_ids(X.nnz, 500_000, 1))
    B.setPrecision(rel, 1.5)
    if biased:
        B.setBias(rel, "users")
        B.setBias(rel, "movies")
    return B.RelationData(rel)


def once(torch, stream, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def span(xs):
    return {"min_us": round(min(xs), 2), "max_us": round(max(xs), 2), "runs": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--D", type=int, default=32)
    ap.add_argument("--kernels", action="store_true", help="only the interleaved calls, for a run under rocprofv3 --kernel-trace --stats")
    args = ap.parse_args()
    import torch
    import bdf_amd as B
    from bdf_amd._lib import BiasTerm, check, lib
    from bdf_amd.engine import DevicePairs
    D = args.D
    engines = {}
    for name in ("plain", "biased"):
        rd = ratings(B, name == "biased")
        eng = B.GibbsEngine(rd, D, seed=0)
        eng.register_test((), rd.relations[0].class_cut)
        for i in range(1, 21):
            eng.step(i, 0, (), rd.relations[0].class_cut)
        eng.sync()
        engines[name] = (rd, eng)
    # ---- the calls, on the plain engine's context and factors ---------------------------------------------------------------
    rd, eng = engines["plain"]
    rel = rd.relations[0]
    ctx, facs = eng.ctx, eng.factors_of(rel)
    fp = (C.c_void_p * 2)(*[f.data_ptr() for f in facs])
    ids, vals = np.asarray(rel.data.ids), np.asarray(rel.data.values)
    n, mean = len(vals), rel.model.mean_value
    p = lambda t: C.c_void_p(t.data_ptr())
    ctx.set_sweep(1000)
    pairs = DevicePairs(ctx, ids, vals)
    pairs.sort(1)                                          # as the engine stores the training pairs: sorted by movie
    tids = rel.test_vec.ids.reshape(len(rel.test_vec), 2)
    test = DevicePairs(ctx, tids, np.asarray(rel.test_vec.values))
    test.sort(1)
    om, out, resid, lin, tb = ctx.zeros(n), ctx.zeros(n), ctx.zeros(n), ctx.zeros(n), ctx.zeros(test.n)
    N = [int(x) for x in rel.data.dims]
    bias, lam, tau = [ctx.zeros(N[0]), ctx.zeros(N[1])], ctx.tensor([1.0, 1.0]), [ctx.zeros(N[0]), ctx.zeros(N[1])]

    def terms(modes):
        t = (BiasTerm * len(modes))()
        for k, m in enumerate(modes):
            t[k].mode, t[k].shape, t[k].rate, t[k].bias, t[k].lambda_ = m, 1.0, 1.0, bias[m].data_ptr(), lam.data_ptr() + 8 * m
        return t

    t_u, t_m, t_both = terms([0]), terms([1]), terms([0, 1])
    h = eng.rel[0].handle
    calls = {
        "entity_noise_draw_users": lambda: check(lib().bdf_entity_noise_draw(ctx.handle, h, 0, pairs.handle, D, fp, mean, 1.5, None, 2.0, 2.0, 1, p(tau[0]), p(om), None)),
        "bias_draw_users": lambda: check(lib().bdf_bias_draw(ctx.handle, h, pairs.handle, D, fp, mean, 1.5, None, 1, 1, t_u, p(resid), p(lin))),
        "bias_draw_movies": lambda: check(lib().bdf_bias_draw(ctx.handle, h, pairs.handle, D, fp, mean, 1.5, None, 1, 1, t_m, p(resid), p(lin))),
        "bias_draw_both": lambda: check(lib().bdf_bias_draw(ctx.handle, h, pairs.handle, D, fp, mean, 1.5, None, 1, 2, t_both, p(resid), p(lin))),
        "bias_baseline_test": lambda: check(lib().bdf_bias_baseline(ctx.handle, test.handle, 2, t_both, mean, p(tb))),
        "predict_train": lambda: check(lib().bdf_predict(ctx.handle, pairs.handle, D, fp, mean, p(out))),
    }
    for _ in range(args.warmup):
        for fn in calls.values():
            fn()
    ctx.sync()
    got = {k: [] for k in calls}
    for _ in range(args.runs):                             # interleaved: one call of each per round
        for k, fn in calls.items():
            got[k].append(once(torch, ctx.stream, fn))
    if args.kernels:
        pairs.close()
        test.close()
        for rd, eng in engines.values():
            eng.close()
        return
    shape = {"D": D, "train_pairs": n, "test_pairs": test.n, "rows": N, "group_width": [8 if n <= 32 * x else 64 for x in N]}
    for k, xs in got.items():
        print(json.dumps({"what": "call_" + k, **span(xs), **shape}), flush=True)
    pairs.close()
    test.close()
    # ---- iterations: the two engines take turns -----------------------------------------------------------------------------
    for name, (rd, eng) in engines.items():
        eng.warm_device(50.0)
    it = {name: 21 for name in engines}
    sweeps = {name: [] for name in engines}
    for _ in range(args.runs):
        for name, (rd, eng) in engines.items():
            cut = rd.relations[0].class_cut
            eng.sync()
            t0 = time.perf_counter()
            for i in range(it[name], it[name] + args.iters):
                eng.step(i, 0, (), cut)
            eng.sync()
            sweeps[name].append((time.perf_counter() - t0) * 1e6 / args.iters)
            it[name] += args.iters
    for name, (rd, eng) in engines.items():
        print(json.dumps({"what": "iteration_" + name, **span(sweeps[name]), "iters_per_run": args.iters, "D": D,
                          "rows_dispatch": [eng.rows_dispatch(j) for j in range(2)]}), flush=True)
    # ---- the row launches of both, by device events ---------------------------------------------------------------------------
    rows = {}
    for _ in range(3):
        for name, (rd, eng) in engines.items():
            cut = rd.relations[0].class_cut
            eng.k1_events, eng.k1_event_every = [], 1
            for i in range(it[name], it[name] + 10):
                eng.step(i, 0, (), cut)
            eng.sync()
            it[name] += 10
            for j, timer in eng.k1_events:
                rows.setdefault((name, j), []).append(timer.elapsed_us())
            eng.k1_events = None
    for (name, j), xs in sorted(rows.items()):
        print(json.dumps({"what": "row_launch_%s_%s" % (name, ["users", "movies"][j]), **span(xs), "D": D}), flush=True)
    d = [b - a for a, b in zip(sweeps["plain"], sweeps["biased"])]
    print(json.dumps({"what": "biased_minus_plain_iteration", **span(d), "D": D}), flush=True)
    for rd, eng in engines.values():
        eng.close()


if __name__ == "__main__":
    main()
