"""The cost of predicting cells of new rows (setNewRows / setNewTest) at a stated shape: configuration C3's
MovieLens-1M relation with its dense 6040 x 500 user features (iid N(0, 1), seed 4242), 1,000 users (seeded choice) and ALL their
ratings held out as new rows, D = 32, on the factors of a Macau chain 10 iterations in.  Microseconds of the three launches that
follow every iteration -- bdf_uhat on the new rows' operator, bdf_newrows_quad over the movies, bdf_newrows_update (phase 2) over the
held-out ratings -- each alone and the three together, timed with device events around `reps` launches after `warmup`, `rounds` times
over: the range is printed, not one figure.  Beside them, by the host clock around `iters` iterations synchronised at both ends:
one iteration of the full C3 configuration (6040 users, direct solve; the sweep's code is the parent commit's) and one iteration of
this run with and without the three launches.  From the times: the update's achieved gather rate (two factor rows of D doubles per
cell) and the quad kernel's share of the fp64 matrix peak (78.6 TFLOP/s) over the matrix instructions it issues.  Reads only the
bundled data.  Prints one JSON line per figure.

    python tools/newrows_probe.py [--reps 50] [--warmup 10] [--rounds 7] [--iters 100] [--D 32] [--new 1000]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from interval_probe import timed  # noqa: E402


def spread(xs):
    xs = sorted(xs)
    return {"min": round(xs[0], 2), "median": round(xs[len(xs) // 2], 2), "max": round(xs[-1], 2)}


def held_out_users(B, datasets, n_new, seed=99):
    """C3's relation without n_new users: (RelationData of the others with their features, F of the held-out users, their ratings as
    the table of new cells)"""
    d = datasets.load_movielens(datasets.MOVIELENS_PATH) if os.path.exists(datasets.MOVIELENS_PATH) else datasets.synthetic_movielens_like()
    X = d["X"].tocsr()
    N = X.shape[0]
    F = datasets.c3_user_features("iid", n_users=N)
    new = np.sort(np.random.default_rng(seed).choice(N, size=n_new, replace=False))
    keep = np.setdiff1d(np.arange(N), new)
    users, movies = B.Entity("users", F=F[keep]), B.Entity("movies")
    rel = B.Relation(X[keep].tocsc(), "ratings", [users, movies], class_cut=2.5)
    B.setPrecision(rel, 1.5)
    Xn = X[new].tocoo()
    B.setNewRows(users, F[new])
    B.setNewTest(rel, users, {"users": Xn.row + 1, "movies": Xn.col + 1, "rating": Xn.data.astype(np.float64)})
    return B.RelationData(rel), int(Xn.nnz), int(X.shape[1])


def iteration_us(eng, first, iters, after=None):
    eng.sync()
    t0 = time.perf_counter()
    for i in range(first, first + iters):
        eng.sweep(i)
        if after is not None:
            after()
    eng.sync()
    return (time.perf_counter() - t0) / iters * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--D", type=int, default=32)
    ap.add_argument("--new", type=int, default=1000)
    args = ap.parse_args()
    import torch
    import bdf_amd as B
    from bdf_amd import datasets
    from bdf_amd._lib import check, lib
    from bdf_amd.engine import _ptr
    D = args.D
    # the full C3 configuration's iteration on this machine (the sweep is the parent commit's code: this feature adds nothing to it)
    rd, _ = datasets.c3_relation_data(B, "iid")
    eng = B.GibbsEngine(rd, D, seed=1)
    eng.warm_device(30.0)
    for i in range(1, 11):
        eng.sweep(i)
    c3 = [iteration_us(eng, 11 + k * args.iters, args.iters) for k in range(args.rounds)]
    eng.close()
    print(json.dumps({"figure": "c3_iteration_us", "D": D, **spread(c3)}))

    rd, n_cells, M = held_out_users(B, datasets, args.new)
    rel = rd.relations[0]
    eng = B.GibbsEngine(rd, D, seed=1)
    eng.warm_device(30.0)
    for i in range(1, 11):
        eng.sweep(i)
    eng.sync()
    nr = eng.new_rows()
    ctx, st, so = eng.ctx, nr.st, nr.so
    mean, alpha = rel.model.mean_value, rel.model.alpha
    nr.step(1, (), rel.class_cut, alpha, True)                      # the state exists: the launches below are phase 2
    eng.sync()
    stats = ctx.zeros(8)
    launches = {
        "uhat": lambda: check(lib().bdf_uhat(ctx.handle, nr.F.handle, D, _ptr(st.beta), _ptr(st.mu), _ptr(nr.uhat), _ptr(nr.factors))),
        "quad": lambda: check(lib().bdf_newrows_quad(ctx.handle, D, so.N, _ptr(st.Lambda), _ptr(so.sample), _ptr(nr.q))),
        "update": lambda: check(lib().bdf_newrows_update(ctx.handle, nr.pairs.handle, D, _ptr(nr.factors), _ptr(so.sample), _ptr(nr.q), mean, alpha, None, 2,
                                                         1.0, -1.0, rel.class_cut, 1, _ptr(stats))),
    }
    # (the quad call on 16 rows of V: its one-wave factorisation and inversion of Lambda with next to no product behind it)
    launches["quad_16_rows"] = lambda: check(lib().bdf_newrows_quad(ctx.handle, D, 16, _ptr(st.Lambda), _ptr(so.sample), _ptr(nr.q)))
    launches["all_three"] = lambda: [f() for f in (launches["uhat"], launches["quad"], launches["update"])]
    us = {}
    with torch.cuda.stream(ctx.stream):
        for name, fn in launches.items():
            us[name] = [timed(torch, ctx.stream, args.reps, args.warmup, fn) for _ in range(args.rounds)]
            print(json.dumps({"figure": name + "_us", "new_rows": args.new, "cells": n_cells, "columns": M, "D": D, **spread(us[name])}))
    # the update's gather: two factor rows of D doubles per cell; the quad kernel's matrix instructions: 16 x 16 x 4 x 2 flops each,
    # column block cb of a 16-row tile takes the k-steps 0 .. 4 cb + 3 that lie below D
    DP = 16 if D <= 16 else (32 if D <= 32 else 64)
    per_tile = sum(sum(1 for cb in range(s // 4, DP // 16)) for s in range(DP // 4) if 4 * s < D)
    flops = -(-M // 16) * per_tile * 2048.0
    for name, t in (("min", min(us["update"])), ("median", sorted(us["update"])[len(us["update"]) // 2]), ("max", max(us["update"]))):
        print(json.dumps({"figure": "update_gather_GBps_at_" + name + "_time", "value": round(n_cells * 2 * D * 8 / t / 1e3, 1)}))
    print(json.dumps({"figure": "quad_share_of_fp64_matrix_peak", "mfma_flops": flops,
                      "at_min_time": round(flops / (min(us["quad"]) * 1e-6) / 78.6e12, 5), "at_max_time": round(flops / (max(us["quad"]) * 1e-6) / 78.6e12, 5)}))
    first = 11
    for name, after in (("iteration_without_us", None), ("iteration_with_us", lambda: nr.step(2, (), rel.class_cut, alpha, True)), ("iteration_without_again_us", None)):
        ts = []
        for _ in range(args.rounds):
            ts.append(iteration_us(eng, first, args.iters, after))
            first += args.iters
        print(json.dumps({"figure": name, "users": rd.entities[0].count, **spread(ts)}))
    eng.close()


if __name__ == "__main__":
    main()
