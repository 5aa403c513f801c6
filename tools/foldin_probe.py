"""The cost of folding new rows in from a few cells of their own (setNewObserved) at a stated shape: configuration
C3's MovieLens-1M relation with its dense 6040 x 500 user features (iid N(0, 1), seed 4242), 1,000 users (seeded choice) held out as
new rows, 10 of each user's ratings (seeded shuffle) known and the rest scored, D = 32, on the factors of a Macau chain 10 iterations
in.  Microseconds of the launches that follow every iteration, timed with device events around `reps` launches after `warmup`,
`rounds` times over (the range is printed, not one figure):
  systems        the row sampler's dump launch on the relation of the known cells, with the small launches that make its prior pack
                 (bdf_row_system: the launch that bdf_foldin_cells makes per chunk; one chunk here)
  cells          k_foldin_cells alone on those systems (bdf_foldin_solve)
  foldin_cells   bdf_foldin_cells: the two together, as an iteration enqueues them
  fold           bdf_newrows_update_cells (phase 2)
  all            bdf_uhat, bdf_foldin_cells and the fold: DeviceNewRows.step's launches
and, in the same run on the same users and the same scored cells, section 24's three cold launches (uhat, quad, update).  By the host
clock around `iters` iterations synchronised at both ends: one iteration of this run without and with the fold-in's launches.  From
the times: the gather rate of k_foldin_cells (one row of V, D doubles, per scored cell; the systems and uhat are n* (D^2 + 2 D) doubles
more) and its rate of substitution flops (D (D + 1) per cell, plus 2 D of the dot product).  Reads only the bundled data.  Prints one
JSON line per figure.

    python tools/foldin_probe.py [--reps 50] [--warmup 10] [--rounds 7] [--iters 100] [--D 32] [--new 1000] [--known 10]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from interval_probe import timed  # noqa: E402
from newrows_probe import iteration_us, spread  # noqa: E402


def held_out_users(B, datasets, n_new, n_known, seed=99):
    """C3's relation without n_new users: (RelationData of the others with their features, the numbers of known and scored cells,
    the movies); n_known of every held-out user's ratings are known cells, the rest the cells to score"""
    d = datasets.load_movielens(datasets.MOVIELENS_PATH) if os.path.exists(datasets.MOVIELENS_PATH) else datasets.synthetic_movielens_like()
    X = d["X"].tocsr()
    N = X.shape[0]
    F = datasets.c3_user_features("iid", n_users=N)
    rng = np.random.default_rng(seed)
    new = np.sort(rng.choice(N, size=n_new, replace=False))
    keep = np.setdiff1d(np.arange(N), new)
    users, movies = B.Entity("users", F=F[keep]), B.Entity("movies")
    rel = B.Relation(X[keep].tocsc(), "ratings", [users, movies], class_cut=2.5)
    B.setPrecision(rel, 1.5)
    Xn = X[new].tocoo()
    known = np.zeros(Xn.nnz, dtype=bool)
    for i in range(n_new):
        at = np.nonzero(Xn.row == i)[0]
        known[rng.permutation(at)[:n_known]] = True
    table = lambda sel: {"users": Xn.row[sel] + 1, "movies": Xn.col[sel] + 1, "rating": Xn.data[sel].astype(np.float64)}
    B.setNewRows(users, F[new])
    B.setNewObserved(rel, users, table(known))
    B.setNewTest(rel, users, table(~known))
    return B.RelationData(rel), int(known.sum()), int((~known).sum()), int(X.shape[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--D", type=int, default=32)
    ap.add_argument("--new", type=int, default=1000)
    ap.add_argument("--known", type=int, default=10)
    args = ap.parse_args()
    import torch
    import bdf_amd as B
    from bdf_amd import datasets
    from bdf_amd._lib import check, lib
    from bdf_amd.engine import DeviceNewRows, _ptr
    D = args.D
    rd, n_known, n_cells, M = held_out_users(B, datasets, args.new, args.known)
    rel = rd.relations[0]
    eng = B.GibbsEngine(rd, D, seed=1)
    eng.warm_device(30.0)
    for i in range(1, 11):
        eng.sweep(i)
    eng.sync()
    nr = eng.new_rows()
    observed, rel.model.new_observed = rel.model.new_observed, None
    cold = DeviceNewRows(eng, rel)                                   # section 24's path on the same users and the same scored cells
    rel.model.new_observed = observed
    ctx, st, so = eng.ctx, nr.st, nr.so
    mean, alpha, n_new = rel.model.mean_value, rel.model.alpha, nr.n_rows
    nr.step(1, (), rel.class_cut, alpha, True)                      # the states exist: the launches below are phase 2
    cold.step(1, (), rel.class_cut, alpha, True)
    eng.sync()
    stats = ctx.zeros(8)
    P, b = ctx.zeros(n_new, D, D), ctx.zeros(n_new, D)
    t = nr.term
    L = lib()
    launches = {
        "uhat": lambda: check(L.bdf_uhat(ctx.handle, nr.F.handle, D, _ptr(st.beta), _ptr(st.mu), _ptr(nr.uhat), _ptr(nr.factors))),
        "systems": lambda: check(L.bdf_row_system(ctx.handle, D, n_new, 1, C.byref(t), _ptr(nr.factors), 1, _ptr(st.Lambda), _ptr(P), _ptr(b))),
        "cells": lambda: check(L.bdf_foldin_solve(ctx.handle, D, n_new, _ptr(P), _ptr(b), nr.pairs.handle, M, _ptr(so.sample), mean, _ptr(nr.m),
                                                  _ptr(nr.qc), _ptr(nr.uhat))),
        "foldin_cells": lambda: check(L.bdf_foldin_cells(ctx.handle, D, n_new, C.byref(t), _ptr(nr.factors), 1, _ptr(st.Lambda), nr.pairs.handle, mean,
                                                         _ptr(nr.m), _ptr(nr.qc), _ptr(nr.uhat))),
        "fold": lambda: check(L.bdf_newrows_update_cells(ctx.handle, nr.pairs.handle, _ptr(nr.m), _ptr(nr.qc), alpha, None, 2, 1.0, -1.0, rel.class_cut,
                                                         1, _ptr(stats))),
        "cold_quad": lambda: check(L.bdf_newrows_quad(ctx.handle, D, so.N, _ptr(st.Lambda), _ptr(so.sample), _ptr(cold.q))),
        "cold_update": lambda: check(L.bdf_newrows_update(ctx.handle, cold.pairs.handle, D, _ptr(nr.factors), _ptr(so.sample), _ptr(cold.q), mean,
                                                          alpha, None, 2, 1.0, -1.0, rel.class_cut, 1, _ptr(stats))),
    }
    launches["all"] = lambda: nr.step(2, (), rel.class_cut, alpha, True)
    launches["cold_all_three"] = lambda: cold.step(2, (), rel.class_cut, alpha, True)
    us = {}
    with torch.cuda.stream(ctx.stream):
        launches["uhat"]()                                          # (mu_i of the new rows: what the systems' launch reads)
        for name, fn in launches.items():
            us[name] = [timed(torch, ctx.stream, args.reps, args.warmup, fn) for _ in range(args.rounds)]
            print(json.dumps({"figure": name + "_us", "new_rows": n_new, "known_cells": n_known, "cells": n_cells, "columns": M, "D": D, **spread(us[name])}))
    med = lambda xs: sorted(xs)[len(xs) // 2]
    for name, tm in (("min", min(us["cells"])), ("median", med(us["cells"])), ("max", max(us["cells"]))):
        print(json.dumps({"figure": "cells_at_" + name + "_time", "gather_GBps": round((n_cells * D + n_new * (D * D + 2 * D)) * 8 / tm / 1e3, 1),
                          "substitution_GFLOPs": round(n_cells * (D * (D + 1) + 2 * D) / tm / 1e3, 1)}))
    first = 11
    for name, after in (("iteration_without_us", None), ("iteration_with_foldin_us", lambda: nr.step(2, (), rel.class_cut, alpha, True)),
                        ("iteration_with_cold_us", lambda: cold.step(2, (), rel.class_cut, alpha, True)), ("iteration_without_again_us", None)):
        ts = []
        for _ in range(args.rounds):
            ts.append(iteration_us(eng, first, args.iters, after))
            first += args.iters
        print(json.dumps({"figure": name, "users": rd.entities[0].count, **spread(ts)}))
    cold.close()
    eng.close()


if __name__ == "__main__":
    main()
