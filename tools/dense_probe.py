"""The cost of a dense relation (setDense) at the MovieLens-1M shape taken as a full 6040 x 3952 matrix
(planted rank 8, noise sd 0.3), D = 32 by default, alpha fixed, no test set.  Three models of the same data:

    dense      denseRelation: the matrix on the device, the two products and the prior in front of both row launches
    explicit   every cell listed, plain Gaussian noise: what the sampler did with such a matrix before setDense
    weights    every cell listed with setWeights(ones): the weighted row kernel, which DESIGN.md section 20 timed

Whole iterations by the host clock around `iters` of them (the listed models: `iters_explicit`), synchronised at both ends, after the
engine's device warm-up; the engines take turns, `rounds` times, and the median round is reported beside all of them.  Then device
events around `reps` launches after `warmup` of every launch the dense model adds -- the Gram matrices, the two products, the two
priors -- and the products' achieved bytes per second (8 N M bytes of R per product).  One JSON line per figure.

    python tools/dense_probe.py [--D 32] [--alpha 10] [--rounds 5] [--iters 100] [--iters-explicit 3] [--no-explicit] [--N 6040] [--M 3952]
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
    ap.add_argument("--D", type=int, default=32)
    ap.add_argument("--N", type=int, default=6040)
    ap.add_argument("--M", type=int, default=3952)
    ap.add_argument("--alpha", type=float, default=10.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--iters-explicit", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--no-explicit", action="store_true")
    args = ap.parse_args()
    import torch
    import bdf_amd as B
    from bdf_amd._lib import check, lib
    D, N, M = args.D, args.N, args.M
    rng = np.random.default_rng(0)
    Y = rng.standard_normal((N, 8)) @ rng.standard_normal((M, 8)).T + 0.3 * rng.standard_normal((N, M))
    print(json.dumps({"what": "data", "N": N, "M": M, "cells": N * M, "D": D, "alpha": args.alpha, "matrix_bytes": 8 * N * M}), flush=True)

    def entities():
        return [B.Entity("rows"), B.Entity("cols")]

    models = {"dense": B.RelationData(B.denseRelation(Y, "panel", entities(), alpha=args.alpha))}
    if not args.no_explicit:
        t0 = time.perf_counter()
        ii, jj = np.meshgrid(np.arange(1, N + 1), np.arange(1, M + 1), indexing="ij")
        ids = np.stack([ii.ravel(), jj.ravel()], axis=1)
        del ii, jj
        for name in ("explicit", "weights"):
            rel = B.Relation((ids, Y.ravel()), "panel", entities(), alpha=args.alpha, dims=[N, M])
            if name == "weights":
                B.setWeights(rel, np.ones(N * M))
            models[name] = B.RelationData(rel)
        print(json.dumps({"what": "explicit_listings_built", "rows": N * M, "host_seconds": round(time.perf_counter() - t0, 1)}), flush=True)
    engines, at = {}, {}
    for name, rd in models.items():
        t0 = time.perf_counter()
        eng = B.GibbsEngine(rd, D, seed=0)
        for i in range(1, 4):
            eng.sweep(i)
        eng.sync()
        eng.warm_device(50.0)
        engines[name], at[name] = eng, 4
        print(json.dumps({"what": "engine", "model": name, "set_up_seconds": round(time.perf_counter() - t0, 1), "native": bool(eng.native),
                          "rows_dispatch": [eng.rows_dispatch(j) for j in range(2)]}), flush=True)
    per = {name: [] for name in engines}
    for _ in range(args.rounds):
        for name, eng in engines.items():
            n = args.iters if name == "dense" else args.iters_explicit
            eng.sync()
            t0 = time.perf_counter()
            for i in range(at[name], at[name] + n):
                eng.sweep(i)
            eng.sync()
            per[name].append((time.perf_counter() - t0) * 1e6 / n)
            at[name] += n
    med = {name: float(np.median(v)) for name, v in per.items()}
    for name, v in per.items():
        print(json.dumps({"what": "iteration", "model": name, "us_median": round(med[name], 1), "us_min": round(min(v), 1), "us_max": round(max(v), 1),
                          "us_rounds": [round(x, 1) for x in v]}), flush=True)
    if "explicit" in med:
        print(json.dumps({"what": "iteration_ratios", "explicit_over_dense": round(med["explicit"] / med["dense"], 1),
                          "weights_over_dense": round(med["weights"] / med["dense"], 1)}), flush=True)
    # the launches the dense model adds, one by one
    eng, rd = engines["dense"], models["dense"]
    ctx, dn = eng.ctx, eng.rel[0].dense
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    parts = {"what": "parts", "D": D}
    for j, en in enumerate(rd.entities):
        st, so = eng.ent[j], eng.ent[1 - j]
        s = eng.rel[0].fold_sums[1 - j]
        parts[f"gram_for_{en.name}_us"] = round(timed(torch, ctx.stream, args.reps, args.warmup, lambda: check(lib().bdf_hyper_sums(
            ctx.handle, D, so.N, p(so.sample), None, p(s[:D]), p(s[D:])))), 2)
        us = timed(torch, ctx.stream, args.reps, args.warmup, lambda: check(lib().bdf_dense_product(
            ctx.handle, p(dn["R"]), N, M, D, p(so.sample), j, p(dn["C"][j]))))
        parts[f"product_for_{en.name}_us"] = round(us, 2)
        parts[f"product_for_{en.name}_GBps"] = round(8.0 * N * M / us / 1e3, 1)
        parts[f"gram_product_prior_{en.name}_us"] = round(timed(torch, ctx.stream, args.reps, args.warmup, lambda: eng._row_prior(j)), 2)
        mu, is_matrix, Lam, pack = eng._row_prior(j)     # (device addresses)
        terms, nxt = eng._terms(j), ctx.zeros(st.N, D)
        parts[f"rows_{en.name}_us"] = round(timed(torch, ctx.stream, args.reps, args.warmup, lambda: check(lib().bdf_sample_rows(
            ctx.handle, D, st.N, 1, terms, mu, is_matrix, Lam, 900 + j, 0, 1, p(nxt), None))), 2)
    print(json.dumps(parts), flush=True)
    for e in engines.values():
        e.close()


if __name__ == "__main__":
    main()
