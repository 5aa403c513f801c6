"""The cost and the gain of background cells (setBackground) on MovieLens-1M as implicit data: the ratings
of 4 and 5 are the listed cells and all hold 1; held out are a fifth of them and as many unlisted cells (value 0).  D = 32 by
default, alpha and c0 fixed.  Three models of the same data:

    background   the listed cells + setBackground(rel, c0): the fold in front of both row launches, the rows on K1c
    listed       the listed cells alone: what the sampler saw before (all residuals zero)
    explicit     every cell of the N x M matrix listed, with setWeights (1 on the listed ones, c0 on the rest): the same model as
                 `background` through the code as it stood before setBackground, k_rows_w over 24 M rows

Whole iterations by the host clock around `iters` of them (the explicit model: `iters_explicit`), synchronised at both ends, after
the engine's device warm-up; the three engines take turns, `rounds` times, and the median round is reported beside all of them.
The difference between `background` and `listed` is split with device events around `reps` launches after `warmup`: the two
bdf_hyper_sums launches, the two bdf_background_prior launches, and each entity's row launch with the folded and with the plain
prior.  Then the held-out AUC of `background` and `listed` after burnin + psamples iterations.  One JSON line per figure.

    python tools/background_probe.py [--D 32] [--c0 0.1] [--alpha 10] [--rounds 5] [--iters 200] [--iters-explicit 3] [--no-explicit]
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


def implicit_movielens(seed=1):
    """(N, M, train ids, test ids, test values, source): ids 1-based (n, 2)"""
    from bdf_amd import datasets
    try:
        X, source = datasets.load_movielens()["X"], "movielens_1m.mat"
    except (OSError, ValueError):
        X, source = datasets.synthetic_movielens_like()["X"], "synthetic"
    coo = X.tocoo()
    N, M = X.shape
    keep = coo.data >= 4
    ones = np.stack([coo.row[keep], coo.col[keep]], axis=1).astype(np.int64)
    rng = np.random.default_rng(seed)
    ones = ones[rng.permutation(len(ones))]
    nt = len(ones) // 5
    listed = np.zeros(N * M, dtype=bool)
    listed[ones[:, 0] * M + ones[:, 1]] = True
    free = np.flatnonzero(~listed)
    z = rng.choice(free, size=nt, replace=False)
    test = np.concatenate([ones[:nt], np.stack([z // M, z % M], axis=1)]) + 1
    return N, M, ones[nt:] + 1, test, np.concatenate([np.ones(nt), np.zeros(nt)]), source


def relation_data(B, N, M, ids, y, test, tv, alpha, weights=None, background=None):
    rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "plays", [B.Entity("users"), B.Entity("movies")], class_cut=0.5, alpha=alpha,
                     dims=[N, M])
    B.setTest(rel, {"u": test[:, 0], "v": test[:, 1], "y": tv})
    if weights is not None:
        B.setWeights(rel, weights)
    if background is not None:
        B.setBackground(rel, background)
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
    ap.add_argument("--D", type=int, default=32)
    ap.add_argument("--c0", type=float, default=0.1)
    ap.add_argument("--alpha", type=float, default=10.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--iters-explicit", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--burnin", type=int, default=20)
    ap.add_argument("--psamples", type=int, default=20)
    ap.add_argument("--no-explicit", action="store_true")
    args = ap.parse_args()
    import torch
    import bdf_amd as B
    from bdf_amd._lib import check, lib
    D, c0 = args.D, args.c0
    N, M, ids, test, tv, source = implicit_movielens()
    ones = np.ones(len(ids))
    print(json.dumps({"what": "data", "source": source, "N": N, "M": M, "listed": len(ids), "cells": N * M, "test": len(test), "D": D,
                      "c0": c0, "alpha": args.alpha}), flush=True)
    models = {"background": relation_data(B, N, M, ids, ones, test, tv, args.alpha, background=c0),
              "listed": relation_data(B, N, M, ids, ones, test, tv, args.alpha)}
    if not args.no_explicit:
        t0 = time.perf_counter()
        W = np.full((N, M), c0)
        W[ids[:, 0] - 1, ids[:, 1] - 1] = 1.0
        Y = np.zeros((N, M))
        Y[ids[:, 0] - 1, ids[:, 1] - 1] = 1.0
        ii, jj = np.meshgrid(np.arange(1, N + 1), np.arange(1, M + 1), indexing="ij")
        models["explicit"] = relation_data(B, N, M, np.stack([ii.ravel(), jj.ravel()], axis=1), Y.ravel(), test, tv, args.alpha, weights=W.ravel())
        del W, Y, ii, jj
        print(json.dumps({"what": "explicit_listing_built", "rows": N * M, "host_seconds": round(time.perf_counter() - t0, 1)}), flush=True)
    engines, at = {}, {}
    for name, rd in models.items():
        t0 = time.perf_counter()
        eng = B.GibbsEngine(rd, D, seed=0)
        rel = rd.relations[0]
        eng.register_test((), rel.class_cut)
        for i in range(1, 4):
            eng.step(i, 0, (), rel.class_cut)
        eng.sync()
        eng.warm_device(50.0)
        engines[name], at[name] = eng, 4
        print(json.dumps({"what": "engine", "model": name, "set_up_seconds": round(time.perf_counter() - t0, 1), "mean_value": rel.model.mean_value,
                          "rows_dispatch": [eng.rows_dispatch(j) for j in range(2)]}), flush=True)
    # whole iterations, the engines taking turns
    per = {name: [] for name in engines}
    for _ in range(args.rounds):
        for name, eng in engines.items():
            n = args.iters_explicit if name == "explicit" else args.iters
            cut = models[name].relations[0].class_cut
            eng.sync()
            t0 = time.perf_counter()
            for i in range(at[name], at[name] + n):
                eng.step(i, 0, (), cut)
            eng.sync()
            per[name].append((time.perf_counter() - t0) * 1e6 / n)
            at[name] += n
    med = {name: float(np.median(v)) for name, v in per.items()}
    for name, v in per.items():
        print(json.dumps({"what": "iteration", "model": name, "us_median": round(med[name], 1), "us_rounds": [round(x, 1) for x in v]}), flush=True)
    row = {"what": "iteration_ratios", "background_over_listed": round(med["background"] / med["listed"], 2),
           "background_minus_listed_us": round(med["background"] - med["listed"], 1)}
    if "explicit" in med:
        row["explicit_over_background"] = round(med["explicit"] / med["background"], 1)
    print(json.dumps(row), flush=True)
    # where the difference goes: the sums, the fold, the rows
    eng, rd = engines["background"], models["background"]
    plain = engines["listed"]
    ctx, rel, dr = eng.ctx, rd.relations[0], eng.rel[0]
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    ctx.set_sweep(100000)
    parts = {"what": "parts", "D": D}
    for j, en in enumerate(rd.entities):
        st, so = eng.ent[j], eng.ent[1 - j]
        s = dr.fold_sums[1 - j]
        parts[f"sums_{en.name}_us"] = round(timed(torch, ctx.stream, args.reps, args.warmup, lambda: check(lib().bdf_hyper_sums(
            ctx.handle, D, so.N, p(so.sample), None, p(s[:D]), p(s[D:])))), 2)
        parts[f"sums_and_fold_{en.name}_us"] = round(timed(torch, ctx.stream, args.reps, args.warmup, lambda: eng._row_prior(j)), 2)
        mu, _, Lam, pack = eng._row_prior(j)             # (device addresses)
        terms, nxt = eng._terms(j), ctx.zeros(st.N, D)
        parts[f"rows_{en.name}_folded_prior_us"] = round(timed(torch, ctx.stream, args.reps, args.warmup, lambda: check(lib().bdf_sample_rows(
            ctx.handle, D, st.N, 1, terms, mu, 0, Lam, 900 + j, 0, 1, p(nxt), pack))), 2)
        pst, pterms = plain.ent[j], plain._terms(j)
        parts[f"rows_{en.name}_plain_prior_us"] = round(timed(torch, plain.ctx.stream, args.reps, args.warmup, lambda: check(lib().bdf_sample_rows(
            plain.ctx.handle, D, pst.N, 1, pterms, p(pst.mu), 0, p(pst.Lambda), 900 + j, 0, 1, p(nxt), p(pst.prior_pack)))), 2)
    print(json.dumps(parts), flush=True)
    for e in engines.values():
        e.close()
    # what the background buys: held-out AUC
    for name in ("background", "listed"):
        rd = relation_data(B, N, M, ids, ones, test, tv, args.alpha, background=c0 if name == "background" else None)
        res = B.macau(rd, num_latent=D, burnin=args.burnin, psamples=args.psamples, verbose=False, seed=0)
        print(json.dumps({"what": "held_out", "model": name, "AUC": round(float(res["ROC"]), 4), "burnin": args.burnin, "psamples": args.psamples}), flush=True)
        rd._engine.close()


if __name__ == "__main__":
    main()
