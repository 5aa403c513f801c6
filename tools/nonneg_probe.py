"""The cost of the non-negative prior's row step (setNonNegative) on one GPU.  JSON lines; no assertion.

(1) MovieLens-1M-shaped synthetic data (6,040 x 3,952, the bench's 500,000-rating test split; datasets.synthetic_movielens_like),
    the item entity, at every --D (default 32 and 64), in one run:
      * the system dump (bdf_row_system: K1's dump launch, what bdf_sample_rows_nonneg launches first) and the sweep
        (bdf_nonneg_sweep on those systems), each alone,
      * bdf_sample_rows_nonneg whole (lambda, prior pack, dump, sweep),
      * the yardsticks, existing kernels on the same plan: bdf_sample_rows_spike (k_rows_ss) and the general k_rows launch
        (bdf_sample_rows with BDF_K1_GENERAL_KERNEL set and the low-rank sampler off).
    The launches are timed one after the other, `reps` times in turn after `warmup` turns, with events around each call.
(2) A many-row shape (--rows x --cols with --pairs pairs from the library's generator, datasets.synth_ratings; default
    1,000,000 x 1,000 with 10 M pairs, D = 32), the row entity non-negative, at 16 k, 64 k, 256 k rows per chunk and the default:
    the whole call and, per chunk, its share; the sweep alone on the first 64 k rows' systems and its bandwidth against
    (D^2 + 2 D) * 8 bytes per row; the share of a whole iteration (GibbsEngine.sweep, no test set) that the entity's call takes.

    python tools/nonneg_probe.py [--reps 30] [--warmup 10] [--D 32 64] [--no-many] [--rows 1000000] [--cols 1000] [--pairs 10000000]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

os.environ["BDF_K1_GENERAL_KERNEL"] = "1"          # (read once, when the library first routes a launch: the yardstick's variant)

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stats(v):
    return {"median": round(float(np.median(v)), 1), "min": round(float(np.min(v)), 1), "max": round(float(np.max(v)), 1)}


def _timed(ctx, fns, warmup, reps):
    """{name: [microseconds]}: the calls of `fns` one after the other, events around each, `reps` turns after `warmup`"""
    import torch
    times = {name: [] for name, _ in fns}
    for turn in range(warmup + reps):
        for name, fn in fns:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ctx.stream)
            fn()
            e1.record(ctx.stream)
            e1.synchronize()
            if turn >= warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    return times


def movielens(args, D):
    import bdf_amd as B
    from bdf_amd import datasets
    from bdf_amd._lib import check, lib
    X = datasets.synthetic_movielens_like()["X"]
    rel = B.Relation(X, "ratings", [B.Entity("users"), B.Entity("movies")])
    B.assignToTest(rel, datasets.split_test_ids(X.nnz, 500_000, 1))
    B.setPrecision(rel, 1.5)
    rd = B.RelationData(rel)
    eng = B.GibbsEngine(rd, D, seed=0)
    for i in range(1, 11):                         # ten Gaussian iterations: factors of a running chain
        eng.sweep(i)
    eng.sync()
    ctx, j = eng.ctx, 1
    ctx.set_lowrank(0)
    st = eng.ent[j]
    terms = eng._terms(j)
    N = st.N
    tau, state = ctx.tensor(np.ones(D)), ctx.tensor(np.concatenate([np.full(D, 0.5), np.ones(D), np.zeros(D), np.zeros(D)]))
    Lam, mu, out = ctx.tensor(np.eye(D)), ctx.zeros(D), ctx.zeros(N, D)
    P, c = ctx.zeros(N, D, D), ctx.zeros(N, D)
    u = ctx.tensor(np.abs(st.sample.cpu().numpy()))
    ctx.set_sweep(1000)
    L, h, nt = lib(), ctx.handle, len(terms)
    fns = [("dump", lambda: check(L.bdf_row_system(h, D, N, nt, terms, _p(mu), 0, _p(Lam), _p(P), _p(c)))),
           ("sweep", lambda: check(L.bdf_nonneg_sweep(h, D, N, _p(P), _p(c), _p(u), st.tag, 0, _p(out)))),
           ("nonneg_call", lambda: check(L.bdf_sample_rows_nonneg(h, D, N, nt, terms, _p(tau), _p(u), st.tag, 0, 1, _p(out)))),
           ("k_rows_ss", lambda: check(L.bdf_sample_rows_spike(h, D, N, nt, terms, _p(state), _p(u), st.tag, 0, 1, _p(out)))),
           ("k_rows_general", lambda: check(L.bdf_sample_rows(h, D, N, nt, terms, _p(mu), 0, _p(Lam), st.tag, 0, 1, _p(out), None)))]
    times = _timed(ctx, fns, args.warmup, args.reps)
    row = {"what": "item_rows", "D": D, "rows": N, "train_pairs": rel.data.nnz(), "reps": args.reps}
    for name, v in times.items():
        row[name + "_us"] = _stats(v)
    row["sweep_GBps"] = round(N * (D * D + 2 * D) * 8 / np.median(times["sweep"]) / 1e3, 1)
    print(json.dumps(row), flush=True)
    eng.close()


def many_rows(args):
    import bdf_amd as B
    from bdf_amd import datasets
    from bdf_amd._lib import check, lib
    D = 32
    rd = datasets.c4_relation_data(B, n_rows=args.rows, n_cols=args.cols, nnz=args.pairs, test_fraction=0.0)
    rel = rd.relations[0]
    B.setNonNegative(rel.entities[0])
    eng = B.GibbsEngine(rd, D, seed=0)
    for i in range(1, 4):
        eng.sweep(i)
    eng.sync()
    t0 = time.perf_counter()
    for i in range(4, 4 + args.iters):
        eng.sweep(i)
    eng.sync()
    iter_us = (time.perf_counter() - t0) * 1e6 / args.iters
    ctx, j = eng.ctx, 0
    st = eng.ent[j]
    terms = eng._terms(j)
    N = st.N
    L, h, nt = lib(), ctx.handle, len(terms)
    out = ctx.zeros(N, D)
    ctx.set_sweep(1000)
    default = (1 << 30) // ((D * D + D) * 8) // 64 * 64
    for chunk in (16384, 65536, 262144, 0):
        ctx.set_nonneg_chunk(chunk)
        fns = [("call", lambda: check(L.bdf_sample_rows_nonneg(h, D, N, nt, terms, _p(st.nonneg_tau), _p(st.sample), st.tag, 0, 1, _p(out))))]
        v = _timed(ctx, fns, 2, args.many_reps)["call"]
        rows = chunk or default
        n_chunks = -(-N // rows)
        print(json.dumps({"what": "many_rows_call", "D": D, "rows": N, "pairs": rel.data.nnz(), "rows_per_chunk": rows, "chunks": n_chunks,
                          "call_us": _stats(v), "per_chunk_us": round(float(np.median(v)) / n_chunks, 1),
                          "share_of_iteration": round(float(np.median(v)) / iter_us, 3), "iteration_us": round(iter_us, 1)}), flush=True)
    ctx.set_nonneg_chunk(0)
    n = min(N, 65536)
    rng = np.random.default_rng(0)
    A = 0.1 * rng.standard_normal((n, D, 4))
    P = ctx.tensor(np.einsum("nij,nkj->nik", A, A) + np.eye(D)[None])
    c, u, o = ctx.tensor(rng.standard_normal((n, D))), ctx.tensor(np.abs(rng.standard_normal((n, D)))), ctx.zeros(n, D)
    v = _timed(ctx, [("sweep", lambda: check(L.bdf_nonneg_sweep(h, D, n, _p(P), _p(c), _p(u), st.tag, 0, _p(o))))], args.warmup, args.reps)["sweep"]
    print(json.dumps({"what": "sweep_alone", "D": D, "rows": n, "us": _stats(v),
                      "GBps_against_(D^2+2D)*8_bytes_per_row": round(n * (D * D + 2 * D) * 8 / np.median(v) / 1e3, 1)}), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--D", type=int, nargs="+", default=[32, 64])
    ap.add_argument("--no-many", action="store_true")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--cols", type=int, default=1_000)
    ap.add_argument("--pairs", type=int, default=10_000_000)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--many-reps", type=int, default=5)
    args = ap.parse_args()
    for D in args.D:
        movielens(args, D)
    if not args.no_many:
        many_rows(args)


if __name__ == "__main__":
    main()
