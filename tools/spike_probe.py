"""The cost of the spike-and-slab prior's row step (setSpikeAndSlab) on MovieLens-1M-shaped synthetic data
(6,040 x 3,952, the bench's 500,000-rating test split; datasets.synthetic_movielens_like), by default at D = 32, on one GPU:

  * the item entity's row launch under k_rows_ss (bdf_sample_rows_spike),
  * the same rows under the general k_rows kernel on the same plan (bdf_sample_rows with BDF_K1_GENERAL_KERNEL set and the
    low-rank sampler off: every row one K1 item, the gathers the spike launch uses too) -- existing code,
  * the hyper step (bdf_spike_hyper: two launches).

The two row launches are timed one after the other, `reps` times in turn after `warmup` turns, each with the events that ride on
the kernel's own dispatch (bdf_ctx_time_next_rows: the prior's small pre-launches are outside); the hyper step with events around
`reps` calls.  Prints the medians, their ratio and the runs' spread (min, max) as JSON lines.

Then the view-by-component activity matrix of a planted two-view GFA model (200 samples; views of 30 and 25 columns; two shared
components, one of view 1 only, one of view 2 only; D = 8): the posterior activity of every component in either view's
spike-and-slab column entity.  No assertion is made on either.

    python tools/spike_probe.py [--reps 30] [--warmup 10] [--D 32] [--no-gfa]

--D 64 shows what one wave per SIMD costs the D > 32 variant; --no-gfa leaves the planted model out.
"""
import argparse
import ctypes as C
import json
import os
import sys

os.environ["BDF_K1_GENERAL_KERNEL"] = "1"          # (read once, when the library first routes a launch)

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _p(t):
    return C.c_void_p(t.data_ptr())


def rows_and_hyper(args):
    import torch
    import bdf_amd as B
    from bdf_amd import datasets
    from bdf_amd._lib import check, lib
    from bdf_amd.engine import KernelTimer
    D = args.D
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
    state = ctx.tensor(np.concatenate([np.full(D, 0.5), np.ones(D), np.zeros(D), np.zeros(D)]))
    Lam, mu, out = ctx.tensor(np.eye(D)), ctx.zeros(D), ctx.zeros(st.N, D)
    ctx.set_sweep(1000)

    def spike():
        check(lib().bdf_sample_rows_spike(ctx.handle, D, st.N, len(terms), terms, _p(state), _p(st.sample), st.tag, 0, 1, _p(out)))

    def general():
        check(lib().bdf_sample_rows(ctx.handle, D, st.N, len(terms), terms, _p(mu), 0, _p(Lam), st.tag, 0, 1, _p(out), None))

    times = {"k_rows_ss": [], "k_rows_general": []}
    for turn in range(args.warmup + args.reps):
        for name, fn in (("k_rows_ss", spike), ("k_rows_general", general)):
            t = KernelTimer()
            check(lib().bdf_ctx_time_next_rows(ctx.handle, t.start, t.stop))
            fn()
            ctx.sync()
            if turn >= args.warmup:
                times[name].append(t.elapsed_us())
    disp = ctx.rows_dispatch(st.tag)
    row = {"what": "item_rows", "D": D, "rows": st.N, "train_pairs": rel.data.nnz(), "reps": args.reps, "dispatch_of_the_last_launch": disp}
    for name, v in times.items():
        row[name + "_us"] = {"median": round(float(np.median(v)), 1), "min": round(float(np.min(v)), 1), "max": round(float(np.max(v)), 1)}
    row["ss_over_general"] = round(float(np.median(times["k_rows_ss"]) / np.median(times["k_rows_general"])), 3)
    print(json.dumps(row), flush=True)

    def hyper():
        check(lib().bdf_spike_hyper(ctx.handle, D, st.N, _p(out), 1.0, 1.0, 1.0, 1.0, st.tag, _p(state)))

    spike()
    hs = []
    for turn in range(5):
        for _ in range(args.warmup):
            hyper()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ctx.stream)
        for _ in range(args.reps):
            hyper()
        e1.record(ctx.stream)
        e1.synchronize()
        hs.append(e0.elapsed_time(e1) * 1e3 / args.reps)
    print(json.dumps({"what": "hyper_step", "D": D, "rows": st.N, "us": {"median": round(float(np.median(hs)), 2), "min": round(float(np.min(hs)), 2),
                                                                         "max": round(float(np.max(hs)), 2)}}), flush=True)
    eng.close()


def gfa():
    import bdf_amd as B
    rng = np.random.default_rng(0)
    N, M1, M2, D = 200, 30, 25, 8
    Z = rng.standard_normal((N, 4))
    W1, W2 = rng.standard_normal((M1, 4)), rng.standard_normal((M2, 4))
    W1[:, 3] = 0.0                                  # components 0, 1 shared; 2 in view 1 only; 3 in view 2 only
    W2[:, 2] = 0.0
    samples, v1, v2 = B.Entity("samples"), B.Entity("view1"), B.Entity("view2")
    rd = B.RelationData()
    for name, W, M, en in (("x1", W1, M1, v1), ("x2", W2, M2, v2)):
        Y = Z @ W.T + 0.3 * rng.standard_normal((N, M))
        i, k = np.meshgrid(np.arange(1, N + 1), np.arange(1, M + 1), indexing="ij")
        rel = B.Relation({"samples": i.ravel(), en.name: k.ravel(), "y": Y.ravel()}, name, [samples, en], alpha=1.0 / 0.09, dims=[N, M])
        B.addRelation(rd, rel)
    B.setSpikeAndSlab(v1)
    B.setSpikeAndSlab(v2)
    res = B.macau(rd, num_latent=D, burnin=150, psamples=100, verbose=False, seed=3)
    rd._engine.close()
    act = np.stack([res["spike"]["view1"]["activity"], res["spike"]["view2"]["activity"]])
    order = np.argsort(-act.sum(axis=0))
    print(json.dumps({"what": "gfa_activity", "planted": "2 shared, 1 of view 1 only, 1 of view 2 only; D = 8", "components_by_total_activity": order.tolist(),
                      "view1": np.round(act[0, order], 3).tolist(), "view2": np.round(act[1, order], 3).tolist()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--D", type=int, default=32)
    ap.add_argument("--no-gfa", action="store_true")
    args = ap.parse_args()
    rows_and_hyper(args)
    if not args.no_gfa:
        gfa()


if __name__ == "__main__":
    main()
