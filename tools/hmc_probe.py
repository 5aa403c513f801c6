"""Milliseconds per macau_hmc iteration on MovieLens-1M (the bench's test split) at D = 10 (the reference's default) and
D = 32 with L = 10, L_inner = 1, eps = 0.01, timed with device events around every iteration (the host waits for each
iteration's decision before it enqueues the next leapfrog, so the device time includes that hand-over); the acceptance
rate and how eps and L adapt; and one iteration of the vectorised numpy restatement (tests/hmc_restatement.py) on the
host's CPUs.  Prints one JSON line per figure.  A run stops early once the adapted L exceeds --max-L.

    python tools/hmc_probe.py [--iters 40] [--dims 10,32] [--max-L 400] [--no-cpu] [--no-gpu]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--dims", default="10,32")
    ap.add_argument("--max-L", type=int, default=400)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-gpu", action="store_true")
    args = ap.parse_args()
    import bdf_amd as B
    from bdf_amd import datasets, _lib
    rd, source = datasets.movielens_relation_data(B)
    rel = rd.relations[0]
    ids = np.asfortranarray(rel.data.ids, dtype=np.int64)
    vals = np.ascontiguousarray(rel.data.values, dtype=np.float64)
    dims = np.array([rd.entities[0].count, rd.entities[1].count], dtype=np.int64)
    check, lib = _lib.check, B.lib()
    for D in ([] if args.no_gpu else [int(x) for x in args.dims.split(",")]):
        import torch
        from bdf_amd.engine import Context, DevicePairs
        ctx = Context(seed=0)
        h = C.c_void_p()
        check(lib.bdf_hmc_create(ctx.handle, D, dims.ctypes.data_as(_lib.c_i64p), len(vals), ids.ctypes.data_as(C.c_void_p), 8,
                                 vals.ctypes.data_as(_lib.c_dp), float(rel.model.alpha), C.byref(h)))
        test = DevicePairs(ctx, rel.test_vec.ids, rel.test_vec.values)
        check(lib.bdf_hmc_set_test(h, test.handle, 1.0, 5.0))
        check(lib.bdf_hmc_set_params(h, 10, 1, 8, 0.01, args.iters // 2))
        st = np.zeros(16)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.iters)]
        recs = []
        t0 = time.perf_counter()
        for i in range(args.iters):
            ev[i][0].record(ctx.stream)
            check(lib.bdf_hmc_iterate(h, 1))
            ev[i][1].record(ctx.stream)
            check(lib.bdf_hmc_stats(h, st.ctypes.data_as(_lib.c_dp), None, 0))
            recs.append(st.copy())
            if st[10] > args.max_L:
                break
        wall = (time.perf_counter() - t0) / len(recs)
        # iterations with the starting L = 10 (21 leapfrog launches), after the first (warm-up)
        ms = [ev[i][0].elapsed_time(ev[i][1]) for i in range(len(recs))]
        at10 = [m for m, r in zip(ms[1:], recs[1:]) if r[2] == 10]
        print(json.dumps({"what": "hmc_iteration_gpu", "D": D, "source": source, "iterations": len(recs),
                          "ms_per_iteration_at_L10": round(float(np.median(at10)), 4) if at10 else None,
                          "us_per_launch_at_L10": round(float(np.median(at10)) * 1e3 / 24, 2) if at10 else None,
                          "wall_ms_per_iteration_with_stats": round(wall * 1e3, 3),
                          "accepted": int(sum(r[8] for r in recs)), "L_sequence": [int(r[2]) for r in recs],
                          "eps_final": float(recs[-1][9]), "dH": [round(float(r[7]), 2) for r in recs],
                          "rmse": round(float(recs[-1][14]), 5), "rmse_avg": round(float(recs[-1][15]), 5)}), flush=True)
        # the cost of the per-iteration decision hand-over: n iterations in one call (host waits for each decision) against
        # the same n with the wait ... measured as wall time per iteration of one bdf_hmc_iterate(n) call
        check(lib.bdf_hmc_set_params(h, 10, 1, 8, 1e-6, 0))
        n = 10
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(ctx.stream)
        check(lib.bdf_hmc_iterate(h, n))
        e1.record(ctx.stream)
        check(lib.bdf_hmc_stats(h, st.ctypes.data_as(_lib.c_dp), None, 0))
        wall = (time.perf_counter() - t0) / n
        print(json.dumps({"what": "hmc_iterate_n", "D": D, "n": n, "L": int(st[2]),
                          "device_ms_per_iteration": round(e0.elapsed_time(e1) / n, 4),
                          "wall_ms_per_iteration": round(wall * 1e3, 4)}), flush=True)
        lib.bdf_hmc_destroy(h)
        test.close()
        ctx.close()
    if not args.no_cpu:
        import hmc_restatement as H
        for D in [int(x) for x in args.dims.split(",")]:
            t0 = time.perf_counter()
            H.run(ids[:, 0], ids[:, 1], vals, rel.test_vec.ids[:, 0], rel.test_vec.ids[:, 1], rel.test_vec.values,
                  int(dims[0]), int(dims[1]), D, rel.model.alpha, 0, L=10, clamp=(1.0, 5.0), vectorised=True, niter=1)
            t = time.perf_counter() - t0
            print(json.dumps({"what": "hmc_iteration_cpu_numpy", "D": D, "L": 10, "threads": os.environ.get("OMP_NUM_THREADS"),
                              "ms_per_iteration": round(t * 1e3, 1)}), flush=True)


if __name__ == "__main__":
    main()
