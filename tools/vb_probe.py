"""Milliseconds per bpmf_vb iteration on MovieLens-1M (the bench's 500,000-rating test split) at D = 10 (the reference's
default) and D = 32, timed with device events around `iters` iterations after `warmup`; and one iteration of the vectorised
numpy restatement (tests/vb_restatement.py) on the host's CPUs.  Prints one JSON line per figure.

    python tools/vb_probe.py [--iters 20] [--warmup 3] [--dims 10,32] [--no-cpu]
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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dims", default="10,32")
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    import torch
    import bdf_amd as B
    from bdf_amd import datasets, _lib
    from bdf_amd.engine import Context, DevicePairs
    rd, source = datasets.movielens_relation_data(B)
    rel = rd.relations[0]
    ids = np.asfortranarray(rel.data.ids, dtype=np.int64)
    vals = np.ascontiguousarray(rel.data.values, dtype=np.float64)
    dims = np.array([rd.entities[0].count, rd.entities[1].count], dtype=np.int64)
    for D in [int(x) for x in args.dims.split(",")]:
        rng = np.random.default_rng(0)
        mu_u, mu_v = rng.standard_normal((dims[0], D)), rng.standard_normal((dims[1], D))
        ctx = Context(seed=0)
        vb = C.c_void_p()
        _lib.check(B.lib().bdf_vb_create(ctx.handle, D, dims.ctypes.data_as(_lib.c_i64p), len(vals), ids.ctypes.data_as(C.c_void_p), 8,
                                         vals.ctypes.data_as(_lib.c_dp), float(rel.model.alpha), mu_u.ctypes.data_as(_lib.c_dp),
                                         mu_v.ctypes.data_as(_lib.c_dp), C.byref(vb)))
        test = DevicePairs(ctx, rel.test_vec.ids, rel.test_vec.values)
        _lib.check(B.lib().bdf_vb_set_test(vb, test.handle, 1.0, 5.0))
        st = np.zeros(4)
        _lib.check(B.lib().bdf_vb_iterate(vb, args.warmup))
        _lib.check(B.lib().bdf_vb_stats(vb, st.ctypes.data_as(_lib.c_dp)))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ctx.stream)
        _lib.check(B.lib().bdf_vb_iterate(vb, args.iters))
        e1.record(ctx.stream)
        _lib.check(B.lib().bdf_vb_stats(vb, st.ctypes.data_as(_lib.c_dp)))
        ms = e0.elapsed_time(e1) / args.iters
        gathered = 2 * len(vals) * (D * (D + 1) // 2 + D) * 8
        print(json.dumps({"what": "vb_iteration_gpu", "D": D, "source": source, "ms_per_iteration": round(ms, 4),
                          "gathered_GB_per_iteration": round(gathered / 1e9, 3), "gather_TBps": round(gathered / ms / 1e9, 3),
                          "rmse": round(float(st[0]), 5), "rmse_train": round(float(st[1]), 5)}), flush=True)
        B.lib().bdf_vb_destroy(vb)
        test.close()
        ctx.close()
    if not args.no_cpu:
        import vb_restatement as R
        for D in [int(x) for x in args.dims.split(",")]:
            rng = np.random.default_rng(0)
            U0, V0 = B.VBModel(D, int(dims[0]), rng), B.VBModel(D, int(dims[1]), rng)
            R.run(U0, V0, ids[:, 0], ids[:, 1], vals, [], [], np.zeros(0), rel.model.alpha, 0)   # (imports, first touches)
            t0 = time.perf_counter()
            R.run(U0, V0, ids[:, 0], ids[:, 1], vals, rel.test_vec.ids[:, 0], rel.test_vec.ids[:, 1], rel.test_vec.values,
                  rel.model.alpha, 1, clamp=(1.0, 5.0), vectorised=True)
            t = time.perf_counter() - t0
            print(json.dumps({"what": "vb_iteration_cpu_numpy", "D": D, "threads": os.environ.get("OMP_NUM_THREADS"),
                              "ms_per_iteration": round(t * 1e3, 1)}), flush=True)


if __name__ == "__main__":
    main()
