"""AUC_ROC on the device (bdf_auc_roc, csrc/k_auc.hip) and what it saves in a verbose macau().  Prints one JSON line per figure:

* auc_device: milliseconds per bdf_auc_roc call at n = 10^4, 5 10^5 and 5 10^6, random scores and heavy ties (200 values),
  timed with device events around `iters` back-to-back calls after `warmup` (workspace allocated beforehand);
* auc_host_numpy: the host AUC_ROC (driver.AUC_ROC, numpy) on the same 5 10^5 scores -- what the verbose report paid per
  iteration before, with the copies of the running average and of the factor matrices (host_report_ms);
* macau_wall: wall milliseconds per iteration of macau() on MovieLens-1M (500,000 held out) at D = 32, verbose=True (the
  report at every iteration, stdout to /dev/null) against verbose=False.

    python tools/auc_probe.py [--iters 50] [--warmup 5] [--burnin 50] [--psamples 50] [--no-macau]
"""
import argparse
import contextlib
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def time_device_auc(args):
    import torch
    import bdf_amd as B
    from bdf_amd import _lib, driver
    from bdf_amd.engine import Context
    ctx = Context(seed=0)
    L = B.lib()
    rng = np.random.default_rng(0)
    for n in (10_000, 500_000, 5_000_000):
        for kind in ("random", "ties"):
            s = rng.standard_normal(n) if kind == "random" else np.round(rng.random(n) * 199.0)
            lab = rng.random(n) < 0.4
            t_s = torch.as_tensor(s, device=ctx.device)
            t_l = torch.as_tensor(lab, device=ctx.device).view(torch.uint8)
            ws = torch.empty(L.bdf_auc_workspace_bytes(n), dtype=torch.uint8, device=ctx.device)
            out = torch.zeros(4, dtype=torch.int64, device=ctx.device)
            call = lambda: _lib.check(L.bdf_auc_roc(ctx.handle, n, C.c_void_p(t_l.data_ptr()), C.c_void_p(t_s.data_ptr()),
                                                    C.c_void_p(ws.data_ptr()), C.c_void_p(out.data_ptr()),
                                                    C.c_void_p(out.data_ptr() + 8)))
            torch.cuda.synchronize()
            for _ in range(args.warmup):
                call()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ctx.stream)
            for _ in range(args.iters):
                call()
            e1.record(ctx.stream)
            ctx.sync()
            ms = e0.elapsed_time(e1) / args.iters
            h = out.cpu().numpy()
            auc = float(h[:1].view(np.float64)[0])
            rec = {"what": "auc_device", "n": n, "scores": kind, "ms_per_call": round(ms, 4), "auc": auc}
            if n == 500_000:
                t0 = time.perf_counter()
                host = driver.AUC_ROC(lab, s)
                rec["host_numpy_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
                rec["abs_diff_vs_host"] = abs(auc - host)
            print(json.dumps(rec), flush=True)
    ctx.close()


def time_macau(args):
    import bdf_amd as B
    from bdf_amd import datasets, driver
    D = 32
    out = {}
    for verbose in (False, True):
        rd, source = datasets.movielens_relation_data(B)
        with open(os.devnull, "w") as null, contextlib.redirect_stdout(null):
            B.macau(rd, num_latent=D, burnin=2, psamples=2, verbose=verbose, seed=1)        # (first launches, allocations)
            t0 = time.perf_counter()
            B.macau(rd, num_latent=D, burnin=args.burnin, psamples=args.psamples, verbose=verbose, seed=1)
            t = time.perf_counter() - t0
        out[verbose] = t * 1e3 / (args.burnin + args.psamples)
    # what the report cost per iteration before it moved to the device: the running average and every factor matrix copied
    # to the host, the numpy AUC and norms (measured on the final state of the last run)
    eng = rd._engine
    rel = rd.relations[0]
    t0 = time.perf_counter()
    eng.sync()
    avg, _ = eng.test_pairs().state()
    driver.AUC_ROC(rel.test_label, -avg)
    for en in rd.entities:
        np.linalg.norm(en.model.sample)
    host_report_ms = (time.perf_counter() - t0) * 1e3
    print(json.dumps({"what": "macau_wall", "D": D, "source": source, "iterations": args.burnin + args.psamples,
                      "ms_per_iteration_quiet": round(out[False], 3), "ms_per_iteration_verbose": round(out[True], 3),
                      "host_report_ms": round(host_report_ms, 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--burnin", type=int, default=50)
    ap.add_argument("--psamples", type=int, default=50)
    ap.add_argument("--no-macau", action="store_true")
    args = ap.parse_args()
    time_device_auc(args)
    if not args.no_macau:
        time_macau(args)


if __name__ == "__main__":
    main()
