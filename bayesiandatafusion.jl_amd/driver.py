"""macau() -- the Gibbs driver of the reference (src/macau.jl:3-255) over the device engine.

Same keyword surface and result keys as the reference.  Worker-process arguments (latent_pids, latent_blas_threads,
cg_pids) are accepted for drop-in compatibility; the GPU replaces the worker pool, so they only decide the
"latent_multi_threading" flag the reference reports (macau.jl:44-66, 253).  Extra keywords: seed, device.
"""
import math
import struct
import sys
import time

import numpy as np

from . import features as feat
from ._lib import ArgumentError
from .engine import GibbsEngine
from .model_options import refuse
from .relation_data import _ordinal_bounds, _waic_bounds, check_new_rows, check_test_interval, hasFeatures, numTest, toStr


def AUC_ROC(Ytrue, scores):
    """src/ROC.jl:1-11.  Scores in a GPU torch tensor (float64; labels a bool or uint8 tensor) are ranked on the device
    (bdf_auc_roc, csrc/k_auc.hip) and give a float; anything else takes the host path below."""
    if _on_gpu(scores):
        from .engine import device_auc_roc
        return device_auc_roc(Ytrue, scores)[0]
    Ytrue = np.asarray(Ytrue, dtype=bool)
    perm = np.argsort(scores, kind="stable")
    roc_y = Ytrue[perm]
    if roc_y.sum() == 0 or (~roc_y).sum() == 0:
        return float("nan")
    stack_x = np.cumsum(roc_y) / roc_y.sum()
    stack_y = np.cumsum(~roc_y) / (~roc_y).sum()
    return float(np.sum((stack_x[1:] - stack_x[:-1]) * stack_y[1:]))


def _on_gpu(x):
    torch = sys.modules.get("torch")          # (a tensor exists only if torch is loaded: numpy callers do not import it)
    return torch is not None and torch.is_tensor(x) and x.device.type == "cuda"


def makeClamped(x, clamp):
    """src/sampling.jl:99-106"""
    if len(clamp) == 0:
        return x
    return np.clip(x, clamp[0], clamp[1])


from .data_reading import read_binary_float32, write_binary_matrix  # noqa: E402,F401  (src/data_reading.jl:61-67, 93-99)


def macau(data, num_latent=10, lambda_beta=float("nan"), burnin=500, psamples=200, verbose=True, full_lambda_u=True,
          reset_model=True, compute_ff_size=6500, latent_pids=(1,), latent_blas_threads=1, cg_pids=(1,),
          full_prediction=False, rmse_train=False, tol=float("nan"), output="", output_beta=False, output_type="csv",
          clamp=(), f=False, seed=0, device=None, engine=None, lpd=False):
    if output_beta and not output:
        raise ArgumentError("To output samples of beta ('output_beta = true') you have to set also output prefix, "
                            "e.g., output = \"my_model\".")
    if output_type not in ("csv", "binary"):
        raise ArgumentError("output_type must be either \"csv\" or \"binary\".")
    clamp = [float(c) for c in clamp]
    # what the first relation's options rule out for this run (model_options.py); the robust noise model and a noise precision per
    # row of one entity (setRobust, setEntityNoise; DESIGN.md sections 18, 22) are sampled on any relation, reported for the first
    for key, asked in (("full_prediction", full_prediction), ("rmse_train", rmse_train), ("lpd", lpd)):
        if asked and data.relations:
            refuse(data.relations[0], key)
    robust = data.relations[0].model.robust if data.relations else None
    noise = data.relations[0].model.entity_noise if data.relations else None
    # cells of rows that were not in training (setNewRows / setNewTest on the first relation), with
    # setNewObserved conditioned on known cells of their own (section 29)
    new_rel = check_new_rows(data)
    if lpd and not (data.relations and numTest(data.relations[0]) > 0) and new_rel is None:
        raise ArgumentError("lpd = true scores held-out cells: the first relation has no test cells (assignToTest / setTest).")

    # top-K lists (setRecommend) are kept for the first relation, like lpd and WAIC
    for r in data.relations[1:]:
        if r.model.recommend is not None:
            raise ArgumentError(f"Relation {r.name} asks for top-k lists (setRecommend) but is not the first relation: macau() keeps the sum of scores for the first relation only.")
    recommend = data.relations[0].model.recommend if data.relations else None
    # acquisition lists (setAcquire) likewise
    for r in data.relations[1:]:
        if r.model.acquire is not None:
            raise ArgumentError(f"Relation {r.name} asks for acquisition lists (setAcquire) but is not the first relation: macau() keeps the moments of scores for the first relation only.")
    acquire = data.relations[0].model.acquire if data.relations else None

    # WAIC on the training cells (setWaic on the first relation)
    waic = data.relations[0].model.waic if data.relations else None
    if waic is not None and psamples < 2:
        raise ArgumentError("WAIC (setWaic) needs the variance of the log-likelihood over the posterior draws: psamples must be at least 2.")

    verbose and print("Model setup")
    eng = engine
    if eng is None or reset_model:
        eng = GibbsEngine(data, num_latent, seed=seed, device=device, lambda_beta=lambda_beta,
                          compute_ff_size=compute_ff_size, full_lambda_u=full_lambda_u, tol=tol)
    if lpd and eng.world > 1:
        raise ArgumentError("lpd = true is not possible with more than one rank: every rank scores only the test cells it predicts.")
    if waic is not None and eng.world > 1:
        raise ArgumentError("WAIC (setWaic) is not possible with more than one rank: every rank holds the state of its own cells only.")
    if new_rel is not None:
        check_new_rows(data, eng.world)
    data._engine = eng
    if eng is engine and (recommend is not None or eng.scores is not None):
        eng.begin_scores()                                   # (an engine that is reused starts the sum of scores again)
    if eng is engine and (acquire is not None or eng.acquire is not None):
        eng.begin_acquire()                                  # (... and the moment planes)
    if robust is not None:
        eng.rel[0].omega_sum = None                          # (an engine that is reused starts the posterior mean of omega again)
    if noise is not None:
        eng.rel[0].tau_sum = None                            # (... and of tau)
    # relations with biases (setBias): sampled on any relation, the verbose line shows the first one's
    biased = any(dr.bias is not None for dr in eng.rel)
    if biased:
        eng.bias_reset()                                     # (... and of the biases and their precisions)
    # entities with the spike-and-slab prior (setSpikeAndSlab)
    spiked = [st for st in eng.ent if st.spike is not None]
    if eng is engine:
        for st in spiked:
            st.spike_reset()                                 # (... and of the spike-and-slab result)
    # entities with the non-negative prior (setNonNegative)
    nonneg = [st for st in eng.ent if st.nonneg is not None]
    if eng is engine:
        for st in nonneg:
            st.nonneg_reset()                                # (... and of the non-negative result)
    D = eng.D

    latent_multi_threading = (len(latent_pids) >= 1 and len(data.relations) == 1 and not hasFeatures(data.relations[0]))
    if verbose:
        if latent_multi_threading:
            print("Sampling of latent vectors: all rows of an entity in one GPU launch.")
        else:
            print("Sampling of latent vectors: general (multi-relation) GPU path.")

    rel = data.relations[0]
    haveTest = numTest(rel) > 0
    test = eng.test_pairs() if haveTest else None
    train = eng.train_pairs() if rmse_train else None
    # (nothing is allocated or launched for new rows unless setNewTest was called)
    newr = eng.new_rows(fresh=True) if new_rel is not None else None
    new_rep = np.full(10, np.nan)
    lpd_new, lpd = lpd, (lpd and haveTest)
    lpd_bounds, lpd_avg = None, float("nan")
    # ordinal first relation with sampled edges: a trace row per iteration, the step size adapted in the burn-in
    ordinal = eng.ordinal_begin(burnin, psamples) if rel.model.ordinal is not None else None
    lpd_codes = None
    if lpd:
        # held-out log predictive density: what kind of record every test cell is -- a 0/1 value of a probit
        # relation, an interval (setTestInterval / setTestBinned), a level of an ordinal relation (setTestOrdinal) or a measurement
        if rel.model.test_interval is not None:
            check_test_interval(rel)
            lpd_bounds = test.ctx.tensor(rel.model.test_interval)
        elif rel.model.test_ordinal is not None:
            # the levels' bins between the fixed edges, once; between sampled edges they follow every draw (refreshed below)
            lpd_bounds = test.ctx.tensor(_ordinal_bounds(rel.model.test_ordinal, np.arange(1, rel.model.ordinal["K"]) + 0.5))
            if ordinal is not None:
                import torch
                lpd_codes = test.ctx.tensor(rel.model.test_ordinal, dtype=torch.int8)
    waic_pairs = waic_bounds = waic_codes = None
    waic_stats = np.full(4, np.nan)
    if waic is not None:
        # what kind of record every training row is (the table of DESIGN.md section 17), built once on the host; between sampled
        # edges the levels' bins follow every draw (refreshed below, from the levels the sampler itself keeps on the device)
        waic_pairs = eng.train_pairs()
        b = _waic_bounds(rel)
        if b is not None:
            waic_bounds = waic_pairs.ctx.tensor(b)
        if ordinal is not None:
            waic_codes = rel._dev.ord_codes
    f_output = []
    yhat_full = None
    if full_prediction:
        if hasFeatures(rel):
            raise ArgumentError("Prediction of all elements is not possible when Relation has features.")   # sampling.jl:92-94
        import torch
        yhat_full = torch.zeros(tuple(rel.data.dims), dtype=torch.float64, device=eng.ctx.device)
    rmse_avg = roc_avg = err_avg = float("nan")

    verbose and print("Sampling")
    for i in range(1, burnin + psamples + 1):
        time0 = time.time()
        # relation models (alpha, relation beta) first, then rows, hyperpriors, beta (macau.jl:83-140), then the reporting
        # step on the test pairs (macau.jl:142-184); without side information all of it is one native call
        phase = 0 if i <= burnin else (1 if i == burnin + 1 else 2)
        if haveTest:
            eng.step(i, phase, clamp, rel.class_cut)
        else:
            eng.sweep(i)
        facs = eng.factors_of(rel)
        if full_prediction and i > burnin:
            yhat_full += eng.pred_all(rel)                    # macau.jl:145-147: a plain dense product, on the device
        if recommend is not None and i > burnin:
            eng.scores.push(facs[0], facs[1])                 # this draw's factors into the ring, on the row stream (a full ring: one accumulate launch)
        if acquire is not None and i > burnin:
            # this draw's factors and its precision into the ring, on the row stream; a sampled alpha is the device scalar of the native
            # iteration, drawn on this stream, and step by step the double the host has read from it
            rm = rel.model
            eng.acquire.push(facs[0], facs[1], rel._dev.alpha_dev if (rm.alpha_sample and eng.native) else rm.alpha)
        if robust is not None and i > burnin:
            eng.robust_accumulate()                           # this iteration's omega into its running sum, on the row stream
        if noise is not None and i > burnin:
            eng.entity_noise_accumulate()                     # this iteration's tau into its running sum, on the row stream
        if biased and i > burnin:
            eng.bias_accumulate()                             # this iteration's biases and precisions into their running sums, on the row stream
        if spiked and i > burnin:
            eng.spike_accumulate()                            # this draw's inclusions, pi and tau into their running sums, on the row stream
        if nonneg and i > burnin:
            eng.nonneg_accumulate()                           # this draw's rows and tau into their running sums, on the row stream
        if lpd or waic is not None or newr is not None:
            # (alpha sampled: the device scalar of the native iteration, drawn on the stream this runs on; step by step the host
            # has read the same double, and the device scalar is redrawn on another stream than the pairs')
            a = 1.0 if rel.model.probit else (rel._dev.alpha_dev if (rel.model.alpha_sample and eng.native) else rel.model.alpha)
        if lpd:
            if lpd_codes is not None:
                # this draw's edges were published on the row stream before this iteration's rows, which the pairs' stream is behind
                ordinal.bounds(test.ctx, lpd_codes, lpd_bounds)
            test.lpd_update(D, facs, rel.model.mean_value, a, phase, lpd_bounds)
            if (lpd_codes is not None or noise is not None) and test.ctx is not eng.ctx:
                # (step by step the pairs have a stream of their own: the next iteration's step may not publish its edges -- or redraw
                # the tau that the cells are scored with -- under this launch.  The native iteration scores on the row stream itself
                # and needs nothing)
                eng.ctx.stream.wait_stream(test.ctx.stream)
        if newr is not None:
            # uhat of the new rows, q of the other entity's rows and the cells' update, on the row stream behind this iteration's last
            # launch: beta, V, (mu, Lambda) and alpha are this iteration's draw (the stream-order argument: DESIGN.md section 24)
            newr.step(phase, clamp, rel.class_cut, a, lpd_new)
        if waic is not None:
            if waic_codes is not None:        # this draw's edges, ordered as for the test cells above
                ordinal.bounds(waic_pairs.ctx, waic_codes, waic_bounds)
            waic_pairs.waic_update(D, facs, rel.model.mean_value, a, phase, waic_bounds)
            if waic_codes is not None and waic_pairs.ctx is not eng.ctx:
                eng.ctx.stream.wait_stream(waic_pairs.ctx.stream)
        if i > burnin:
            if output:
                ndigits = int(math.floor(math.log10(psamples))) + 1
                nstr = str(i - burnin).rjust(ndigits, "0")
                for en in data.entities:
                    S = en.model.sample.astype(np.float32)
                    if output_type == "binary":
                        write_binary_matrix(f"{output}-{en.name}-{nstr}.binary", S)
                    else:
                        np.savetxt(f"{output}-{en.name}-{nstr}.csv", S, delimiter=",")
                    if output_beta and hasFeatures(en):
                        B = en.model.beta.astype(np.float32)
                        if output_type == "binary":
                            write_binary_matrix(f"{output}-{en.name}-{nstr}.beta.binary", B)
                        else:
                            np.savetxt(f"{output}-{en.name}-{nstr}.beta.csv", B, delimiter=",")
            if rmse_train:
                train.update(D, facs, rel.model.mean_value, phase, [], rel.class_cut)
            if i == burnin + 1 and verbose:
                print("--------- Burn-in complete, averaging posterior samples ----------")
            if callable(f):
                eng.sync()
                f_output.append(f(data))

        if verbose or i == burnin + psamples:
            if haveTest:
                # roc_avg = AUC_ROC(test_label, -probe_avg) (macau.jl:200) on the device, behind this iteration's prediction update
                # on the same stream; it lands beside the 4 stats (test.report), read back together after the one sync
                test.auc(rel.class_cut, eng.ctx_p)
            if newr is not None:
                newr.auc()                                    # behind the cells' update on the row stream, beside its 8 scalars
            wbar = eng.robust_mean() if (verbose and robust is not None) else None
            tbar = eng.entity_noise_mean() if (verbose and noise is not None) else None
            brms = eng.bias_rms() if (verbose and rel._dev.bias is not None) else None
            eng.sync()
            eng.sync_host_scalars()
            if haveTest:
                rep = test.report.cpu().numpy()
                s = rep[:4]
                n = numTest(rel)
                rmse_avg = math.sqrt(s[0] / n)
                err_avg = s[2] / n
                roc_avg = float(rep[4])
                if lpd:
                    lpd_avg = float(rep[6]) / n
            if waic is not None:
                waic_stats = waic_pairs.waic_stats.cpu().numpy()
            if newr is not None:
                new_rep = newr.report.cpu().numpy()
            if verbose:
                estr = " ".join(toStr(en) for en in data.entities)
                rstr = " ".join(toStr(r) for r in data.relations)
                lstr = f" LPD={lpd_avg:.4f}" if lpd else ""
                if waic is not None:
                    lstr += f" ELPD={(waic_stats[1] - waic_stats[2]) / max(waic_pairs.n, 1):.4f}"
                if wbar is not None:
                    lstr += f" w̄={float(wbar.item()):.3f}"
                if tbar is not None:
                    lstr += f" τ̄={float(tbar.item()):.3f}"
                if brms is not None:
                    lstr += "".join(f" b:{float(x.item()):.3f}" for x in brms)
                if newr is not None:
                    nsc = max(newr.n_scored, 1)
                    lstr += f" new:RMSE={math.sqrt(new_rep[0] / nsc):6.4f} ROC={new_rep[8]:6.4f}"
                    if lpd_new:
                        lstr += f" LPD={new_rep[5] / nsc:.4f}"
                if ordinal is not None:
                    lstr += " cut=[" + " ".join(f"{e:.3f}" for e in rel.model.ordinal_edges) + "]"
                print(f"{i:3d}: ROC={roc_avg:6.4f} RMSE={rmse_avg:6.4f}{lstr} | {estr} | {rstr} [{time.time() - time0:1.1f}s]")

    rec_dev = None
    if recommend is not None:
        # the lists and the ranking metrics from the device, behind the last draw on the row stream: n_rows x K items and scores and
        # four scalars are all that is read back
        K = recommend["k"]
        items, scores = eng.scores.topk(K, rel.model.mean_value, rel._dev if recommend["exclude_listed"] else None)
        rec_dev = (items, scores, eng.scores.metrics(items, K, test, rel.class_cut) if haveTest else None)
    acq_dev = None
    if acquire is not None:
        # the lists with the moments at their items, gathered on the device: n_rows x K values of each are all that is read back
        acq_dev = eng.acquire.topk(acquire["k"], acquire["rule"], acquire["kappa"], rel._dev if acquire["exclude_listed"] else None)
    eng.sync()
    eng.sync_host_scalars()
    result = {
        "num_latent": num_latent,
        "burnin": burnin,
        "psamples": psamples,
        "lambda_beta": data.entities[0].lambda_beta,
        "RMSE": rmse_avg,
        "accuracy": err_avg,
        "ROC": roc_avg,
    }
    if ordinal is not None:
        got = ordinal.read(burnin + psamples)
        tr = got["trace"]
        # a step was accepted iff it left other edges than it found (the row before; the start k + 1/2 before the first)
        before = np.vstack([np.arange(1, ordinal.K) + 0.5, tr[:-1]]) if len(tr) else tr
        moved = np.any(tr != before, axis=1)[burnin:]
        result["ordinal"] = {"edges": tr[burnin:].mean(axis=0) if psamples else np.full(ordinal.K - 1, np.nan),
                             "edges_trace": tr[burnin:].copy(), "accept": float(moved.mean()) if psamples else float("nan"),
                             "step": got["sigma"]}
    elif rel.model.ordinal is not None:                 # sample_edges = false: the edges are where they started
        e = np.arange(1, rel.model.ordinal["K"]) + 0.5
        result["ordinal"] = {"edges": e, "edges_trace": np.tile(e, (psamples, 1)), "accept": 0.0, "step": rel.model.ordinal["step"]}
    if robust is not None:
        # the posterior mean of every training row's omega, in the caller's order: the cells with a small one are the outliers
        ws = rel._dev.omega_sum
        result["robust"] = {"nu": robust["nu"],
                            "weights": (ws.cpu().numpy()[:rel.data.nnz()] / psamples) if (ws is not None and psamples) else np.full(rel.data.nnz(), np.nan)}
    if noise is not None:
        # the posterior mean of every row's tau, in the order of the entity's rows: the rows with a small one are the noisy ones
        ts, N = rel._dev.tau_sum, int(rel.data.dims[noise["mode"] - 1])
        result["noise"] = {"entity": rel.entities[noise["mode"] - 1].name, "shape": noise["shape"], "rate": noise["rate"],
                           "precision": (ts.cpu().numpy()[:N] / psamples) if (ts is not None and psamples) else np.full(N, np.nan)}
    if biased:
        # per relation and biased entity: the posterior mean bias of every row and the posterior mean of their precision
        result["bias"] = eng.bias_result(psamples)
    if spiked:
        # posterior means of pi_d, tau_d, the share of rows with a nonzero loading and [u_id != 0]
        result["spike"] = {en.name: st.spike_result() for en, st in zip(data.entities, eng.ent) if st.spike is not None}
    if nonneg:
        # posterior means of tau_d and of the rows (all >= 0)
        result["nonneg"] = {en.name: st.nonneg_result() for en, st in zip(data.entities, eng.ent) if st.nonneg is not None}
    if lpd:
        result["LPD"] = lpd_avg
    # relations with background cells (setBackground): what every unlisted cell observed, and how many there were
    bgs = {r.name: {"weight": r.model.background["weight"], "value": r.model.background["value"],
                    "cells": int(r.data.dims[0]) * int(r.data.dims[1]) - r.data.nnz()} for r in data.relations if r.model.background is not None}
    if bgs:
        result["background"] = bgs
    # dense relations (setDense): how many cells the matrix on the device holds, and how many of them were imputed
    dense = {r.name: {"cells": int(r.data.dims[0]) * int(r.data.dims[1]),
                      "holes": int(r.data.dims[0]) * int(r.data.dims[1]) - r.data.nnz()} for r in data.relations if r.model.dense}
    if dense:
        result["dense"] = dense
    if recommend is not None:
        rows = recommend["rows"]
        result["recommend"] = {"k": recommend["k"], "rows": np.arange(1, int(rel.data.dims[0]) + 1) if rows is None else np.array(rows, dtype=np.int64),
                               "items": rec_dev[0].cpu().numpy(), "scores": rec_dev[1].cpu().numpy()}
        if rec_dev[2] is not None:
            m = rec_dev[2].cpu().numpy()
            result["recommend"].update({"recall": float(m[0]), "ndcg": float(m[1]), "hit_rate": float(m[2]), "rows_scored": int(m[3])})
    if acquire is not None:
        rows = acquire["rows"]
        result["acquire"] = {"k": acquire["k"], "rule": acquire["rule"], "kappa": acquire["kappa"], "threshold": acquire["threshold"],
                             "rows": np.arange(1, int(rel.data.dims[0]) + 1) if rows is None else np.array(rows, dtype=np.int64)}
        result["acquire"].update({k: v.cpu().numpy() for k, v in acq_dev.items()})
    if newr is not None:
        # the cells' (pred, stdev, lpd) in the caller's order and the posterior mean of the new rows' factors: all that comes back
        import pandas as pd
        out, fac = newr.result()
        spec, nsc = rel.model.new_test, newr.n_scored
        frame = {rel.data.names[k]: spec["ids"][:, k] for k in range(2)}
        frame[rel.data.names[-1]] = spec["values"]
        frame["pred"], frame["stdev"] = out[:, 0], out[:, 1]
        if lpd_new:
            frame["lpd"] = out[:, 2]
        scored = nsc > 0 and psamples >= 1
        result["new_rows"] = {"entity": rel.entities[spec["mode"] - 1].name, "n_rows": newr.n_rows, "predictions": pd.DataFrame(frame),
                              "RMSE": math.sqrt(new_rep[0] / nsc) if scored else float("nan"), "ROC": float(new_rep[8]),
                              "accuracy": float(new_rep[2] / nsc) if scored else float("nan"), "n_scored": nsc, "factors": fac}
        if newr.foldin:
            # (the new rows were conditioned on known cells of their own, setNewObserved: `factors` is then the posterior mean of uhat_i)
            result["new_rows"]["n_known"] = newr.n_known
        if lpd_new:
            result["new_rows"]["LPD"] = float(new_rep[5] / nsc) if scored else float("nan")
    if waic is not None:
        # lppd, p_waic and the squares of elpd_t about its mean from the device (bdf_pairs_waic): the pointwise table comes to the
        # host only when asked for
        st, pw = waic_pairs.waic(pointwise=waic["pointwise"])
        n = waic_pairs.n
        result["WAIC"] = {"waic": float(-2.0 * (st[0] - st[1])), "elpd": float(st[0] - st[1]), "lppd": float(st[0]), "p_waic": float(st[1]),
                          "se": math.sqrt(float(st[2])), "n_high": int(st[3]), "n": n}
        if waic["pointwise"]:
            import pandas as pd
            ids = np.asarray(rel.data.ids).reshape(n, len(rel.entities))
            frame = {rel.data.names[k]: ids[:, k] for k in range(ids.shape[1])}
            frame["lppd"], frame["p_waic"] = pw[:, 0], pw[:, 1]
            result["WAIC"]["pointwise"] = pd.DataFrame(frame)
    if full_prediction:
        result["predictions_full"] = (yhat_full / psamples).cpu().numpy()        # macau.jl:228-230
    if rmse_train:
        tavg, _ = train.state()
        result["RMSE_train"] = float(np.sqrt(np.mean((rel.data.getValues() - makeClamped(tavg, clamp)) ** 2)))
    if haveTest:
        avg, sq = test.state()
        if psamples >= 3:
            tmp = (sq - avg ** 2 * psamples) / (psamples - 1)
            tmp[tmp < 0] = 0
            stdev = np.sqrt(tmp)
        else:
            stdev = np.full(len(avg), np.nan)
        extra = {"lpd": test.lpd() if psamples >= 1 else np.full(len(avg), np.nan)} if lpd else {}
        result["predictions"] = rel.test_vec.to_frame(pred=makeClamped(avg, clamp), stdev=stdev, **extra)
        import pandas as pd
        tc = np.zeros((numTest(rel), len(rel.entities)), dtype=np.int64)
        for mode in range(len(rel.entities)):
            rp = rel.data._rowptr[mode]
            ids = rel.test_vec.ids[:, mode].astype(np.int64)
            tc[:, mode] = rp[ids] - rp[ids - 1]
        result["train_counts"] = pd.DataFrame(tc, columns=[f"x{k + 1}" for k in range(tc.shape[1])])
    if callable(f):
        result["f_output"] = f_output
    result["latent_multi_threading"] = latent_multi_threading
    return result


# ---- prediction helpers of the reference (src/sampling.jl:9-97) on host copies of the factors --------------------
def pred(r, probe_vec=None, F=None):
    """pred(r) on the training table / pred(r, probe_vec) (sampling.jl:9-18) through the device kernel"""
    eng_rel = r._dev
    if eng_rel is None:
        raise ArgumentError("relation has no device state: run macau() first")
    from .engine import DevicePairs
    ctx = eng_rel.ctx
    ids = r.data.ids if probe_vec is None else np.asarray(getattr(probe_vec, "ids", probe_vec))[:, :len(r.entities)]
    pairs = DevicePairs(ctx, ids, np.zeros(len(ids)))
    facs = [e.model._dev.sample for e in r.entities]
    base = None
    if eng_rel.bias is not None and len(ids):
        # the current draw's biases: the pairs' base is mean + the cell's biases (bdf_bias_baseline)
        from ._lib import check, lib
        from .engine import bias_baseline
        base = bias_baseline(eng_rel, r.model.mean_value, pairs, ctx.zeros(len(ids)))
        check(lib().bdf_pairs_set_baseline(pairs.handle, base.data_ptr()))
    out = pairs.predict(facs[0].shape[1], facs, r.model.mean_value).cpu().numpy()
    pairs.close()
    return out


def pred_all(r):
    """pred_all(r) (sampling.jl:91-97): every cell of the relation, on host copies (test utility, not hot path)"""
    if hasFeatures(r):
        raise ArgumentError("Prediction of all elements is not possible when Relation has features.")
    S = [e.model.sample for e in r.entities]        # D x N_k
    if len(S) == 2:
        return S[0].T @ S[1] + r.model.mean_value
    letters = "abcdefg"[:len(S)]
    expr = ",".join(f"z{c}" for c in letters) + "->" + letters
    return np.einsum(expr, *S) + r.model.mean_value
