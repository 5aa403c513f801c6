"""macau() -- the Gibbs driver of the reference (src/macau.jl:3-255) over the device engine.

Same keyword surface and result keys as the reference.  Worker-process arguments (latent_pids, latent_blas_threads,
cg_pids) are accepted for drop-in compatibility; the GPU replaces the worker pool, so they only decide the
"latent_multi_threading" flag the reference reports (macau.jl:44-66, 253).  Extra keywords: seed, device.
"""
import math
import sys
import time
from types import SimpleNamespace

import numpy as np

from . import features as feat
from . import summaries as sm
from ._lib import ArgumentError
from .engine import GibbsEngine
from .model_options import refuse
from .relation_data import check_new_rows, hasFeatures, numTest, toStr


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
    # what the first relation's options rule out for this run (model_options.py)
    for key, asked in (("full_prediction", full_prediction), ("rmse_train", rmse_train), ("lpd", lpd)):
        if asked and data.relations:
            refuse(data.relations[0], key)
    # cells of rows that were not in training (setNewRows / setNewTest on the first relation), with
    # setNewObserved conditioned on known cells of their own (section 29)
    new_rel = check_new_rows(data)
    if lpd and not (data.relations and numTest(data.relations[0]) > 0) and new_rel is None:
        raise ArgumentError("lpd = true scores held-out cells: the first relation has no test cells (assignToTest / setTest).")
    # top-K and acquisition lists (setRecommend, setAcquire; DESIGN.md sections 21, 30) are kept for the first relation, like lpd and WAIC
    for field, lists, keeps in (("recommend", "top-k lists (setRecommend)", "sum"), ("acquire", "acquisition lists (setAcquire)", "moments")):
        for r in data.relations[1:]:
            if getattr(r.model, field) is not None:
                raise ArgumentError(f"Relation {r.name} asks for {lists} but is not the first relation: macau() keeps the {keeps} of scores for the first relation only.")
    # convergence diagnostics (setDiagnostics) are kept for the first relation's test cells
    for r in data.relations[1:]:
        if r.model.diagnostics is not None:
            raise ArgumentError(f"Relation {r.name} asks for convergence diagnostics (setDiagnostics) but is not the first relation: macau() keeps the draws of the first relation's test cells only.")
    diag = data.relations[0].model.diagnostics if data.relations else None
    if diag is not None and numTest(data.relations[0]) == 0:
        raise ArgumentError("Convergence diagnostics (setDiagnostics) are those of held-out predictions: the first relation has no test cells (assignToTest / setTest).")
    if diag is not None and psamples < 4:
        raise ArgumentError("Convergence diagnostics (setDiagnostics) split the posterior draws into two chains of at least two: psamples must be at least 4.")
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
    if diag is not None and eng.world > 1:
        raise ArgumentError("Convergence diagnostics (setDiagnostics) are not possible with more than one rank: every rank holds the draws of the test cells it predicts only.")
    if waic is not None and eng.world > 1:
        raise ArgumentError("WAIC (setWaic) is not possible with more than one rank: every rank holds the state of its own cells only.")
    if new_rel is not None:
        check_new_rows(data, eng.world)
    data._engine = eng

    latent_multi_threading = (len(latent_pids) >= 1 and len(data.relations) == 1 and not hasFeatures(data.relations[0]))
    if verbose:
        if latent_multi_threading:
            print("Sampling of latent vectors: all rows of an entity in one GPU launch.")
        else:
            print("Sampling of latent vectors: general (multi-relation) GPU path.")

    rel, rm = data.relations[0], data.relations[0].model
    haveTest = numTest(rel) > 0
    test = eng.test_pairs() if haveTest else None
    train = eng.train_pairs() if rmse_train else None
    # the options' posterior summaries (summaries.py), in the order their work is enqueued in an iteration: the
    # registration of an option's summary is its line here.  (Nothing is allocated or launched for an option that is off)
    run = SimpleNamespace(eng=eng, data=data, rel=rel, burnin=burnin, psamples=psamples, verbose=verbose, clamp=clamp, lpd=lpd,
                          test=test, test_report=None, columns={})
    summaries = [cls(run) for cls, on in (
        (sm.FullPrediction, full_prediction),
        (sm.Recommend, rm.recommend is not None),
        (sm.Acquire, rm.acquire is not None),
        (sm.Robust, rm.robust is not None),
        (sm.EntityNoise, rm.entity_noise is not None),
        (sm.Bias, any(dr.bias is not None for dr in eng.rel)),
        (sm.Spike, any(st.spike is not None for st in eng.ent)),
        (sm.NonNeg, any(st.nonneg is not None for st in eng.ent)),
        (sm.Lpd, lpd and haveTest),
        (sm.Diagnostics, diag is not None),
        (sm.NewRows, new_rel is not None),
        (sm.Waic, waic is not None),
        (sm.Ordinal, rm.ordinal is not None),
        (sm.WholeMatrix, any(r.model.background is not None or r.model.dense for r in data.relations))) if on]
    in_line, in_result = ([s for cls in order for s in summaries if type(s) is cls] for order in (sm.LINE_ORDER, sm.RESULT_ORDER))
    lpd = lpd and haveTest
    f_output = []
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
        if summaries:
            it = SimpleNamespace(i=i, phase=phase, facs=facs,
                                 alpha=1.0 if rm.probit else (rel._dev.alpha_dev if (rm.alpha_sample and eng.native) else rm.alpha))
            for s in summaries:
                s.draw(it)
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
                train.update(eng.D, facs, rm.mean_value, phase, [], rel.class_cut)
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
            for s in summaries:
                s.report()
            eng.sync()
            eng.sync_host_scalars()
            if haveTest:
                rep = run.test_report = test.report.cpu().numpy()
                n = numTest(rel)
                rmse_avg = math.sqrt(rep[0] / n)
                err_avg = rep[2] / n
                roc_avg = float(rep[4])
            for s in summaries:
                s.read()
            if verbose:
                estr = " ".join(toStr(en) for en in data.entities)
                rstr = " ".join(toStr(r) for r in data.relations)
                lstr = "".join(s.line() for s in in_line)
                print(f"{i:3d}: ROC={roc_avg:6.4f} RMSE={rmse_avg:6.4f}{lstr} | {estr} | {rstr} [{time.time() - time0:1.1f}s]")

    for s in summaries:
        s.finish()
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
    for s in in_result:
        s.result(result)
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
        result["predictions"] = rel.test_vec.to_frame(pred=makeClamped(avg, clamp), stdev=stdev, **extra, **run.columns)
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
