"""What macau() keeps of the posterior draws for each option, one object per summary: its running state,
its step per draw, its device scalars of the reporting step, its piece of the verbose line and its keys of `result`.  macau() builds
the list of the summaries that are on, in the order their work is enqueued in an iteration; the order of the verbose line's pieces
and of the keys of `result` are the two tuples at the end of this module.  A summary lives for one macau() call: an engine that is
reused has nothing to reset.

`run`, from macau(): eng, data, rel (the first relation), burnin, psamples, verbose, clamp, lpd (as asked), test (the test pairs or
None), test_report (their device scalars on the host, after the reporting sync), columns (what a summary's result() adds to the
columns of result["predictions"]).  `it`, one iteration: i, phase (0 burn-in, 1 the
first posterior draw, 2 later ones), facs (rel's factors), alpha (rel's precision for this draw: 1 for probit; a sampled one is the
device scalar of the native iteration, drawn on the row stream, and step by step the double the host has read from it).
"""
import math

import numpy as np
import torch

from ._lib import ArgumentError, check, lib
from .engine import DIAG_STATS, DeviceAcquire, DeviceDiag, DeviceScores, _ptr
from .relation_data import _ordinal_bounds, _waic_bounds, check_test_interval, hasFeatures


class RunningMean:
    """the posterior mean of a device tensor over the draws: the sum on the device, added to on ctx's stream (the row stream, behind
    the draw that wrote the tensor and ahead of the next one), and the count.  shape: the leading part of the tensor that the host
    array keeps"""

    def __init__(self, ctx, shape):
        self.ctx, self.shape, self.sum, self.count = ctx, tuple(int(s) for s in shape), None, 0

    def add(self, t):
        with torch.cuda.stream(self.ctx.stream):
            if self.sum is None:
                self.sum = t.clone()
            else:
                self.sum += t
        self.count += 1

    def mean(self, on_device=False):
        """the host array, NaN with no draws; on_device: divided as torch divides a device tensor by a number, sum * (1 / count)"""
        if not self.count:
            return np.full(self.shape, np.nan)
        s = self.sum / float(self.count) if on_device else self.sum
        return s.cpu().numpy()[tuple(slice(0, n) for n in self.shape)] / (1.0 if on_device else self.count)


class Summary:
    """the hooks, each a no-op: draw(it) every iteration behind the engine's step; report() on a reporting iteration before its one
    sync, to enqueue device scalars, and read() after it; line(), the piece of the verbose line; finish() before the final sync, to
    enqueue the end of the run's device work; result(result), to add its keys"""

    def __init__(self, run):
        self.run = run

    draw = report = read = finish = result = lambda self, *args: None

    def line(self):
        return ""


class FullPrediction(Summary):
    """full_prediction = true (macau.jl:145-147, 228-230): the mean of pred_all, a plain dense product on the device"""

    def __init__(self, run):
        super().__init__(run)
        if hasFeatures(run.rel):
            raise ArgumentError("Prediction of all elements is not possible when Relation has features.")   # sampling.jl:92-94
        self.mean = RunningMean(run.eng.ctx, run.rel.data.dims)

    def draw(self, it):
        if it.phase:
            self.mean.add(self.run.eng.pred_all(self.run.rel))

    def result(self, result):
        m = self.mean.mean(on_device=True)
        result["predictions_full"] = m if self.mean.count else np.copysign(m, -1.0)      # (no draws: the NaN of 0 * (1 / 0) on the device)


def _scored_rows(rel, spec):
    """(how many rows of the first entity a list is kept for, their 0-based rows of U or None for all, their 1-based ids)"""
    rows, N = spec["rows"], int(rel.data.dims[0])
    if rows is None:
        return N, None, np.arange(1, N + 1)
    return len(rows), np.asarray(rows, dtype=np.int64) - 1, np.array(rows, dtype=np.int64)


class Recommend(Summary):
    """top-K lists of the first relation (setRecommend) from the sum of u.v over the draws: every draw's factors
    go into the ring on the row stream (a full ring: one accumulate launch); the lists and the ranking metrics come from the device
    behind the last draw on that stream: n_rows x K items and scores and four scalars are all that is read back"""

    def __init__(self, run):
        super().__init__(run)
        rel, self.spec = run.rel, run.rel.model.recommend
        n, rows0, self.rows = _scored_rows(rel, self.spec)
        self.dev = DeviceScores(run.eng.ctx, n, int(rel.data.dims[1]), run.eng.D, self.spec["batch"], rows0)

    def draw(self, it):
        if it.phase:
            self.dev.push(it.facs[0], it.facs[1])

    def finish(self):
        run, K = self.run, self.spec["k"]
        self.items, self.scores = self.dev.topk(K, run.rel.model.mean_value, run.rel._dev if self.spec["exclude_listed"] else None)
        self.metrics = self.dev.metrics(self.items, K, run.test, run.rel.class_cut) if run.test is not None else None

    def result(self, result):
        result["recommend"] = {"k": self.spec["k"], "rows": self.rows, "items": self.items.cpu().numpy(), "scores": self.scores.cpu().numpy()}
        if self.metrics is not None:
            m = self.metrics.cpu().numpy()
            result["recommend"].update({"recall": float(m[0]), "ndcg": float(m[1]), "hit_rate": float(m[2]), "rows_scored": int(m[3])})
        self.dev.close()


class Acquire(Summary):
    """acquisition lists of the first relation (setAcquire): the moment planes of u.v over the draws for the
    scored rows.  Every draw's factors and its precision go into the ring on the row stream; the lists with the moments at their
    items are gathered on the device: n_rows x K values of each are all that is read back"""

    def __init__(self, run):
        super().__init__(run)
        rel, self.spec = run.rel, run.rel.model.acquire
        n, rows0, self.rows = _scored_rows(rel, self.spec)
        self.dev = DeviceAcquire(run.eng.ctx, n, int(rel.data.dims[1]), run.eng.D, self.spec["batch"], rows0, rel.model.mean_value,
                                 self.spec["threshold"])

    def draw(self, it):
        if it.phase:
            self.dev.push(it.facs[0], it.facs[1], it.alpha)

    def finish(self):
        s = self.spec
        self.lists = self.dev.topk(s["k"], s["rule"], s["kappa"], self.run.rel._dev if s["exclude_listed"] else None)

    def result(self, result):
        s = self.spec
        result["acquire"] = {"k": s["k"], "rule": s["rule"], "kappa": s["kappa"], "threshold": s["threshold"], "rows": self.rows}
        result["acquire"].update({k: v.cpu().numpy() for k, v in self.lists.items()})
        self.dev.close()


class _DrawMean(Summary):
    """the posterior mean of a tensor that the first relation's model draws before the rows of every iteration, and the mean over
    its entries of this iteration's draw in the verbose line, a device scalar read with the others"""

    def __init__(self, run, tensor, n):
        super().__init__(run)
        self.tensor, self.mean, self.now = tensor, RunningMean(run.eng.ctx, (n,)), None

    def draw(self, it):
        if it.phase:
            self.mean.add(self.tensor)

    def report(self):
        if self.run.verbose:
            with torch.cuda.stream(self.run.eng.ctx.stream):
                self.now = self.tensor.mean()

    def line(self):
        return f" {self.mark}={float(self.now.item()):.3f}"


class Robust(_DrawMean):
    """the robust noise model (setRobust): the posterior mean of every training row's omega, in the caller's
    order -- the cells with a small one are the outliers"""
    mark = "w̄"

    def __init__(self, run):
        super().__init__(run, run.rel._dev.omega, run.rel.data.nnz())

    def result(self, result):
        result["robust"] = {"nu": self.run.rel.model.robust["nu"], "weights": self.mean.mean()}


class EntityNoise(_DrawMean):
    """a noise precision per row of one entity (setEntityNoise): the posterior mean of every row's tau, in the
    order of the entity's rows -- the rows with a small one are the noisy ones"""
    mark = "τ̄"

    def __init__(self, run):
        self.spec = run.rel.model.entity_noise
        super().__init__(run, run.rel._dev.tau, run.rel.data.dims[self.spec["mode"] - 1])

    def result(self, result):
        s = self.spec
        result["noise"] = {"entity": self.run.rel.entities[s["mode"] - 1].name, "shape": s["shape"], "rate": s["rate"], "precision": self.mean.mean()}


class Bias(Summary):
    """biases (setBias), sampled on any relation: per relation and biased entity the posterior mean bias of
    every row and the posterior mean of their precision; the verbose line shows the rms of the first relation's"""

    def __init__(self, run):
        super().__init__(run)
        ctx = run.eng.ctx
        self.sums = [(r, dr, {m0: RunningMean(ctx, (r.data.dims[m0],)) for m0 in dr.bias}, RunningMean(ctx, (len(dr.bias),)))
                     for r, dr in zip(run.data.relations, run.eng.rel) if dr.bias is not None]
        self.rms = None

    def draw(self, it):
        if it.phase:
            for r, dr, rows, lam in self.sums:
                for m0, b in dr.bias.items():
                    rows[m0].add(b)
                lam.add(dr.bias_lambda)

    def report(self):
        run = self.run
        if run.verbose and run.rel._dev.bias is not None:
            with torch.cuda.stream(run.eng.ctx.stream):
                self.rms = [b[:int(run.rel.data.dims[m0])].square().mean().sqrt() for m0, b in run.rel._dev.bias.items()]

    def line(self):
        return "".join(f" b:{float(x.item()):.3f}" for x in self.rms) if self.rms is not None else ""

    def result(self, result):
        result["bias"] = {}
        for r, dr, rows, lam in self.sums:
            lm = lam.mean()
            result["bias"][r.name] = {r.entities[m0].name: {"mean": rows[m0].mean(), "precision": float(lm[t])} for t, m0 in enumerate(dr.bias_spec)}


class _PriorSums(Summary):
    """entities with a prior of their own (`key`) whose result a library kernel (`fn`) sums over the draws: per loading (N x D) and
    per component (`hyper` x D doubles), zeroed on the row stream, which is the one that adds to them (DESIGN.md section 8:
    hipMemset) once this iteration's hyper step (the hyperprior stream) has written the prior's state (`state`)"""
    key, state, fn, hyper = None, None, None, 1

    def __init__(self, run):
        super().__init__(run)
        self.sums = [(en, st, run.eng.ctx.zeros(st.N, st.D), run.eng.ctx.zeros(self.hyper * st.D))
                     for en, st in zip(run.data.entities, run.eng.ent) if getattr(st, self.key) is not None]
        self.draws = 0

    def draw(self, it):
        eng = self.run.eng
        if it.phase:
            if eng.ctx_h is not eng.ctx:
                eng.ctx.stream.wait_stream(eng.ctx_h.stream)
            for en, st, rows, hyper in self.sums:
                check(getattr(lib(), self.fn)(st.ctx.handle, st.D, st.n_real, _ptr(st.sample), _ptr(getattr(st, self.state)), _ptr(rows), _ptr(hyper)))
            self.draws += 1

    def result(self, result):
        torch.cuda.synchronize(self.run.eng.ctx.device)
        result[self.key] = {}
        for en, st, rows, hyper in self.sums:
            h, rows = hyper.cpu().numpy(), rows.cpu().numpy()[:st.n_real]
            if not self.draws:
                h, rows = np.full(len(h), np.nan), np.full(rows.shape, np.nan)
            result[self.key][en.name] = self.means(h, rows, max(self.draws, 1), st)


class Spike(_PriorSums):
    """the spike-and-slab prior (setSpikeAndSlab): this draw's inclusions, pi, tau and counts; the posterior
    means of pi_d, tau_d, the share of rows with a nonzero loading and [u_id != 0]"""
    key, state, fn, hyper = "spike", "spike_state", "bdf_spike_accumulate", 3

    @staticmethod
    def means(h, rows, n, st):
        D = st.D
        return {"inclusion": h[:D] / n, "precision": h[D:2 * D] / n, "activity": h[2 * D:] / (n * float(st.n_real)), "row_inclusion": rows / n}


class NonNeg(_PriorSums):
    """the non-negative prior (setNonNegative): this draw's rows and tau; the posterior means of tau_d and of
    the rows (all >= 0)"""
    key, state, fn = "nonneg", "nonneg_tau", "bdf_nonneg_accumulate"

    @staticmethod
    def means(h, rows, n, st):
        return {"precision": h / n, "factors": rows / n}


class Lpd(Summary):
    """held-out log predictive density of the test cells (lpd = true): what kind of record every test cell
    is -- a 0/1 value of a probit relation, an interval (setTestInterval / setTestBinned), a level of an ordinal relation
    (setTestOrdinal) or a measurement.  Step by step the pairs have a stream of their own: the next iteration's step may not publish
    its edges -- or redraw the tau that the cells are scored with -- under this draw's launch, so the row stream waits for it; the
    native iteration scores on the row stream itself and needs nothing"""

    def __init__(self, run):
        super().__init__(run)
        rel, test = run.rel, run.test
        self.bounds, self.codes, self.avg = None, None, float("nan")
        if rel.model.test_interval is not None:
            check_test_interval(rel)
            self.bounds = test.ctx.tensor(rel.model.test_interval)
        elif rel.model.test_ordinal is not None:
            # the levels' bins between the fixed edges, once; between sampled edges they follow every draw
            self.bounds = test.ctx.tensor(_ordinal_bounds(rel.model.test_ordinal, np.arange(1, rel.model.ordinal["K"]) + 0.5))
            if rel._dev.ordinal is not None:
                self.codes = test.ctx.tensor(rel.model.test_ordinal, dtype=torch.int8)
        self.wait = (self.codes is not None or rel.model.entity_noise is not None) and test.ctx is not run.eng.ctx

    def draw(self, it):
        run, test = self.run, self.run.test
        if self.codes is not None:
            # this draw's edges were published on the row stream before this iteration's rows, which the pairs' stream is behind
            run.rel._dev.ordinal.bounds(test.ctx, self.codes, self.bounds)
        test.lpd_update(run.eng.D, it.facs, run.rel.model.mean_value, it.alpha, it.phase, self.bounds)
        if self.wait:
            run.eng.ctx.stream.wait_stream(test.ctx.stream)

    def read(self):
        self.avg = float(self.run.test_report[6]) / self.run.test.n

    def line(self):
        return f" LPD={self.avg:.4f}"

    def result(self, result):
        result["LPD"] = self.avg


class Diagnostics(Summary):
    """convergence diagnostics of the test cells' predictions (setDiagnostics on the first relation): every
    posterior draw of the predictions, of the draw's sum of squared test errors and of a sampled alpha goes into one plane on the
    device, a second gather of the test pairs beside the prediction update's; the split R-hat, effective sample size and Monte Carlo
    standard error of every series come from the device at the end of the run: 6 + 3 per scalar doubles are read back, and three
    columns when asked for.  The push runs on the pairs' stream, where Lpd scores.  The native iteration's is the row stream: behind
    this iteration's rows, its biases' base and its alpha, ahead of the next ones in order.  Step by step it is the prediction
    stream, which is behind this iteration's rows; the next iteration's rows cannot overwrite the factors under the push, because an
    entity's three sample buffers rotate -- the buffer of draw t is next written by the rows of iteration t + 3 -- and those rows
    wait for the hyperprior stream, which at the start of iteration t + 2 has waited for all that the prediction stream held when
    iteration t + 1 began, this push included (GibbsEngine.sweep: the same argument as for the prediction update).  A base that the row stream rewrites (biases, relation features) keeps the pairs on the row stream, and
    alpha is then the double the host has read"""

    def __init__(self, run):
        super().__init__(run)
        rel, test = run.rel, run.test
        self.spec = rel.model.diagnostics
        self.names = ("sse", "alpha") if rel.model.alpha_sample else ("sse",)
        self.dev = DeviceDiag(test.ctx, test.n, len(self.names), run.psamples)

    def draw(self, it):
        if it.phase:
            run = self.run
            self.dev.push(run.test, run.eng.D, it.facs, run.rel.model.mean_value, it.alpha)

    def finish(self):
        s = self.spec
        self.stats, self.out = self.dev.compute(s["rhat_cut"], s["ess_cut"], s["pointwise"], self.run.test._order)

    def result(self, result):
        st, s, n = self.stats.cpu().numpy(), self.spec, len(DIAG_STATS)
        d = {k: (float(v) if k in ("max_rhat", "min_ess") else int(v)) for k, v in zip(DIAG_STATS, st)}
        d = {"n_draws": d.pop("n_draws"), **d, "rhat_cut": s["rhat_cut"], "ess_cut": s["ess_cut"],
             "scalars": {name: dict(zip(("rhat", "ess", "mcse"), (float(x) for x in st[n + 3 * k:n + 3 * k + 3]))) for k, name in enumerate(self.names)}}
        result["diagnostics"] = d
        if self.out is not None:
            cols = self.out.cpu().numpy()
            self.run.columns.update(rhat=cols[:, 0].copy(), ess=cols[:, 1].copy(), mcse=cols[:, 2].copy())
        if self.run.verbose:
            print(f"Diagnostics: max R̂={d['max_rhat']:.4f} min ESS={d['min_ess']:.1f} ({d['n_rhat_high']} of {self.dev.n_cells} cells above {s['rhat_cut']:g})")
        self.dev.close()


class Waic(Summary):
    """WAIC on the training cells (setWaic on the first relation): what kind of record every training row is
    (the table of section 17) is built once on the host; between sampled edges the levels' bins follow every draw, from the levels
    the sampler itself keeps on the device, ordered as for the test cells (Lpd).  lppd, p_waic and the squares of elpd_t about its
    mean come from the device (bdf_pairs_waic): the pointwise table comes to the host only when asked for"""

    def __init__(self, run):
        super().__init__(run)
        rel, self.spec = run.rel, run.rel.model.waic
        self.pairs = run.eng.train_pairs()
        b = _waic_bounds(rel)
        self.bounds = self.pairs.ctx.tensor(b) if b is not None else None
        self.codes = rel._dev.ord_codes if rel._dev.ordinal is not None else None
        self.stats = np.full(4, np.nan)

    def draw(self, it):
        run, pairs = self.run, self.pairs
        if self.codes is not None:
            run.rel._dev.ordinal.bounds(pairs.ctx, self.codes, self.bounds)
        pairs.waic_update(run.eng.D, it.facs, run.rel.model.mean_value, it.alpha, it.phase, self.bounds)
        if self.codes is not None and pairs.ctx is not run.eng.ctx:
            run.eng.ctx.stream.wait_stream(pairs.ctx.stream)

    def read(self):
        self.stats = self.pairs.waic_stats.cpu().numpy()

    def line(self):
        return f" ELPD={(self.stats[1] - self.stats[2]) / max(self.pairs.n, 1):.4f}"

    def result(self, result):
        import pandas as pd
        rel, n = self.run.rel, self.pairs.n
        st, pw = self.pairs.waic(pointwise=self.spec["pointwise"])
        result["WAIC"] = {"waic": float(-2.0 * (st[0] - st[1])), "elpd": float(st[0] - st[1]), "lppd": float(st[0]), "p_waic": float(st[1]),
                          "se": math.sqrt(float(st[2])), "n_high": int(st[3]), "n": n}
        if self.spec["pointwise"]:
            ids = np.asarray(rel.data.ids).reshape(n, len(rel.entities))
            frame = {rel.data.names[k]: ids[:, k] for k in range(ids.shape[1])}
            frame["lppd"], frame["p_waic"] = pw[:, 0], pw[:, 1]
            result["WAIC"]["pointwise"] = pd.DataFrame(frame)


class NewRows(Summary):
    """cells of rows that were not in training (setNewRows / setNewTest on the first relation), with
    setNewObserved conditioned on known cells of their own (section 29).  uhat of the new rows, q of the other entity's rows and the
    cells' update run on the row stream behind this iteration's last launch: beta, V, (mu, Lambda) and alpha are this iteration's
    draw (section 24).  The cells' (pred, stdev, lpd) and the posterior mean of the new rows' factors are all that comes back"""

    def __init__(self, run):
        super().__init__(run)
        self.dev = run.eng.new_rows(fresh=True)
        self.factors = RunningMean(run.eng.ctx, (self.dev.n_rows, run.eng.D))
        self.rep = np.full(10, np.nan)

    def draw(self, it):
        run = self.run
        factors = self.dev.step(it.phase, run.clamp, run.rel.class_cut, it.alpha, run.lpd)
        if it.phase:
            self.factors.add(factors)

    def report(self):
        self.dev.auc()                                    # behind the cells' update on the row stream, beside its 8 scalars

    def read(self):
        self.rep = self.dev.report.cpu().numpy()

    def line(self):
        nsc = max(self.dev.n_scored, 1)
        s = f" new:RMSE={math.sqrt(self.rep[0] / nsc):6.4f} ROC={self.rep[8]:6.4f}"
        return s + (f" LPD={self.rep[5] / nsc:.4f}" if self.run.lpd else "")

    def result(self, result):
        import pandas as pd
        run, rel, dev, rep = self.run, self.run.rel, self.dev, self.rep
        out = dev.result()
        spec, nsc = rel.model.new_test, dev.n_scored
        frame = {rel.data.names[k]: spec["ids"][:, k] for k in range(2)}
        frame[rel.data.names[-1]] = spec["values"]
        frame["pred"], frame["stdev"] = out[:, 0], out[:, 1]
        if run.lpd:
            frame["lpd"] = out[:, 2]
        scored = nsc > 0 and run.psamples >= 1
        result["new_rows"] = {"entity": rel.entities[spec["mode"] - 1].name, "n_rows": dev.n_rows, "predictions": pd.DataFrame(frame),
                              "RMSE": math.sqrt(rep[0] / nsc) if scored else float("nan"), "ROC": float(rep[8]),
                              "accuracy": float(rep[2] / nsc) if scored else float("nan"), "n_scored": nsc, "factors": self.factors.mean(on_device=True)}
        if dev.foldin:
            # (the new rows were conditioned on known cells of their own, setNewObserved: `factors` is then the posterior mean of uhat_i)
            result["new_rows"]["n_known"] = dev.n_known
        if run.lpd:
            result["new_rows"]["LPD"] = float(rep[5] / nsc) if scored else float("nan")


class Ordinal(Summary):
    """an ordinal first relation (setOrdinal).  Sampled edges: a trace row per iteration, the step size
    adapted in the burn-in; a step was accepted iff it left other edges than it found.  sample_edges = false: the edges are where
    they started"""

    def __init__(self, run):
        super().__init__(run)
        self.dev = run.eng.ordinal_begin(run.burnin, run.psamples)

    def line(self):
        return " cut=[" + " ".join(f"{e:.3f}" for e in self.run.rel.model.ordinal_edges) + "]" if self.dev is not None else ""

    def result(self, result):
        spec, burnin, psamples = self.run.rel.model.ordinal, self.run.burnin, self.run.psamples
        e = np.arange(1, spec["K"]) + 0.5
        if self.dev is None:
            result["ordinal"] = {"edges": e, "edges_trace": np.tile(e, (psamples, 1)), "accept": 0.0, "step": spec["step"]}
            return
        got = self.dev.read(burnin + psamples)
        tr = got["trace"]
        before = np.vstack([e, tr[:-1]]) if len(tr) else tr          # (the row before; the start k + 1/2 before the first)
        moved = np.any(tr != before, axis=1)[burnin:]
        result["ordinal"] = {"edges": tr[burnin:].mean(axis=0) if psamples else np.full(len(e), np.nan),
                             "edges_trace": tr[burnin:].copy(), "accept": float(moved.mean()) if psamples else float("nan"),
                             "step": got["sigma"]}


class WholeMatrix(Summary):
    """relations with background cells (setBackground): what every unlisted cell observed, and how many there
    were; dense relations (setDense; section 25): how many cells the matrix on the device holds, and how many of them were imputed"""

    def result(self, result):
        rels = [(r, int(r.data.dims[0]) * int(r.data.dims[1])) for r in self.run.data.relations]
        bgs = {r.name: {"weight": r.model.background["weight"], "value": r.model.background["value"], "cells": n - r.data.nnz()}
               for r, n in rels if r.model.background is not None}
        dense = {r.name: {"cells": n, "holes": n - r.data.nnz()} for r, n in rels if r.model.dense}
        result.update({k: v for k, v in (("background", bgs), ("dense", dense)) if v})


# the pieces of the verbose line and the keys of `result`, in their order (the list in macau() is in the order of an iteration's work)
LINE_ORDER = (Lpd, Waic, Robust, EntityNoise, Bias, NewRows, Ordinal)
RESULT_ORDER = (Ordinal, Robust, EntityNoise, Bias, Spike, NonNeg, Lpd, Diagnostics, WholeMatrix, Recommend, Acquire, NewRows, Waic, FullPrediction)
