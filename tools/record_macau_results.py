#!/usr/bin/env python3
"""What macau() returns and prints with each option's posterior summary on, recorded from the package itself (needs a GPU).

    python tools/record_macau_results.py              writes tests/golden/macau_summaries.json
    python tools/record_macau_results.py --out FILE   writes FILE instead
    python tools/record_macau_results.py --against A  compares with recording A: a case that differs goes under "unstable"
    python tools/record_macau_results.py --detail     keeps every leaf's own hash and every line (with --out: to find what differs)

A case builds a fresh seeded model -- two entities of 24 and 18 rows, 200 listed cells (240 under setDense, which takes a relation
with half of its cells listed) with the values 1 .. 5 and 40 test cells, num_latent = 4 --, sets its options and runs
macau(burnin=2, psamples=5, verbose=True) once on the native iteration and once step by step (BDF_NO_NATIVE).
Recorded per case and path: the keys of `result` in order, a SHA-256 over the leaves of `result` (arrays and the columns of frames
by their bytes, floats by float.hex()), a SHA-256 over the verbose lines without their "[...s]" suffix and the last of them as text,
or the message of the error macau() raised.  A path that gives what the native one gives is written as "native".  tests/test_gpu_macau_summaries.py replays the file on the working tree: record it on the commit whose
behaviour is to be kept, twice -- the second time with --against the first.
"""
import contextlib
import hashlib
import io
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "macau_summaries.json")

N1, N2, N3, D = 24, 18, 10, 4
RUN = {"burnin": 2, "psamples": 5}
PATHS = ("native", "step")


class Model:
    """the fixture: relation `ratings` (users x items) with its test cells; `extra` adds a second relation users x genres"""

    def __init__(self, B, item_features=False, test=True, extra=False, listed=200):
        rng = np.random.default_rng(1)
        cells = rng.permutation(N1 * N2)[:listed + 40]
        ids = np.stack([cells // N2 + 1, cells % N2 + 1], axis=1).astype(np.int64)
        U, V = rng.standard_normal((N1, 2)), rng.standard_normal((N2, 2))
        raw = np.sum(U[ids[:, 0] - 1] * V[ids[:, 1] - 1], axis=1) + 0.3 * rng.standard_normal(len(ids))
        vals = np.clip(np.round(3.0 + 1.2 * raw), 1, 5)
        self.users = B.Entity("users")
        self.items = B.Entity("items", F=rng.standard_normal((N2, 3))) if item_features else B.Entity("items")
        self.rel = B.Relation((ids[:listed], vals[:listed]), "ratings", [self.users, self.items], class_cut=3.0, dims=[N1, N2])
        if test:
            B.setTest(self.rel, (ids[listed:], vals[listed:]))
        rels = [self.rel]
        if extra:
            self.genres = B.Entity("genres")
            c2 = rng.permutation(N1 * N3)[:90]
            ids2 = np.stack([c2 // N3 + 1, c2 % N3 + 1], axis=1).astype(np.int64)
            self.rel2 = B.Relation((ids2, rng.standard_normal(len(ids2))), "tastes", [self.users, self.genres], dims=[N1, N3])
            rels.append(self.rel2)
        self.data = B.RelationData(*rels) if len(rels) == 1 else _relation_data(B, rels)
        self.rng = rng


def _relation_data(B, rels):
    d = B.RelationData(rels[0])
    for r in rels[1:]:
        B.addRelation(d, r)
    return d


def _new_cells(m, n_new=3):
    """cells of n_new new rows of `items` against existing users: (test table, known table)"""
    rng = np.random.default_rng(2)
    c = rng.permutation(N1 * n_new)[:30]
    ids = np.stack([c % N1 + 1, c // N1 + 1], axis=1).astype(np.int64)
    vals = np.clip(np.round(3.0 + rng.standard_normal(len(ids))), 1, 5)
    vals[3] = np.nan
    return (ids[:18], vals[:18]), (ids[18:], np.nan_to_num(vals[18:], nan=3.0))


def _new_rows(B, m, observed):
    B.setNewRows(m.items, np.random.default_rng(3).standard_normal((3, 3)))
    test, known = _new_cells(m)
    if observed:
        B.setNewObserved(m.rel, m.items, known)
    B.setNewTest(m.rel, m.items, test)


def _new_rows_no_features(B, m):
    test, known = _new_cells(m)
    B.setNewObserved(m.rel, m.items, known, n_rows=3)
    B.setNewTest(m.rel, m.items, test)


def _ordinal(B, m, sample_edges, test=True):
    B.setOrdinal(m.rel, 5, sample_edges=sample_edges)
    if test:
        B.setTestOrdinal(m.rel)


def _alpha_sample(B, m):
    m.rel.model.alpha_sample = True


# what sets a summary's option on a Model, by the key model_options.py knows it by: (model keywords, setter, macau() keywords)
SUMMARIES = {
    "lpd": ({}, lambda B, m: None, {"lpd": True}),
    "waic": ({}, lambda B, m: B.setWaic(m.rel, pointwise=True), {}),
    "recommend": ({}, lambda B, m: B.setRecommend(m.rel, 3, batch=2), {}),
    "acquire": ({}, lambda B, m: B.setAcquire(m.rel, 3, batch=2), {}),
    "robust": ({}, lambda B, m: B.setRobust(m.rel), {}),
    "entity_noise": ({}, lambda B, m: B.setEntityNoise(m.rel, m.items), {}),
    "bias": ({}, lambda B, m: (B.setBias(m.rel, m.users), B.setBias(m.rel, m.items)), {}),
    "spike": ({}, lambda B, m: B.setSpikeAndSlab(m.users), {}),
    "nonneg": ({}, lambda B, m: B.setNonNegative(m.users), {}),
    "new_test": ({"item_features": True}, lambda B, m: _new_rows(B, m, False), {}),
    "ordinal": ({}, lambda B, m: _ordinal(B, m, True, test=False), {}),
    "full_prediction": ({}, lambda B, m: None, {"full_prediction": True}),
    "background": ({}, lambda B, m: B.setBackground(m.rel, 0.1, 2.0), {}),
    "dense": ({"listed": 240}, lambda B, m: B.setDense(m.rel), {}),
}
# the further options a key brings with it, for the table
_WITH = {"new_test": ("new_rows", "entity_features")}


def compatible(order):
    """the summaries of `order` that go together by model_options.refused, taken greedily"""
    from bdf_amd.model_options import refused
    on = []
    for key in order:
        keys = (key,) + _WITH.get(key, ())
        if not any(refused(a, b)[0] for have in on for a in (have,) + _WITH.get(have, ()) for b in keys):
            on.append(key)
    return on


def _case(*keys, model=None, run=None, second=False, extra_set=()):
    return {"keys": list(keys), "model": dict(model or {}), "run": dict(run or {}), "second": second, "extra_set": tuple(extra_set)}


def cases():
    out = {"plain": _case()}
    for key in SUMMARIES:
        out[key] = _case(key)
        if key != "waic":                          # (WAIC refuses psamples < 2)
            out[key + "_no_draws"] = _case(key, run={"psamples": 0})
    out["all_forward"] = _case(*compatible(list(SUMMARIES)))
    out["all_reverse"] = _case(*compatible(list(SUMMARIES)[::-1]))
    out["all_forward_quiet"] = _case(*compatible(list(SUMMARIES)), run={"verbose": False})
    out["all_forward_no_burnin"] = _case(*compatible(list(SUMMARIES)), run={"burnin": 0})
    out["acquire_threshold"] = _case(extra_set=[lambda B, m: B.setAcquire(m.rel, 3, rule="prob_above", threshold=3.5, batch=2)])
    out["acquire_rows"] = _case(extra_set=[lambda B, m: B.setAcquire(m.rel, 2, rule="sd", rows=[2, 5, 24], exclude_listed=False, batch=2)])
    out["recommend_rows"] = _case(extra_set=[lambda B, m: B.setRecommend(m.rel, 2, rows=[2, 5, 24], exclude_listed=False, batch=2)])
    out["alpha_sample_lpd_waic_acquire"] = _case("lpd", "waic", "acquire", extra_set=[_alpha_sample])
    out["alpha_sample_new_rows"] = _case("new_test", run={"lpd": True}, extra_set=[_alpha_sample])
    out["ordinal_sampled_lpd_waic"] = _case("lpd", "waic", extra_set=[lambda B, m: _ordinal(B, m, True)])
    out["ordinal_fixed_lpd_waic"] = _case("lpd", "waic", extra_set=[lambda B, m: _ordinal(B, m, False)])
    out["ordinal_fixed"] = _case(extra_set=[lambda B, m: _ordinal(B, m, False, test=False)])
    out["entity_noise_lpd"] = _case("entity_noise", "lpd")
    out["new_rows_lpd"] = _case("new_test", run={"lpd": True})
    out["new_rows_observed_lpd"] = _case(model={"item_features": True}, run={"lpd": True}, extra_set=[lambda B, m: _new_rows(B, m, True)])
    out["new_rows_observed_no_features"] = _case(extra_set=[_new_rows_no_features])
    out["new_rows_no_test_lpd"] = _case("new_test", model={"test": False}, run={"lpd": True})
    out["reuse_robust_spike_recommend"] = _case("robust", "spike", "recommend", second=True)
    out["reuse_bias"] = _case("bias", second=True)
    out["reuse_nonneg_acquire"] = _case("nonneg", "acquire", second=True)
    out["second_relation_bias"] = _case(model={"extra": True}, extra_set=[lambda B, m: B.setBias(m.rel2, m.genres)])
    out["second_relation_entity_noise"] = _case(model={"extra": True}, extra_set=[lambda B, m: B.setEntityNoise(m.rel2, m.users)])
    out["no_test_waic_recommend_spike"] = _case("waic", "recommend", "spike", model={"test": False})
    out["no_test_robust_full_prediction"] = _case("robust", "full_prediction", model={"test": False})
    out["inline_rmse_train_clamp_f"] = _case(run={"rmse_train": True, "clamp": (1.0, 5.0), "f": "callback"})
    return out


# ---- hashing ----------------------------------------------------------------------------------------------------------
def _sha(a):
    a = np.ascontiguousarray(a)
    h = hashlib.sha256()
    h.update(f"{a.dtype.str}{a.shape}".encode())
    h.update(a.tobytes() if a.dtype != object else repr(a.tolist()).encode())
    return h.hexdigest()


def leaves(x, path="", out=None):
    """{path: what stands for the value}: a SHA-256 for arrays and the columns of frames, float.hex() for floats, repr otherwise"""
    out = {} if out is None else out
    if isinstance(x, dict):
        for k, v in x.items():
            leaves(v, f"{path}/{k}", out)
    elif isinstance(x, (list, tuple)):
        out[path + "/#"] = str(len(x))
        for k, v in enumerate(x):
            leaves(v, f"{path}/{k}", out)
    elif hasattr(x, "columns") and hasattr(x, "to_numpy"):                      # a pandas frame
        out[path + "/columns"] = repr([str(c) for c in x.columns])
        for c in x.columns:
            out[f"{path}/{c}"] = _sha(x[c].to_numpy())
    elif isinstance(x, np.ndarray):
        out[path] = _sha(x)
    elif isinstance(x, (float, np.floating)):
        out[path] = float(x).hex()
    else:
        out[path] = repr(x.item() if isinstance(x, np.generic) else x)
    return out


_TIMING = re.compile(r" \[\d+\.\d+s\]$")


def _call(B, data, kwargs):
    buf = io.StringIO()
    rec = {}
    try:
        with contextlib.redirect_stdout(buf):
            res = B.macau(data, **kwargs)
        rec["keys"] = list(res)
        rec["leaves"] = leaves(res)
    except Exception as e:          # noqa: BLE001 -- the message is what is recorded
        rec["error"] = f"{type(e).__name__}: {e}"
    rec["lines"] = [_TIMING.sub("", l) for l in buf.getvalue().splitlines()]
    return rec


def run_case(B, case, path):
    """the record of one case on one path: {"first": ..., "second": ...}"""
    had = os.environ.pop("BDF_NO_NATIVE", None)
    if path == "step":
        os.environ["BDF_NO_NATIVE"] = "1"
    try:
        kw = {}
        for key in case["keys"]:
            kw.update(SUMMARIES[key][0])
        kw.update(case["model"])
        run = dict(RUN, num_latent=D, seed=7, verbose=True)
        rec = {}
        try:
            m = Model(B, **kw)
            for key in case["keys"]:
                SUMMARIES[key][1](B, m)
                run.update(SUMMARIES[key][2])
            for fn in case["extra_set"]:
                fn(B, m)
        except B.ArgumentError as e:
            return {"first": {"error": f"set-up: {e}"}}
        run.update(case["run"])
        if run.get("f") == "callback":
            run["f"] = lambda data: float(np.sum(data.entities[0].model.sample[:, 0]))
        rec["first"] = _call(B, m.data, run)
        if case["second"] and "error" not in rec["first"]:
            rec["second"] = _call(B, m.data, dict(run, engine=m.data._engine, reset_model=False))
        eng = getattr(m.data, "_engine", None)
        if eng is not None:
            eng.close()
        return rec
    finally:
        os.environ.pop("BDF_NO_NATIVE", None)
        if had is not None:
            os.environ["BDF_NO_NATIVE"] = had


def brief(call):
    """one call's record as the golden keeps it: the keys of `result`, one SHA-256 over all its leaves, one over the verbose lines,
    and the last line as text (it shows every piece of the line in its order)"""
    out = {k: call[k] for k in ("error", "keys") if k in call}
    if "leaves" in call:
        out["result"] = hashlib.sha256(json.dumps(call["leaves"], sort_keys=True).encode()).hexdigest()
    out["lines"] = hashlib.sha256("\n".join(call["lines"]).encode()).hexdigest()
    out["last_line"] = call["lines"][-1] if call["lines"] else ""
    return out


def record(B, only=None, detail=False):
    """{case: {"options", "native": {call: record}, "step": the same, or "native" where it equals that one}}"""
    out = {}
    for name, case in cases().items():
        if only and name not in only:
            continue
        recs = {p: {c: r if detail else brief(r) for c, r in run_case(B, case, p).items()} for p in PATHS}
        out[name] = {"options": case["keys"], **{p: r if (p == PATHS[0] or r != recs[PATHS[0]]) else PATHS[0] for p, r in recs.items()}}
    return out


def write(rec, path):
    """one case per line: the file is read by a test, and by a person only when the test fails"""
    with open(path, "w") as f:
        f.write('{"run": %s, "unstable": %s, "cases": {\n' % (json.dumps(rec["run"], sort_keys=True), json.dumps(rec["unstable"], sort_keys=True)))
        f.write(",\n".join(f" {json.dumps(n)}: {json.dumps(c, sort_keys=True, ensure_ascii=False)}" for n, c in sorted(rec["cases"].items())))
        f.write("\n}}\n")


def differences(a, b, path=""):
    """the paths at which two records differ"""
    if isinstance(a, dict) and isinstance(b, dict):
        return [d for k in sorted(set(a) | set(b)) for d in (differences(a[k], b[k], f"{path}/{k}") if k in a and k in b else [f"{path}/{k}"])]
    return [] if a == b else [path]


def main(argv):
    import bdf_amd as B
    out_path, against, only, detail = GOLDEN, None, [], False
    args = list(argv)
    while args:
        a = args.pop(0)
        if a == "--out":
            out_path = args.pop(0)
        elif a == "--against":
            against = args.pop(0)
        elif a == "--detail":
            detail = True
        else:
            only.append(a)
    rec = {"run": dict(RUN, num_latent=D), "cases": record(B, only, detail), "unstable": {}}
    if against:
        with open(against) as f:
            first = json.load(f)
        for name in list(rec["cases"]):
            diff = differences(first["cases"].get(name, {}), rec["cases"][name])
            if diff:
                rec["unstable"][name] = diff
                del rec["cases"][name]
    write(rec, out_path)
    errors = {n: c[p]["first"]["error"] for n, c in rec["cases"].items() for p in PATHS if isinstance(c[p], dict) and "error" in c[p]["first"]}
    for n, e in errors.items():
        print(f"{n}: {e}")
    print(f"{len(rec['cases'])} cases, {len(errors)} that raise, {len(rec['unstable'])} unstable -> {out_path}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
