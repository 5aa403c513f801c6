#!/usr/bin/env python3
"""Which model options a relation and its entities take together, recorded from the code itself (host only: the built library, no device).

    python tools/record_option_outcomes.py            writes tests/golden/option_outcomes.json
    python tools/record_option_outcomes.py --matrix   prints the matrix of the working tree as text and writes nothing

A case builds a fresh two-entity RelationData (a 4 x 4 relation, 10 distinct cells listed, all values 1, features on the second
entity only), applies option A, then option B, then the build-time pass -- check_model on the relation, check_spike and check_nonneg
on its entities, check_new_rows -- and records "set" if B's setter refused, "build" if only the pass did, "ok" otherwise, with the
message.  Every option alone is recorded too (all "ok"), each alone on two ranks, what relation_of (bpmf_vb, macau_hmc) says to each,
and what macau() says to lpd, rmse_train and full_prediction per noise kind.  tests/test_option_table_host.py replays the file on
the working tree: record it on the commit whose behaviour is to be kept.

Entity priors go on the first entity (the one without features), setNewRows / setNewTest on the second.  "test_ordinal" makes the
relation ordinal first when it is not; "new_test" gives the second entity new rows first when it has none.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "option_outcomes.json")

CELLS = [(1, 1), (1, 2), (2, 2), (2, 3), (3, 3), (3, 4), (4, 4), (4, 1), (1, 3), (2, 4)]
TEST_CELLS = [(3, 1), (4, 2)]


def fixture(B):
    e1, e2 = B.Entity("users"), B.Entity("items", F=np.arange(8.0).reshape(4, 2) + 1.0)
    ids = np.array(CELLS, dtype=np.int64)
    r = B.Relation((ids, np.ones(len(ids))), "ratings", [e1, e2], dims=[4, 4])
    B.setTest(r, (np.array(TEST_CELLS, dtype=np.int64), np.ones(len(TEST_CELLS))))
    return B.RelationData(r), r, e1, e2


def _features(B, d, r, e1, e2):
    r.F = np.ones((len(CELLS), 2))


def _alpha_sample(B, d, r, e1, e2):
    r.model.alpha_sample = True


def _entity_features(B, d, r, e1, e2):
    e1.F = np.arange(8.0).reshape(4, 2) + 1.0


def _test_ordinal(B, d, r, e1, e2):
    if r.model.ordinal is None:
        B.setOrdinal(r, 4)
    B.setTestOrdinal(r)


def _new_test(B, d, r, e1, e2):
    if e2.new_rows is None:
        B.setNewRows(e2, np.ones((2, 2)))
    B.setNewTest(r, e2, (np.array([[1, 1], [2, 2]], dtype=np.int64), np.ones(2)))


n = len(CELLS)
OPTIONS = {
    "features": _features,
    "alpha_sample": _alpha_sample,
    "precision": lambda B, d, r, e1, e2: B.setPrecision(r, 2.0),
    "probit": lambda B, d, r, e1, e2: B.setProbit(r),
    "censored": lambda B, d, r, e1, e2: B.setCensored(r, np.array([1] + [0] * (n - 1))),
    "interval": lambda B, d, r, e1, e2: B.setInterval(r, np.full(n, 0.5), np.full(n, 1.5)),
    "ordinal": lambda B, d, r, e1, e2: B.setOrdinal(r, 4),
    "robust": lambda B, d, r, e1, e2: B.setRobust(r),
    "weights": lambda B, d, r, e1, e2: B.setWeights(r, np.full(n, 2.0)),
    "logit": lambda B, d, r, e1, e2: B.setLogit(r),
    "counts": lambda B, d, r, e1, e2: B.setCounts(r, 2),
    "entity_noise": lambda B, d, r, e1, e2: B.setEntityNoise(r, e1),
    "bias": lambda B, d, r, e1, e2: B.setBias(r, e1),
    "background": lambda B, d, r, e1, e2: B.setBackground(r, 0.5),
    "dense": lambda B, d, r, e1, e2: B.setDense(r),
    "recommend": lambda B, d, r, e1, e2: B.setRecommend(r, 2),
    "waic": lambda B, d, r, e1, e2: B.setWaic(r),
    "test_interval": lambda B, d, r, e1, e2: B.setTestInterval(r, np.full(len(TEST_CELLS), 0.5), np.full(len(TEST_CELLS), 1.5)),
    "test_ordinal": _test_ordinal,
    "new_test": _new_test,
    "entity_features": _entity_features,
    "spike": lambda B, d, r, e1, e2: B.setSpikeAndSlab(e1),
    "nonneg": lambda B, d, r, e1, e2: B.setNonNegative(e1),
    "new_rows": lambda B, d, r, e1, e2: B.setNewRows(e2, np.ones((2, 2))),
}
NO_SETTER = ("features", "alpha_sample", "entity_features")      # plain assignments: nothing can refuse them before the build
REGISTRY_KEYS = {"test_ordinal": ("ordinal", "test_ordinal"), "new_test": ("new_test", "new_rows")}     # (the others set the option of their name)
NOISE_KINDS = ("gauss", "probit", "censored", "interval", "ordinal", "robust", "weights", "logit", "counts", "entity_noise")


def build_pass(B, d, world=1):
    from bdf_amd.relation_data import check_model, check_new_rows, check_nonneg, check_spike
    for r in d.relations:
        check_model(r, world)
    for en in d.entities:
        if en.spike is not None:
            check_spike(en, world)
        if en.nonneg is not None:
            check_nonneg(en, world)
    if check_new_rows(d) is not None:
        check_new_rows(d, world)


def run_case(B, first, second=None, world=1):
    """(outcome, message) of option `first`, then `second`, then the build-time pass"""
    d, r, e1, e2 = fixture(B)
    OPTIONS[first](B, d, r, e1, e2)
    try:
        if second is not None:
            OPTIONS[second](B, d, r, e1, e2)
    except B.ArgumentError as e:
        return "set", str(e)
    try:
        build_pass(B, d, world)
    except B.ArgumentError as e:
        return "build", str(e)
    return "ok", ""


class _HostChecksPassed(Exception):
    pass


class _NoEngine:
    """stands where macau() expects an engine: the first thing macau() asks of it ends the call, after all its host-side refusals"""

    def __getattr__(self, name):
        raise _HostChecksPassed(name)


def run_macau(B, kind, flag):
    d, r, e1, e2 = fixture(B)
    if kind != "gauss":
        OPTIONS[kind](B, d, r, e1, e2)
    try:
        B.macau(d, num_latent=2, burnin=1, psamples=2, verbose=False, engine=_NoEngine(), reset_model=False, **{flag: True})
    except B.ArgumentError as e:
        return "refused", str(e)
    except _HostChecksPassed:
        return "ok", ""
    raise AssertionError("macau() ran without an engine")


def run_trainer(B, option, who):
    from bdf_amd._two_mode import relation_of
    d, r, e1, e2 = fixture(B)
    OPTIONS[option](B, d, r, e1, e2)
    try:
        relation_of(d, 2, who)
    except B.ArgumentError as e:
        return "refused", str(e)
    return "ok", ""


def record(B):
    def cell(outcome, message):
        return {"outcome": outcome, "message": message}
    out = {"options": list(OPTIONS), "no_setter": list(NO_SETTER)}
    out["single"] = {a: cell(*run_case(B, a)) for a in OPTIONS}
    out["ranks"] = {a: cell(*run_case(B, a, world=2)) for a in OPTIONS}
    out["pairs"] = {f"{a}>{b}": cell(*run_case(B, a, b)) for a in OPTIONS for b in OPTIONS if a != b}
    out["trainers"] = {f"{who}:{a}": cell(*run_trainer(B, a, who)) for who in ("bpmf_vb", "macau_hmc") for a in OPTIONS}
    out["macau"] = {f"{flag}:{k}": cell(*run_macau(B, k, flag)) for flag in ("lpd", "rmse_train", "full_prediction") for k in NOISE_KINDS}
    return out


def matrix_text(rec):
    """rows: the option that is there; columns: the one that comes.  S: its setter refuses, B: only the build does, .: accepted"""
    opts = rec["options"]
    w = max(len(o) for o in opts)
    lines = [" " * w + " " + " ".join(f"{i:2d}" for i in range(1, len(opts) + 1))]
    for i, a in enumerate(opts, 1):
        row = [" -" if a == b else {"set": " S", "build": " B", "ok": " ."}[rec["pairs"][f"{a}>{b}"]["outcome"]] for b in opts]
        lines.append(f"{a:>{w}s} " + " ".join(row) + f"   {i}")
    return "\n".join(lines)


def main(argv):
    import bdf_amd as B
    rec = record(B)
    if "--matrix" in argv:
        print(matrix_text(rec))
        return 0
    bad = [a for a, c in rec["single"].items() if c["outcome"] != "ok"]
    if bad:
        raise SystemExit(f"options refused on their own, the fixture is wrong: {bad}")
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True, ensure_ascii=False)
        f.write("\n")
    print(f"{len(rec['pairs'])} pairs -> {GOLDEN}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
