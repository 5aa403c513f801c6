"""The table of model options (model_options.py) against tests/golden/option_outcomes.json, which tools/record_option_outcomes.py
recorded from the hand-written guards the table replaced: every option alone, every ordered pair of options, every option on two
ranks, under bpmf_vb and macau_hmc, and macau()'s lpd / rmse_train / full_prediction per noise kind.  Host only."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("record_option_outcomes", os.path.join(ROOT, "tools", "record_option_outcomes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


T = _tool()
with open(T.GOLDEN) as f:
    GOLD = json.load(f)


@pytest.fixture(scope="module")
def now(B):
    """the recording's cases, run once on the working tree"""
    return T.record(B)


def _keys(option):
    return T.REGISTRY_KEYS.get(option, (option,))


def _split(pair):
    return tuple(pair.split(">"))


def test_every_option_alone_is_accepted():
    assert list(GOLD["options"]) == list(T.OPTIONS)
    assert {a: c["outcome"] for a, c in GOLD["single"].items()} == {a: "ok" for a in T.OPTIONS}


@pytest.mark.parametrize("section", ["single", "ranks", "pairs", "trainers", "macau"])
def test_outcomes_are_the_recorded_ones(now, section):
    assert set(now[section]) == set(GOLD[section])                     # every case, none left out
    assert len(GOLD["pairs"]) == len(T.OPTIONS) * (len(T.OPTIONS) - 1)
    differ = {k: (GOLD[section][k]["outcome"], c["outcome"], c["message"]) for k, c in now[section].items()
              if c["outcome"] != GOLD[section][k]["outcome"]}
    assert not differ


def _says(message, key):
    from bdf_amd.model_options import OPTION
    return OPTION[key].phrase in message or (OPTION[key].has is not None and OPTION[key].has in message)


def test_a_refusal_names_its_subject_and_both_options(now):
    for pair, c in now["pairs"].items():
        if c["outcome"] == "ok":
            continue
        a, b = _split(pair)
        assert any(name in c["message"] for name in ("Relation ratings", "Entity users", "Entity items")), (pair, c["message"])
        for option in (a, b):
            assert any(_says(c["message"], k) for k in _keys(option)), (pair, option, c["message"])
    for case, c in now["macau"].items():
        if c["outcome"] != "ok":
            flag, kind = case.split(":")
            assert "Relation ratings" in c["message"] and _says(c["message"], flag) and _says(c["message"], kind), (case, c["message"])
    for case, c in now["trainers"].items():
        if c["outcome"] != "ok":
            who, option = case.split(":")
            assert who in c["message"] and any(_says(c["message"], k) for k in _keys(option)), (case, c["message"])


def _with_setters():
    return [a for a in GOLD["options"] if a not in GOLD["no_setter"]]


def test_the_late_list_is_exactly_the_recorded_asymmetries():
    """(A, B) is in _REFUSED_ONLY_AT_BUILD iff the recording has A then B refused by the build alone and B then A by A's setter"""
    from bdf_amd.model_options import _REFUSED_ONLY_AT_BUILD, refused
    out = {_split(p): c["outcome"] for p, c in GOLD["pairs"].items()}
    seen = set()
    for a in _with_setters():
        for b in _with_setters():
            if a == b:
                continue
            late = {(ka, kb) for ka in _keys(a) for kb in _keys(b)} & _REFUSED_ONLY_AT_BUILD
            if out[a, b] == "build":
                assert out[b, a] == "set" and late, (a, b)
            else:
                assert not late, (a, b, late)
            seen |= late
    assert seen == _REFUSED_ONLY_AT_BUILD
    assert all(refused(a, b)[0] for a, b in _REFUSED_ONLY_AT_BUILD)


def test_the_table_is_symmetric_apart_from_the_late_list():
    from bdf_amd.model_options import OPTION, RUN, refused
    for a in OPTION:
        for b in OPTION:
            assert refused(a, b)[0] == refused(b, a)[0]
    # and so is the recording, for the options that a setter leaves on the relation or the entity (setPrecision and the test
    # bounds, which only macau(lpd=True) reads, are never found there by another setter)
    stays = [a for a in _with_setters() if not all(OPTION[k].scope == RUN for k in _keys(a))]
    out = {_split(p): c["outcome"] != "ok" for p, c in GOLD["pairs"].items()}
    assert not [(a, b) for a in stays for b in stays if a != b and out[a, b] != out[b, a]]


# fields that are parameters, state or bookkeeping, not options: a new field goes here or into the registry
RELATION_PARAMETERS = {"alpha_nu0", "alpha_lambda0", "lambda_beta", "alpha", "beta", "mean_value", "ordinal_codes", "ordinal_edges"}
ENTITY_PARAMETERS = {"FF", "use_FF", "relations", "count", "name", "modes", "modes_other", "lambda_beta", "lambda_beta_sample", "mu", "nu", "model"}


def test_every_option_field_is_in_the_registry(B):
    from bdf_amd.model_options import ENTITY, OPTIONS
    fields = {scope: {o.field for o in OPTIONS if o.field is not None and (o.scope == ENTITY) == (scope == ENTITY)} for scope in (ENTITY, "relation")}
    assert set(vars(B.RelationModel())) - RELATION_PARAMETERS <= fields["relation"]
    assert set(vars(B.Entity("e"))) - ENTITY_PARAMETERS <= fields[ENTITY]
    assert len({o.key for o in OPTIONS}) == len(OPTIONS)
