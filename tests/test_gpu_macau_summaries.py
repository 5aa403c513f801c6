"""macau()'s posterior summaries (summaries.py) against tests/golden/macau_summaries.json, which
tools/record_macau_results.py recorded -- twice, with equal outcome -- on the commit before the summaries had a module of their own:
per option, with every compatible option on, with no draws, with no burn-in, on an engine that is reused, with a second relation
and without test cells, on both iteration paths.  Per case: the keys of `result` in order, every leaf of it bit for bit (one
SHA-256 over them all) and every verbose line without its timing (one over them, the last line also as text).  When a case
fails, `tools/record_macau_results.py --detail --out FILE` on both commits shows which leaf or line differs."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("record_macau_results", os.path.join(ROOT, "tools", "record_macau_results.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TOOL = _tool()
with open(TOOL.GOLDEN) as _f:
    GOLDEN = json.load(_f)


def test_golden_holds_every_case_and_none_was_unstable():
    assert GOLDEN["unstable"] == {}
    assert set(GOLDEN["cases"]) == set(TOOL.cases())
    assert GOLDEN["run"] == dict(TOOL.RUN, num_latent=TOOL.D)
    for name, case in GOLDEN["cases"].items():
        assert set(case) == {"options", *TOOL.PATHS}, name


def test_cases_cover_what_the_summaries_can_get_wrong():
    cases = TOOL.cases()
    on = {k for c in cases.values() for k in c["keys"]}
    assert on == set(TOOL.SUMMARIES)
    assert all(k + "_no_draws" in cases for k in TOOL.SUMMARIES if k != "waic")
    reused = {k for c in cases.values() if c["second"] for k in c["keys"]}
    assert reused >= {"robust", "bias", "spike", "nonneg", "recommend", "acquire"}
    assert len(cases["all_forward"]["keys"]) >= 5 and cases["all_forward_no_burnin"]["run"] == {"burnin": 0}


@pytest.mark.parametrize("path", TOOL.PATHS)
@pytest.mark.parametrize("name", sorted(TOOL.cases()))
def test_macau_returns_and_prints_what_it_did(name, path):
    import bdf_amd as B
    want = GOLDEN["cases"][name][path]
    want = GOLDEN["cases"][name][want] if isinstance(want, str) else want          # ("native": this path gave what that one gave)
    got = TOOL.run_case(B, TOOL.cases()[name], path)
    assert set(got) == set(want)
    for call in sorted(want):
        w, g = want[call], TOOL.brief(got[call])
        assert g.get("error") == w.get("error"), (call, g.get("error"))
        assert g.get("keys") == w.get("keys"), call
        assert g["last_line"] == w["last_line"], call
        assert g["lines"] == w["lines"], (call, got[call]["lines"])
        assert g.get("result") == w.get("result"), (call, got[call].get("leaves"))
