"""Top-K lists (setRecommend) on the host (no GPU): the restatement against brute-force loops, the setter
and what it guards in both call orders, csrc/recommend.h compiled for the host, the entry points' declarations and the resource
listing the build leaves for the new kernels."""
import math
import os
import re
import shutil
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import background_restatement as BR
import recommend_restatement as RR
from test_probit_host import _resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bayesiandatafusion.jl_amd", "csrc")
# the tile of the accumulate kernel, as tests/test_gpu_recommend.py names it
TN, TM = 64, 128


def _relation(B, names=("u", "v")):
    ids, y, _ = BR.listing()
    return B.Relation({names[0]: ids[:, 0], names[1]: ids[:, 1], "y": y}, "plays", [B.Entity(nm) for nm in names], dims=[37, 29])


# ---- the restatement against brute force -------------------------------------------------------------------------------------------
def _case_7x9():
    """7 x 9 scores in eighths with ties; row 0 has every cell listed, row 1 none; row 2 has more relevant items than K"""
    rng = np.random.default_rng(3)
    S = rng.integers(-4, 5, (7, 9)) / 8.0
    S[3, :] = 0.25                                           # a row of equal scores: the item ids decide
    listed = [set(range(9)), set(), {0, 8}, {1}, {2, 3, 4}, {8}, {0}]
    relevant = [{1, 2}, {3}, {2, 3, 4, 5, 6, 7}, set(), {9}, {1, 9}, {5}]
    return S, listed, relevant


@pytest.mark.parametrize("K", [1, 3, 9, 12])
def test_restatement_lists_equal_the_brute_force_loop(K):
    S, listed, _ = _case_7x9()
    for lst in (listed, [set()] * 7):
        it, sc = RR.topk(S, K, lst)
        bi, bs = RR.brute_topk(S, K, lst)
        assert np.array_equal(it, bi) and np.array_equal(sc, bs, equal_nan=True)
    it, sc = RR.topk(S, K, listed)
    assert not it[0].any() and np.isnan(sc[0]).all()         # every cell listed: padding only
    assert np.array_equal(it[3, :min(K, 8)], [c for c in range(1, 10) if c != 2][:K])      # ties: rising item id
    assert np.array_equal(RR.topk(S, K)[0], RR.topk(S, K, [set()] * 7)[0])


@pytest.mark.parametrize("K", [1, 3, 9])
def test_restatement_metrics_equal_the_brute_force_loop(K):
    S, listed, relevant = _case_7x9()
    items, _ = RR.topk(S, K, listed)
    got, exp = RR.metrics(items, relevant), RR.brute_metrics(items, relevant)
    assert got[3] == exp[3] == 6                             # the row without a relevant item is left out
    assert np.allclose(got[:3], exp[:3], rtol=1e-14, atol=0)
    if K < 6:
        assert len(relevant[2]) > K                          # n_i > K: the ideal list is K long
    assert RR.metrics(np.zeros((7, K), dtype=np.int32), relevant)[:3] == (0.0, 0.0, 0.0)   # padding never hits
    assert RR.metrics(items, [set()] * 7)[3] == 0 and math.isnan(RR.metrics(items, [set()] * 7)[0])


def test_restatement_sum_equals_the_dense_product_and_a_row_subset():
    rng = np.random.default_rng(4)
    draws = [(rng.standard_normal((7, 6)), rng.standard_normal((9, 6))) for _ in range(3)]
    acc, mag = RR.score_sum(draws)
    exp = sum(U @ V.T for U, V in draws)
    assert np.all(np.abs(acc - exp) <= 1e-14 * mag)
    sub, _ = RR.score_sum(draws, rows0=[5, 0, 2])
    assert np.array_equal(sub, acc[[5, 0, 2]])
    assert np.array_equal(RR.scores_of(acc, 3, 0.5), acc / 3.0 + 0.5)
    assert np.isnan(RR.scores_of(np.zeros((2, 2)), 0, 1.0)).all()


# ---- the setter ----------------------------------------------------------------------------------------------------------------------
def test_default_has_none_and_tostr_has_no_tag(B):
    rel = _relation(B)
    assert rel.model.recommend is None and B.RelationModel().recommend is None
    assert "rec:" not in B.toStr(rel)


def test_setrecommend_stores_its_arguments_and_resets_the_device_state(B):
    rel = _relation(B)
    rel._dev = object()
    assert B.setRecommend(rel, 10) is None
    assert rel.model.recommend == {"k": 10, "rows": None, "exclude_listed": True, "batch": 8} and rel._dev is None
    B.setRecommend(rel, 64, rows=[5, 1, 37], exclude_listed=False, batch=32)
    m = rel.model.recommend
    assert m["k"] == 64 and m["batch"] == 32 and m["exclude_listed"] is False and np.array_equal(m["rows"], [5, 1, 37])
    assert "rec:64" in B.toStr(rel)
    from bdf_amd.relation_data import check_model
    check_model(rel)


@pytest.mark.parametrize("bad", [0, 65, -1, 2.0, "3", None, True])
def test_refuses_a_k_out_of_range(B, bad):
    rel = _relation(B)
    with pytest.raises(B.ArgumentError, match="k = "):
        B.setRecommend(rel, bad)
    assert rel.model.recommend is None


@pytest.mark.parametrize("bad", [0, 33, 1.5, "8", None, False])
def test_refuses_a_batch_out_of_range(B, bad):
    rel = _relation(B)
    with pytest.raises(B.ArgumentError, match="batch = "):
        B.setRecommend(rel, 5, batch=bad)


@pytest.mark.parametrize("bad,what", [([0, 1], "outside"), ([1, 38], "outside"), ([3, 3], "more than once"), ([1.0, 2.0], "integer ids"),
                                      ([[1, 2]], "integer ids"), ("ab", "integer ids"), ([True, False], "integer ids")])
def test_refuses_bad_rows(B, bad, what):
    rel = _relation(B)
    with pytest.raises(B.ArgumentError, match=what):
        B.setRecommend(rel, 5, rows=bad)


def test_check_model_repeats_the_range_checks(B):
    from bdf_amd.relation_data import check_model
    rel = _relation(B)
    B.setRecommend(rel, 5)
    for field, bad in (("k", 0), ("batch", 40), ("rows", [2, 2])):
        keep = rel.model.recommend[field]
        rel.model.recommend[field] = bad
        with pytest.raises(B.ArgumentError, match="setRecommend"):
            check_model(rel)
        rel.model.recommend[field] = keep
    check_model(rel)


def test_refuses_three_modes(B):
    rng = np.random.default_rng(0)
    t = {"a": rng.integers(1, 5, 20), "b": rng.integers(1, 6, 20), "c": rng.integers(1, 4, 20), "y": rng.standard_normal(20)}
    rel = B.Relation(t, "tensor", [B.Entity("a"), B.Entity("b"), B.Entity("c")], dims=[4, 5, 3])
    with pytest.raises(B.ArgumentError, match="has 3 modes"):
        B.setRecommend(rel, 5)


def test_refuses_relation_features_in_both_orders(B):
    from bdf_amd.relation_data import check_model
    rel = _relation(B)
    rel.F = np.ones((rel.data.nnz(), 2))
    with pytest.raises(B.ArgumentError, match="has features"):
        B.setRecommend(rel, 5)
    rel = _relation(B)
    B.setRecommend(rel, 5)
    rel.F = np.ones((rel.data.nnz(), 2))
    with pytest.raises(B.ArgumentError, match="has features.*setRecommend"):
        check_model(rel)


def test_an_entitys_side_information_is_fine(B):
    from bdf_amd.relation_data import check_model
    rel = _relation(B)
    rel.entities[0].F = np.ones((37, 3))
    B.setRecommend(rel, 5)
    check_model(rel)


def _binary(B):
    ids, _, _ = BR.listing()
    return B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": np.resize([0.0, 1.0], len(ids))}, "plays", [B.Entity("u"), B.Entity("v")], dims=[37, 29])


@pytest.mark.parametrize("name", ["setProbit", "setLogit", "setCounts"])
def test_refuses_the_links_whose_prediction_is_not_the_dot_product_in_both_orders(B, name):
    from bdf_amd.relation_data import check_model
    setter = {"setProbit": lambda r: B.setProbit(r), "setLogit": lambda r: B.setLogit(r), "setCounts": lambda r: B.setCounts(r, 2)}[name]
    rel = _binary(B)
    setter(rel)
    with pytest.raises(B.ArgumentError, match="setRecommend"):
        B.setRecommend(rel, 5)
    assert rel.model.recommend is None
    rel = _binary(B)
    B.setRecommend(rel, 5)
    setter(rel)
    with pytest.raises(B.ArgumentError, match="setRecommend"):
        check_model(rel)


@pytest.mark.parametrize("name", ["setWeights", "setRobust", "setCensored", "setInterval", "setBinned", "setOrdinal", "setBackground"])
def test_the_other_noise_models_take_it_in_both_orders(B, name):
    from bdf_amd.relation_data import check_model
    ids, _, _ = BR.listing()
    n = len(ids)

    def make():
        return B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": np.resize([1.0, 2.0, 3.0, 4.0], n)}, "plays", [B.Entity("u"), B.Entity("v")], dims=[37, 29])
    setter = {"setWeights": lambda r: B.setWeights(r, np.full(n, 2.0)), "setRobust": lambda r: B.setRobust(r),
              "setCensored": lambda r: B.setCensored(r, np.zeros(n, dtype=np.int8)),
              "setInterval": lambda r: B.setInterval(r, r.data.values - 1.0, r.data.values + 1.0), "setBinned": lambda r: B.setBinned(r, [0.0, 1.5, 2.5, 4.5]),
              "setOrdinal": lambda r: B.setOrdinal(r), "setBackground": lambda r: B.setBackground(r, 0.1)}[name]
    for first in (True, False):
        rel = make()
        if first:
            setter(rel)
            B.setRecommend(rel, 5)
        else:
            B.setRecommend(rel, 5)
            setter(rel)
        check_model(rel)
        assert rel.model.recommend["k"] == 5


def test_refuses_more_than_one_rank(B):
    from bdf_amd.relation_data import check_model
    rel = _relation(B)
    B.setRecommend(rel, 5)
    check_model(rel, 1)
    with pytest.raises(B.ArgumentError, match=r"setRecommend\): one rank only"):
        check_model(rel, 2)


def test_macau_refuses_a_later_relation(B):
    u, v, w = B.Entity("u"), B.Entity("v"), B.Entity("w")
    ids, y, _ = BR.listing()
    r1 = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "plays", [u, v], dims=[37, 29])
    r2 = B.Relation({"u": ids[:, 0], "w": ids[:, 1], "y": y}, "skips", [u, w], dims=[37, 29])
    rd = B.RelationData(r1)
    B.addRelation(rd, r2)
    B.setRecommend(r2, 5)
    with pytest.raises(B.ArgumentError, match="skips.*not the first relation"):
        B.macau(rd, num_latent=4, burnin=1, psamples=1, verbose=False)


@pytest.mark.parametrize("who", ["bpmf_vb", "macau_hmc"])
def test_the_other_trainers_refuse_it(B, who):
    from bdf_amd._two_mode import relation_of
    rel = _relation(B)
    B.setRecommend(rel, 5)
    with pytest.raises(B.ArgumentError, match=who + ".*setRecommend"):
        relation_of(B.RelationData(rel), 8, who)


# ---- csrc/recommend.h on the host ----------------------------------------------------------------------------------------------------
_HOST_SRC = r"""
#include <cstdio>
#include <cstring>
#include <cstdint>
#include "recommend.h"
int main() {
    for (int r = 1; r <= BDF_REC_MAX_K; r++) { double d = bdf_rec_discount(r); uint64_t u; memcpy(&u, &d, 8); printf("%016llx\n", (unsigned long long)u); }
    double sa, sb; int ia, ib;
    while (scanf("%lf %d %lf %d", &sa, &ia, &sb, &ib) == 4) printf("%d\n", bdf_rec_before(sa, ia, sb, ib) ? 1 : 0);
    printf("%.17g\n", bdf_rec_score(7.0, 3.0, 0.1));
    return 0;
}
"""


def test_recommend_header_on_the_host():
    cxx = [shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")]
    if cxx[0] is None:
        cxx = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "c++"]
    rng = np.random.default_rng(6)
    n = 200
    score = rng.integers(-3, 4, n) / 8.0                     # seven values: many repeats
    item = rng.permutation(1000)[:n] + 1                     # distinct items
    pairs = [(a, b) for a in range(n) for b in range(n)]
    td = tempfile.mkdtemp()
    try:
        open(os.path.join(td, "t.cpp"), "w").write(_HOST_SRC)
        subprocess.run(cxx + ["-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, os.path.join(td, "t.cpp"), "-o", os.path.join(td, "t")], check=True)
        text = "".join("%.17g %d %.17g %d\n" % (score[a], item[a], score[b], item[b]) for a, b in pairs)
        out = subprocess.run([os.path.join(td, "t")], input=text, capture_output=True, text=True, check=True).stdout.split()
    finally:
        shutil.rmtree(td, ignore_errors=True)
    # the discount, to the bit
    for r in range(1, 65):
        assert out[r - 1] == "%016x" % struct.unpack("<Q", struct.pack("<d", 1.0 / math.log2(r + 1)))[0], r
    before = np.array([int(x) for x in out[64:64 + n * n]], dtype=bool).reshape(n, n)
    assert float(out[64 + n * n]) == 7.0 / 3.0 + 0.1
    # a strict total order: irreflexive, exactly one of a < b and b < a for a != b, transitive
    assert not before.diagonal().any()
    assert np.array_equal(before ^ before.T, ~np.eye(n, dtype=bool))
    bi = before.astype(np.int64)
    assert not np.any((bi @ bi > 0) & ~before)
    # ... and the one the lists are specified by: falling score, equal scores by rising item
    order = np.lexsort((item, -score))
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.arange(n)
    assert np.array_equal(before, rank[:, None] < rank[None, :])


# ---- the C ABI and the build's listing ------------------------------------------------------------------------------------------------
ENTRY_POINTS = ("bdf_scores_create", "bdf_scores_destroy", "bdf_scores_push", "bdf_scores_flush", "bdf_scores_topk", "bdf_scores_metrics",
                "bdf_scores_copy", "bdf_scores_set_draws")


def test_entry_points_are_declared_bound_and_documented(B):
    h = open(os.path.join(ROOT, "include", "bdf.h")).read()
    jl = open(os.path.join(ROOT, "julia", "BDFHip.jl")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRY_POINTS:
        assert name + "(" in h and name in B.declared_symbols() and (":" + name) in jl and name in doc, name
    assert "typedef struct bdf_scores bdf_scores;" in h
    assert "setRecommend" in B.__dict__ and "setRecommend" in open(os.path.join(ROOT, "README.md")).read()


def test_new_kernels_use_no_scratch_and_fit_the_register_file():
    res = _resources("k_recommend")
    names = sorted(res)
    assert len(res) == 7, names
    for stem, count in (("k_scores_accum", 3), ("k_scores_push", 1), ("k_topk_rows", 1), ("k_rec_metrics", 2)):
        assert sum(stem in k for k in names) == count, (stem, names)
    for k, (vgprs, scratch, occ) in res.items():
        assert scratch == 0, (k, scratch)
        assert vgprs <= 256 and occ >= 1, (k, vgprs, occ)


def test_tile_constants_are_the_ones_the_gpu_tests_name():
    text = open(os.path.join(CSRC, "recommend.h")).read()
    got = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (BDF_REC_\w+) (\d+)", text)}
    import test_gpu_recommend as G
    assert (got["BDF_REC_TN"], got["BDF_REC_TM"]) == (TN, TM) == (G.TN, G.TM)
    assert got["BDF_REC_TN"] % got["BDF_REC_WN"] == 0 and got["BDF_REC_TM"] % got["BDF_REC_WM"] == 0
    assert got["BDF_REC_WN"] % 16 == 0 and got["BDF_REC_WM"] % 16 == 0
    assert (got["BDF_REC_TN"] // got["BDF_REC_WN"]) * (got["BDF_REC_TM"] // got["BDF_REC_WM"]) == 4      # the workgroup's four waves
    assert got["BDF_REC_MAX_K"] == 64 and got["BDF_REC_MAX_BATCH"] == 32
    from bdf_amd.relation_data import RECOMMEND_MAX_BATCH, RECOMMEND_MAX_K
    assert (RECOMMEND_MAX_K, RECOMMEND_MAX_BATCH) == (got["BDF_REC_MAX_K"], got["BDF_REC_MAX_BATCH"])
