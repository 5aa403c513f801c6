"""Acquisition lists (setAcquire) on the host (no GPU): the setter and every argument it refuses, the option
table's rows for it in both orders, the other trainers and two ranks, the Welford restatement of tests/acquire_restatement.py against
np.mean / np.var in extended precision, csrc/acquire.h compiled for the host against the restatement's scores, the resource listing
the build leaves for the kernels of k_acquire.hip (no scratch) and the header's declarations in the bindings."""
import os
import re
import shutil
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import acquire_restatement as AR
import background_restatement as BR
from test_foldin_host import _resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bayesiandatafusion.jl_amd", "csrc")
# the tile of k_acquire_accum, as tests/test_gpu_acquire.py names it
TN, TM = 64, 64


def _relation(B, values=None, names=("u", "v")):
    ids, y, _ = BR.listing()
    y = y if values is None else np.resize(np.asarray(values, dtype=np.float64), len(ids))
    return B.Relation({names[0]: ids[:, 0], names[1]: ids[:, 1], "y": y}, "plays", [B.Entity(nm) for nm in names], alpha=2.0, dims=[37, 29])


# ---- the setter -------------------------------------------------------------------------------------------------------------------
def test_setter_round_trips_and_clears(B):
    from bdf_amd.relation_data import check_model
    rel = _relation(B)
    assert rel.model.acquire is None and B.RelationModel().acquire is None and "acq:" not in B.toStr(rel)
    rel._dev = object()
    assert B.setAcquire(rel, 5) is None
    assert rel._dev is None                                  # (the device state is built again)
    assert rel.model.acquire == {"k": 5, "rule": "ucb", "kappa": 1.0, "threshold": None, "rows": None, "exclude_listed": True, "batch": 8}
    assert "acq:5" in B.toStr(rel) and "rec:" not in B.toStr(rel)
    B.setAcquire(rel, 64, rule="prob_above", threshold=6, rows=[30, 3, 1], exclude_listed=False, batch=32, kappa=0)
    m = rel.model.acquire
    assert m["k"] == 64 and m["rule"] == "prob_above" and m["threshold"] == 6.0 and isinstance(m["threshold"], float) and m["kappa"] == 0.0
    assert m["rows"].tolist() == [30, 3, 1] and m["rows"].dtype == np.int64 and m["exclude_listed"] is False and m["batch"] == 32
    B.setAcquire(rel, np.int64(3), rule="sd", kappa=np.float64(0.25))
    assert rel.model.acquire["rule"] == "sd" and rel.model.acquire["k"] == 3 and rel.model.acquire["threshold"] is None
    check_model(rel)
    rel._dev = object()
    B.setAcquire(rel, None)
    assert rel.model.acquire is None and rel._dev is None and "acq:" not in B.toStr(rel)
    assert "setAcquire" in B.__dict__ and "LISTED cells' precision" in B.setAcquire.__doc__


BAD_ARGUMENTS = [
    (dict(k=0), "k = 0 must be an integer in 1 ... 64"), (dict(k=65), "k = 65"), (dict(k=2.0), "k = 2.0"), (dict(k=True), "k = True"),
    (dict(k=3, batch=0), "batch = 0 must be an integer in 1 ... 32"), (dict(k=3, batch=33), "batch = 33"), (dict(k=3, batch=1.5), "batch = 1.5"),
    (dict(k=3, exclude_listed=1), "exclude_listed = 1 must be true or false"),
    (dict(k=3, rows=[1.5]), "rows must be a list of integer ids of u"), (dict(k=3, rows=[[1, 2]]), "rows must be a list"),
    (dict(k=3, rows=[True]), "rows must be a list"), (dict(k=3, rows=[0]), r"outside 1 \.\.\. 37"), (dict(k=3, rows=[38]), r"outside 1 \.\.\. 37"),
    (dict(k=3, rows=[2, 2]), "more than once"),
    (dict(k=3, rule="ei"), "rule = 'ei' must be one of 'ucb', 'sd', 'prob_above'"), (dict(k=3, rule=0), "rule = 0 must be one of"),
    (dict(k=3, kappa=-0.5), "kappa = -0.5 must be a finite number, not negative"), (dict(k=3, kappa=float("inf")), "kappa = inf"),
    (dict(k=3, kappa=float("nan")), "kappa = nan"), (dict(k=3, kappa="1"), "kappa = 1 must be"), (dict(k=3, kappa=True), "kappa = True"),
    (dict(k=3, rule="prob_above"), "needs a finite threshold, not None"), (dict(k=3, rule="prob_above", threshold=float("inf")), "finite threshold, not inf"),
    (dict(k=3, rule="prob_above", threshold=float("nan")), "finite threshold"), (dict(k=3, rule="prob_above", threshold="6"), "finite threshold"),
    (dict(k=3, rule="ucb", threshold=6.0), "a threshold goes with rule 'prob_above', not with 'ucb'"),
    (dict(k=3, rule="sd", threshold=6.0), "not with 'sd'"),
]


@pytest.mark.parametrize("args,what", BAD_ARGUMENTS)
def test_setter_refuses_bad_arguments(B, args, what):
    rel = _relation(B)
    with pytest.raises(B.ArgumentError, match=r"Relation plays: .*" + what + r".*\(setAcquire\)\."):
        B.setAcquire(rel, **args)
    assert rel.model.acquire is None                         # a refused call changes nothing


def test_setrecommend_still_names_itself(B):
    """the shared checks name the setter that called them"""
    rel = _relation(B)
    with pytest.raises(B.ArgumentError, match=r"k = 0 must be an integer in 1 \.\.\. 64 \(setRecommend\)"):
        B.setRecommend(rel, 0)
    with pytest.raises(B.ArgumentError, match=r"more than once \(setRecommend\)"):
        B.setRecommend(rel, 3, rows=[1, 1])


def test_check_model_repeats_the_checks(B):
    from bdf_amd.relation_data import check_model
    rel = _relation(B)
    B.setAcquire(rel, 5)
    for field, bad, what in (("k", 0, "k = 0"), ("batch", 99, "batch = 99"), ("rows", [0], "outside"), ("exclude_listed", 2, "exclude_listed"),
                             ("rule", "ei", "rule = 'ei'"), ("kappa", -1.0, "kappa = -1.0"), ("threshold", 1.0, "a threshold goes with")):
        keep, rel.model.acquire[field] = rel.model.acquire[field], bad
        with pytest.raises(B.ArgumentError, match=what):
            check_model(rel)
        rel.model.acquire[field] = keep
    check_model(rel)


def test_refuses_three_modes(B):
    rng = np.random.default_rng(0)
    t = {"a": rng.integers(1, 5, 20), "b": rng.integers(1, 6, 20), "c": rng.integers(1, 4, 20), "y": rng.standard_normal(20)}
    r3 = B.Relation(t, "cube", [B.Entity("a"), B.Entity("b"), B.Entity("c")])
    with pytest.raises(B.ArgumentError, match=r"has 3 modes: acquisition lists \(setAcquire\) take a two-mode relation"):
        B.setAcquire(r3, 3)


# ---- the option table -------------------------------------------------------------------------------------------------------------
def _dense_relation(B):
    i, j = np.meshgrid(np.arange(1, 10), np.arange(1, 8), indexing="ij")
    ents = [B.Entity("u"), B.Entity("v")]
    return B.Relation({"u": i.ravel(), "v": j.ravel(), "y": np.random.default_rng(1).standard_normal(63)}, "plays", ents, alpha=2.0, dims=[9, 7])


def _new_test(B, r):
    e = r.entities[0]
    B.setNewRows(e, np.ones((2, 3)))
    B.setNewTest(r, e, {"u": [1, 2], "v": [1, 2], "y": [0.5, 0.25]})


def _new_test_fresh(B):
    r = _relation(B)
    r.entities[0].F = np.ones((37, 3))
    return r


def _features(r):
    r.F = np.ones((r.data.nnz(), 2))


# (option key, the relation's values it needs or a maker of the relation, its setter, the table's reason) of everything setAcquire refuses
def _refused_with(B):
    ones = lambda r: np.ones(r.data.nnz())
    not_dot, not_one, new_row = "its prediction is not u.v \\+ mean", "an unlisted cell's precision is not one alpha", "no list is ranked for a new row"
    return [("probit", [0.0, 1.0], lambda r: B.setProbit(r), not_dot), ("logit", [0.0, 1.0], lambda r: B.setLogit(r), not_dot),
            ("counts", [0.0, 3.0, 1.0], lambda r: B.setCounts(r, 2), not_dot),
            ("robust", None, lambda r: B.setRobust(r), not_one), ("weights", None, lambda r: B.setWeights(r, ones(r)), not_one),
            ("entity_noise", None, lambda r: B.setEntityNoise(r, r.entities[0]), not_one),
            ("ordinal", [1.0, 2.0, 3.0, 4.0], lambda r: B.setOrdinal(r), "a level is not on the latent's scale"),
            ("dense", _dense_relation, lambda r: B.setDense(r), None),
            ("new_test", _new_test_fresh, lambda r: _new_test(B, r), new_row),
            ("new_observed", None, lambda r: B.setNewObserved(r, r.entities[0], {"u": [1, 2], "v": [1, 7], "y": [0.5, 0.25]}, n_rows=2), new_row),
            ("bias", None, lambda r: B.setBias(r, r.entities[0]), "the score is u.v \\+ mean alone"),
            ("recommend", None, lambda r: B.setRecommend(r, 3), "a relation keeps one ranked list")]


def test_the_option_record(B):
    from bdf_amd import model_options as MO
    rec = MO.OPTION["acquire"]
    assert rec.scope == MO.RELATION and rec.field == "acquire" and rec.one_rank is True and rec.phrase == "acquisition lists (setAcquire)"
    assert rec.trainer == "keeps no moments of scores over draws"
    assert not [p for p in MO._REFUSED_ONLY_AT_BUILD if "acquire" in p]                 # nothing is left to the build-time pass alone
    taken = ("censored", "interval", "background", "alpha_sample", "waic", "lpd", "entity_features", "spike", "nonneg")
    assert not [k for k in taken if MO.refused("acquire", k)[0] or MO.refused(k, "acquire")[0]]


def test_every_row_of_the_table_is_refused_in_both_orders_at_the_setter(B):
    """each option that setAcquire does not go with, set before it and after it: refused at the setter both times, with a message that
    names the relation and both options (and the table's reason)"""
    from bdf_amd import model_options as MO
    phrase = r"acquisition lists \(setAcquire\)"
    seen = []
    for key, values, setter, why in _refused_with(B):
        fresh = (lambda: values(B)) if callable(values) else (lambda: _relation(B, values))
        other = MO.OPTION[key]
        named = re.escape(other.phrase) + ("|" + re.escape(other.has) if other.has else "")
        tail = (", " + why) if why else ""
        r = fresh()
        setter(r)
        with pytest.raises(B.ArgumentError, match=r"Relation plays (has )?(%s): it does not take %s%s\." % (named, phrase, tail)):
            B.setAcquire(r, 3)
        assert r.model.acquire is None
        r = fresh()
        B.setAcquire(r, 3)
        B.RelationData(r)                                    # (an entity learns of its relations here: what its own setters look at)
        with pytest.raises(B.ArgumentError, match=r"Relation plays has %s: .*(%s)" % (phrase, named)) as e:
            setter(r)
        if why:
            assert re.search(why, str(e.value)), (key, str(e.value))
        seen.append(key)
    assert sorted(seen) == sorted(["probit", "logit", "counts", "robust", "weights", "entity_noise", "ordinal", "dense", "new_test", "new_observed",
                                   "bias", "recommend"])
    # relation features: a plain assignment, nothing refuses it before the build-time pass; setAcquire after it is refused at once
    from bdf_amd.relation_data import check_model
    r = _relation(B)
    _features(r)
    with pytest.raises(B.ArgumentError, match=r"Relation plays has features \(relation-level side information\): it does not take " + phrase):
        B.setAcquire(r, 3)
    r = _relation(B)
    B.setAcquire(r, 3)
    _features(r)
    with pytest.raises(B.ArgumentError, match="relation-level side information.*" + phrase):
        check_model(r)


def test_what_it_goes_with_is_taken_in_both_orders(B):
    from bdf_amd.relation_data import check_model
    n = len(BR.listing()[0])
    for setter in (lambda r: B.setCensored(r, np.zeros(n, dtype=np.int8)), lambda r: B.setBinned(r, [-0.5, 0.5]), lambda r: B.setBackground(r, 0.2),
                   lambda r: B.setWaic(r), lambda r: setattr(r.model, "alpha_sample", True), lambda r: B.setSpikeAndSlab(r.entities[0]),
                   lambda r: B.setNonNegative(r.entities[1]), lambda r: setattr(r.entities[0], "F", np.ones((37, 3)))):
        for first in (True, False):
            r = _relation(B)
            B.RelationData(r)
            if first:
                B.setAcquire(r, 5, rule="prob_above", threshold=0.5)
                setter(r)
            else:
                setter(r)
                B.setAcquire(r, 5, rule="prob_above", threshold=0.5)
            check_model(r)
            assert r.model.acquire["k"] == 5


def test_refuses_more_than_one_rank(B):
    from bdf_amd.relation_data import check_model
    rel = _relation(B)
    B.setAcquire(rel, 5)
    check_model(rel, 1)
    with pytest.raises(B.ArgumentError, match=r"Relation plays has acquisition lists \(setAcquire\): one rank only"):
        check_model(rel, 2)


def test_macau_refuses_a_later_relation(B):
    u, v, w = B.Entity("u"), B.Entity("v"), B.Entity("w")
    ids, y, _ = BR.listing()
    r1 = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "plays", [u, v], dims=[37, 29])
    r2 = B.Relation({"u": ids[:, 0], "w": ids[:, 1], "y": y}, "skips", [u, w], dims=[37, 29])
    rd = B.RelationData(r1)
    B.addRelation(rd, r2)
    B.setAcquire(r2, 5)
    with pytest.raises(B.ArgumentError, match=r"skips asks for acquisition lists \(setAcquire\) but is not the first relation"):
        B.macau(rd, num_latent=4, burnin=1, psamples=1, verbose=False)


@pytest.mark.parametrize("who", ["bpmf_vb", "macau_hmc"])
def test_the_other_trainers_refuse_it(B, who):
    from bdf_amd._two_mode import relation_of
    rel = _relation(B)
    B.setAcquire(rel, 5)
    with pytest.raises(B.ArgumentError, match=who + ".*setAcquire"):
        relation_of(B.RelationData(rel), 8, who)


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def test_welford_fold_against_extended_precision_at_a_large_offset():
    """p = 1e6 + N(0, 1) over S draws for 4,000 cells, folded one draw at a time, against np.mean and np.var(ddof = 1) of the same doubles
    in np.longdouble.  The mean to 1e-12 of itself.  The variance to 1e-12 RELATIVE TO ITS CONDITION: the relative condition number
    of a variance is kappa = sqrt(1 + mean^2 / var), 1e6 here, and no fold that keeps the running mean as a double can be closer than
    kappa 2^-53 = 1.1e-10 of the variance (the mean is rounded to an ulp of 1e6 = 1.2e-10, which every delta inherits); the bound is
    1e-12 kappa var = 1e-12 |mean| sd.  A difference of the sums p and p^2 misses it by three orders of magnitude (asserted): its
    error is about 2^-53 mean^2.  Measured here over S = 2, 8, 50, 200: the mean within 1.0e-15 of itself; the variance within 2.0e-16
    of kappa var (1.5e-10 .. 3.4e-10 of the variance itself from S = 8 on: the literal reading "1e-12 of the variance" is out of
    reach of the fold the device runs, and of any other that keeps the mean as a double); the difference of sums 1.4e-9 .. 7.9e-7 of
    kappa var"""
    rng = np.random.default_rng(0)
    for S in (2, 8, 50, 200):
        p = 1e6 + rng.standard_normal((S, 4000))
        mean, M2 = np.zeros(4000), np.zeros(4000)
        for b in range(S):
            mean, M2 = AR.fold_one(p[b], b + 1, mean, M2)
        ext = p.astype(np.longdouble)
        em, ev = ext.mean(axis=0), ext.var(axis=0, ddof=1)
        var = AR.sd_of(M2, S) ** 2
        kappa = np.sqrt(1.0 + em * em / ev)
        err_m, err_v = float(np.max(np.abs(mean - em) / np.abs(em))), float(np.max(np.abs(var - ev) / (kappa * ev)))
        naive = (np.sum(p * p, axis=0) - np.sum(p, axis=0) ** 2 / S) / (S - 1)
        err_n = float(np.max(np.abs(naive - ev) / (kappa * ev)))
        print(f"S={S}: mean {err_m:.1e} of itself, variance {err_v:.1e} of kappa var (of var itself {float(np.max(np.abs(var - ev) / ev)):.1e}); "
              f"difference of sums {err_n:.1e}")
        assert err_m <= 1e-12 and err_v <= 1e-12
        assert err_n > 1e-10
    assert np.isnan(AR.sd_of(np.ones(3), 1)).all() and np.isnan(AR.sd_of(np.ones(3), 0)).all()


def test_restatement_product_is_the_dense_product_and_a_row_subset():
    rng = np.random.default_rng(4)
    draws = [(rng.standard_normal((7, 6)), rng.standard_normal((9, 6))) for _ in range(5)]
    alphas = [0.5, 1.0, 2.0, 4.0, 3.0]
    planes, mag = AR.fold(draws, alphas=alphas, mean_value=0.25, threshold=0.5)
    P = np.stack([U @ V.T for U, V in draws])
    assert np.allclose(planes["mean"], P.mean(axis=0), rtol=1e-13, atol=1e-14) and np.allclose(planes["M2"], P.var(axis=0, ddof=1) * 4, rtol=1e-12)
    from scipy.stats import norm
    exp = sum(norm.cdf(np.sqrt(a) * (p + 0.25 - 0.5)) for a, p in zip(alphas, P))
    assert np.allclose(planes["psum"], exp, rtol=1e-13)
    assert np.allclose(mag, np.max([np.abs(U) @ np.abs(V).T for U, V in draws], axis=0), rtol=1e-14)
    rows0 = [5, 0, 3]
    sub, _ = AR.fold(draws, rows0, alphas, 0.25, 0.5)
    assert all(np.array_equal(sub[k], planes[k][rows0]) for k in planes)
    # the rules
    s = AR.scores_of(planes, 5, "ucb", 0.75, 0.25)
    assert np.allclose(s, P.mean(axis=0) + 0.25 + 0.75 * P.std(axis=0, ddof=1), rtol=1e-12)
    assert np.array_equal(AR.scores_of(planes, 5, "ucb", 0.0, 0.25), planes["mean"] + 0.25)          # kappa = 0: the mean
    assert np.array_equal(AR.scores_of(planes, 5, "sd"), AR.sd_of(planes["M2"], 5))
    assert np.array_equal(AR.scores_of(planes, 5, "prob_above"), planes["psum"] / 5.0)
    assert np.isnan(AR.scores_of(planes, 1, "ucb", 1.0)).all() and np.isnan(AR.scores_of(planes, 1, "sd")).all()
    assert not np.isnan(AR.scores_of(planes, 1, "prob_above")).any() and np.isnan(AR.scores_of(planes, 0, "prob_above")).all()
    items, vals = AR.topk(s, 3)
    g = AR.gathered(planes, 5, items, 0.25)
    assert np.array_equal(g["mean"], np.take_along_axis(planes["mean"] + 0.25, items - 1, axis=1)) and g["prob"].shape == (7, 3)


# ---- csrc/acquire.h on the host ---------------------------------------------------------------------------------------------------
_HOST_SRC = r"""
#include <cstdio>
#include <cstring>
#include <cstdint>
#include "acquire.h"
static void show(double x) { uint64_t b; std::memcpy(&b, &x, 8); std::printf("%016llx\n", (unsigned long long)b); }
int main()
{
    std::printf("%d %d %d %d %d %d %d\n", BDF_ACQ_TN, BDF_ACQ_TM, BDF_ACQ_WN, BDF_ACQ_WM, BDF_ACQ_UCB, BDF_ACQ_SD, BDF_ACQ_PROB);
    int rule;
    double mean, M2, psum, n, kappa, mv, p, alpha, thr;
    while (std::scanf("%d %la %la %la %la %la %la %la %la %la", &rule, &mean, &M2, &psum, &n, &kappa, &mv, &p, &alpha, &thr) == 10) {
        show(bdf_acq_score(rule, mean, M2, psum, n, kappa, mv));
        double a = mean, q = M2;
        bdf_acq_fold(p, n, a, q);
        show(a); show(q);
        show(bdf_acq_prob(p, alpha, mv, thr));
    }
    return 0;
}
"""


def _bits(a):
    return ["%016x" % struct.unpack("<Q", struct.pack("<d", float(x)))[0] for x in np.asarray(a).ravel()]


def test_acquire_header_on_the_host_gives_the_restatements_bits():
    """bdf_acq_score, bdf_acq_fold and bdf_acq_prob compiled for the host, on 600 random cells (three rules; n in 0, 1, 2, 7), against
    scores_of, fold_one and prob_term: the same bits (Phi through the C library's erfc, as math.erfc is)"""
    cxx = [shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")]
    if cxx[0] is None:
        cxx = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "c++"]
    rng = np.random.default_rng(8)
    n_cells = 600
    rule = rng.integers(0, 3, n_cells)
    mean, M2, psum = rng.standard_normal(n_cells) * 3, rng.random(n_cells) * 5, rng.random(n_cells) * 7
    n = rng.choice([0.0, 1.0, 2.0, 7.0], n_cells)
    kappa, mv = rng.integers(0, 9, n_cells) / 4.0 + rng.random(n_cells) * (rng.random(n_cells) < 0.5), rng.standard_normal(n_cells)
    p, root_alpha, thr = rng.standard_normal(n_cells) * 2, np.sqrt(rng.random(n_cells) * 4 + 0.1), rng.standard_normal(n_cells)
    td = tempfile.mkdtemp()
    try:
        open(os.path.join(td, "t.cpp"), "w").write(_HOST_SRC)
        subprocess.run(cxx + ["-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, os.path.join(td, "t.cpp"), "-o", os.path.join(td, "t")], check=True)
        text = "".join("%d %s\n" % (rule[q], " ".join(float(x).hex() for x in (mean[q], M2[q], psum[q], n[q], kappa[q], mv[q], p[q], root_alpha[q], thr[q])))
                       for q in range(n_cells))
        out = subprocess.run([os.path.join(td, "t")], input=text, capture_output=True, text=True, check=True).stdout.split()
    finally:
        shutil.rmtree(td, ignore_errors=True)
    assert [int(x) for x in out[:7]] == [TN, TM, 32, 32, 0, 1, 2]
    got = np.array(out[7:]).reshape(n_cells, 4)
    for q in range(n_cells):
        planes = {"mean": mean[q:q + 1], "M2": M2[q:q + 1], "psum": psum[q:q + 1]}
        s = AR.scores_of(planes, n[q], AR.RULES[rule[q]], kappa[q], mv[q])
        with np.errstate(divide="ignore", invalid="ignore"):
            a, m2 = AR.fold_one(p[q:q + 1], n[q], mean[q:q + 1], M2[q:q + 1])
        # (the restatement's prob_term takes alpha and roots it; the header's takes the root)
        pr = AR.phi(root_alpha[q] * (p[q] + mv[q] - thr[q]))
        exp = _bits(s) + _bits(a) + _bits(m2) + _bits(pr)
        if np.isnan(s[0]):
            assert np.isnan(struct.unpack("<d", struct.pack("<Q", int(got[q, 0], 16)))[0]), q
            exp[0] = got[q, 0]
        if n[q] == 0:
            continue                                         # (the fold is never asked for a draw number 0)
        assert list(got[q]) == exp, (q, rule[q], n[q])


# ---- the resource listing and the bindings ----------------------------------------------------------------------------------------
def test_acquire_kernels_use_no_scratch_and_no_lds():
    """k_acquire.hip: the two instantiations of k_acquire_accum (with and without the psum plane), the slot's alpha, the score plane
    and the gather -- no scratch memory and no LDS in any of them; the accumulate kernel within the 512 registers of a lane at one wave
    per SIMD of its 256-thread workgroup, and the product and three planes (128 registers) leave at least two"""
    res = _resources("k_acquire")
    accum = {k: v for k, v in res.items() if "k_acquire_accumILb" in k}
    assert len(accum) == 2 and len(res) == 5, sorted(res)
    for name in ("k_acquire_alpha", "k_acquire_score", "k_acquire_gather"):
        assert sum(name in k for k in res) == 1, name
    for k, v in res.items():
        assert v["ScratchSize"] == 0 and v["LDS"] == 0, (k, v)
    for k, v in accum.items():
        assert 128 <= v["VGPRs"] <= 256 and v["Occupancy"] >= 2, (k, v)


def test_the_c_abi_is_bound_and_documented(B):
    """bdf.h's new declarations in the ctypes table, in julia/BDFHip.jl and in INTEGRATION.md"""
    h = open(os.path.join(ROOT, "include", "bdf.h")).read()
    jl = open(os.path.join(ROOT, "julia", "BDFHip.jl")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("bdf_acquire_create", "bdf_acquire_destroy", "bdf_acquire_push", "bdf_acquire_flush", "bdf_acquire_topk", "bdf_acquire_copy",
                 "bdf_acquire_set_draws"):
        assert "int " + name + "(" in h and name in B.declared_symbols() and (":" + name) in jl and name in doc, name
    assert sorted(s for s in B.declared_symbols() if s.startswith("bdf_acquire_")) == sorted(re.findall(r"int (bdf_acquire_\w+)\(", h))


def test_tile_constants_are_the_ones_the_gpu_tests_name():
    text = open(os.path.join(CSRC, "acquire.h")).read()
    got = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (BDF_ACQ_\w+) (\d+)", text)}
    assert got["BDF_ACQ_TN"] == TN and got["BDF_ACQ_TM"] == TM and got["BDF_ACQ_WN"] * 2 == TN and got["BDF_ACQ_WM"] * 2 == TM
    from bdf_amd.engine import ACQUIRE_PLANES, ACQUIRE_RULES
    assert ACQUIRE_RULES == {"ucb": got["BDF_ACQ_UCB"], "sd": got["BDF_ACQ_SD"], "prob_above": got["BDF_ACQ_PROB"]}
    assert ACQUIRE_PLANES == {"mean": got["BDF_ACQ_MEAN"], "M2": got["BDF_ACQ_M2"], "psum": got["BDF_ACQ_PSUM"], "score": got["BDF_ACQ_SCORE"]}
