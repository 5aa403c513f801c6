"""The fold-in of new rows on the host (no GPU): setNewObserved and everything it refuses, the option table's
rows for it in both orders, the closed-form conditional of tests/foldin_restatement.py against 400,000 sampled factors of a new row,
the restatement with an empty known table against newrows_restatement on the same draw, the recorded quality figures against the
computation, the resource listing the build leaves for the kernels of k_foldin.hip (no scratch) and the header's declarations in
the Julia binding."""
import math
import os
import re

import numpy as np
import pytest

import foldin_restatement as FR
import newrows_restatement as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the setter -------------------------------------------------------------------------------------------------------------------
def _relation(B, values=None, n=60, feats=True, modes=2, seed=3):
    rng = np.random.default_rng(seed)
    dims = [9, 7, 4][:modes]
    ids = np.unique(np.stack([rng.integers(1, d + 1, n) for d in dims], axis=1), axis=0)
    y = rng.standard_normal(len(ids)) if values is None else np.resize(np.asarray(values, dtype=np.float64), len(ids))
    names = ["u", "v", "w"][:modes]
    ents = [B.Entity(nm) for nm in names]
    if feats:
        ents[0].F = rng.standard_normal((dims[0], 5))
    table = {nm: ids[:, k] for k, nm in enumerate(names)}
    table["y"] = y
    return B.Relation(table, "ratings", ents, alpha=2.0, dims=dims), ents


def _known(n_new=4):
    return {"u": [1, 2, n_new, 1], "v": [1, 7, 3, 2], "y": [0.5, 0.25, -1.0, 2.0]}


def _cells():
    return {"u": [1, 3], "v": [2, 5], "y": [0.1, float("nan")]}


def test_setter_round_trips_and_clears(B):
    from bdf_amd.relation_data import check_new_rows
    rel, (u, v) = _relation(B)
    assert rel.model.new_observed is None and B.RelationModel().new_observed is None
    # an entity with features: n* is the rows of F_new
    B.setNewRows(u, np.ones((4, 5)))
    assert B.setNewObserved(rel, u, _known()) is None
    m = rel.model.new_observed
    assert m["mode"] == 1 and m["n_rows"] == 4 and m["ids"].dtype == np.int64 and m["ids"].shape == (4, 2) and m["values"][3] == 2.0
    B.setNewObserved(rel, u, _known(), n_rows=4)                      # n_rows may be given when it agrees
    B.setNewTest(rel, u, _cells())
    assert check_new_rows(B.RelationData(rel)) is rel
    B.setNewObserved(rel, u, (np.array([[1.0, 2.0]]), np.array([3.0])))            # ids as whole floats, a table as (ids, values)
    assert rel.model.new_observed["ids"].tolist() == [[1, 2]]
    B.setNewObserved(rel, u, (np.zeros((0, 2), dtype=np.int64), np.zeros(0)))      # an empty table: every row cold
    assert rel.model.new_observed["n_rows"] == 4 and len(rel.model.new_observed["values"]) == 0
    B.setNewObserved(rel, u, None)
    assert rel.model.new_observed is None
    # an entity without features: n* is n_rows, by default the largest new id; setNewTest is taken once setNewObserved names the entity
    plain, (a, b) = _relation(B, feats=False)
    with pytest.raises(B.ArgumentError, match=r"Entity u has no new rows: call setNewRows\(entity, F_new\) before setNewTest\."):
        B.setNewTest(plain, a, _cells())
    B.setNewObserved(plain, a, _known(3))
    assert plain.model.new_observed["n_rows"] == 3
    B.setNewObserved(plain, a, _known(3), n_rows=6)
    assert plain.model.new_observed["n_rows"] == 6
    B.setNewTest(plain, a, {"u": [6, 1], "v": [2, 5], "y": [0.1, float("nan")]})
    assert plain.model.new_test["mode"] == 1 and check_new_rows(B.RelationData(plain)) is plain
    with pytest.raises(B.ArgumentError, match=r"outside 1 \.\.\. 6, the new rows of setNewObserved \(setNewTest\)"):
        B.setNewTest(plain, a, {"u": [7], "v": [2], "y": [0.1]})
    with pytest.raises(B.ArgumentError, match="has no new rows: call setNewRows"):
        B.setNewTest(plain, b, {"u": [1], "v": [1], "y": [0.1]})     # the other entity was not named
    B.setNewObserved(plain, a, (np.zeros((0, 2), dtype=np.int64), np.zeros(0)), n_rows=6)
    assert plain.model.new_observed["n_rows"] == 6
    # the entity in the relation's second column
    B.setNewObserved(plain, None, None)
    B.setNewTest(plain, None, None)
    B.setNewObserved(plain, b, {"u": [9, 1], "v": [2, 1], "y": [0.0, 1.0]})
    assert plain.model.new_observed["mode"] == 2 and plain.model.new_observed["n_rows"] == 2
    # a test cell may also be a known cell
    B.setNewTest(plain, b, {"u": [9], "v": [2], "y": [0.0]})
    assert check_new_rows(B.RelationData(plain)) is plain
    assert "setNewObserved" in B.__dict__ and "fold-in" in B.setNewObserved.__doc__ and "own value in the conditional" in B.setNewObserved.__doc__


def test_setter_refusals(B):
    rel, (u, v) = _relation(B)
    B.setNewRows(u, np.ones((4, 5)))
    with pytest.raises(B.ArgumentError, match="takes an Entity"):
        B.setNewObserved(rel, "u", _known())
    with pytest.raises(B.ArgumentError, match="has no entity"):
        B.setNewObserved(rel, B.Entity("z"), _known())
    for bad, what in (({"u": [5], "v": [1], "y": [0.0]}, r"outside 1 \.\.\. 4, the rows of F_new"), ({"u": [0], "v": [1], "y": [0.0]}, r"outside 1 \.\.\. 4"),
                      ({"u": [1], "v": [8], "y": [0.0]}, r"outside 1 \.\.\. 7"), ({"u": [1], "v": [0], "y": [0.0]}, r"outside 1 \.\.\. 7"),
                      ({"u": [1.5], "v": [1], "y": [0.0]}, "must be integers"), ({"u": [1], "v": [1], "y": [float("inf")]}, "must be finite"),
                      ({"u": [1], "v": [1], "y": [float("nan")]}, "must be finite"), ({"u": [1], "y": [0.0]}, "two id columns"),
                      ({"u": [1, 2, 1], "v": [3, 3, 3], "y": [0.0, 1.0, 2.0]}, "listed twice")):
        with pytest.raises(B.ArgumentError, match=what):
            B.setNewObserved(rel, u, bad)
    with pytest.raises(B.ArgumentError, match="n_rows is 5 but F_new of u has 4 rows"):
        B.setNewObserved(rel, u, _known(), n_rows=5)
    assert rel.model.new_observed is None                            # a refused call changes nothing
    plain, (a, b) = _relation(B, feats=False)
    with pytest.raises(B.ArgumentError, match="needs n_rows"):
        B.setNewObserved(plain, a, (np.zeros((0, 2), dtype=np.int64), np.zeros(0)))
    for n_rows in (0, -1, 2.5, True):
        with pytest.raises(B.ArgumentError, match="positive integer"):
            B.setNewObserved(plain, a, _known(), n_rows=n_rows)
    with pytest.raises(B.ArgumentError, match=r"outside 1 \.\.\. 3, n_rows"):
        B.setNewObserved(plain, a, _known(4), n_rows=3)
    # features but no setNewRows: the new rows' prior mean would leave beta out
    rf, (fu, fv) = _relation(B)
    with pytest.raises(B.ArgumentError, match=r"Entity u has features but no new rows: call setNewRows\(entity, F_new\) before setNewObserved"):
        B.setNewObserved(rf, fu, _known())
    B.setNewObserved(rf, fv, {"u": [9, 1], "v": [2, 1], "y": [0.0, 1.0]})      # (the other entity has none: taken)
    assert rf.model.new_observed["mode"] == 2
    r3, ents = _relation(B, modes=3, feats=False)
    with pytest.raises(B.ArgumentError, match="has 3 modes"):
        B.setNewObserved(r3, ents[0], {"u": [1], "v": [1], "w": [1], "y": [0.0]})


def _setters(B):
    """(option key, the relation's values it needs, its setter on (relation, first entity)) of everything setNewObserved refuses"""
    ones = lambda r: np.ones(r.data.nnz())
    return [("probit", [0.0, 1.0], lambda r, a: B.setProbit(r)), ("censored", None, lambda r, a: B.setCensored(r, np.zeros(r.data.nnz(), dtype=np.int8))),
            ("ordinal", [1.0, 2.0, 3.0, 4.0], lambda r, a: B.setOrdinal(r)), ("interval", None, lambda r, a: B.setBinned(r, [-0.5, 0.5])),
            ("robust", None, lambda r, a: B.setRobust(r)), ("weights", None, lambda r, a: B.setWeights(r, ones(r))),
            ("entity_noise", None, lambda r, a: B.setEntityNoise(r, a)), ("logit", [0.0, 1.0], lambda r, a: B.setLogit(r)),
            ("counts", [0.0, 3.0, 1.0], lambda r, a: B.setCounts(r, 2)), ("background", None, lambda r, a: B.setBackground(r, 0.1)),
            ("dense", "dense", lambda r, a: B.setDense(r)), ("bias", None, lambda r, a: B.setBias(r, a)),
            ("recommend", None, lambda r, a: B.setRecommend(r, 3)), ("spike", None, lambda r, a: B.setSpikeAndSlab(a)),
            ("nonneg", None, lambda r, a: B.setNonNegative(a))]


def _dense_relation(B):
    rng = np.random.default_rng(1)
    i, j = np.meshgrid(np.arange(1, 10), np.arange(1, 8), indexing="ij")
    ents = [B.Entity("u"), B.Entity("v")]
    return B.Relation({"u": i.ravel(), "v": j.ravel(), "y": rng.standard_normal(63)}, "ratings", ents, alpha=2.0, dims=[9, 7]), ents


def test_the_option_table_refuses_in_both_orders_at_the_setter(B):
    """every option the fold-in does not go with, set before setNewObserved and after it: refused at the setter both times, with a reason,
    and nothing of it is left to the build-time pass; what it does go with -- a sampled alpha, features of the entity, the test cells"""
    from bdf_amd import model_options as MO
    rec = MO.OPTION["new_observed"]
    assert rec.scope == MO.RELATION and rec.field == "new_observed" and rec.one_rank is True and "setNewObserved" in rec.phrase
    assert not [p for p in MO._REFUSED_ONLY_AT_BUILD if "new_observed" in p]
    refused = sorted(k for k in MO.OPTION if MO.refused("new_observed", k)[0])
    assert refused == sorted(MO.NOISE + ("background", "dense", "bias", "recommend", "features", "spike", "nonneg"))
    for k in refused:
        assert MO.refused("new_observed", k)[1] and MO.refused(k, "new_observed")[1]      # a reason in both orders
    for key, values, setter in _setters(B):
        def fresh():
            if values == "dense":
                return _dense_relation(B)
            return _relation(B, values=values, feats=False)
        r, (a, b) = fresh()
        setter(r, a)
        with pytest.raises(B.ArgumentError, match=r"does not take known cells of new rows \(setNewObserved\)|which rules out known cells of new rows"):
            B.setNewObserved(r, a, _known(), n_rows=4)
        assert r.model.new_observed is None
        r, (a, b) = fresh()
        B.setNewObserved(r, a, _known(), n_rows=4)
        B.RelationData(r)                                            # (an entity learns of its relations here: what its own setters look at)
        with pytest.raises(B.ArgumentError, match=r"has known cells of new rows \(setNewObserved\)"):
            setter(r, a)
    # relation features
    rf, (a, b) = _relation(B, feats=False)
    rf.F = np.ones((rf.data.nnz(), 2))
    with pytest.raises(B.ArgumentError, match="relation-level side information"):
        B.setNewObserved(rf, a, _known(), n_rows=4)
    # taken: alpha sampled, an entity with features and new rows, the other entity's features
    r, (a, b) = _relation(B)
    r.model.alpha_sample = True
    B.setNewRows(a, np.ones((4, 5)))
    b.F = np.ones((7, 2))
    B.setNewObserved(r, a, _known())
    B.setNewTest(r, a, _cells())
    assert r.model.new_observed["n_rows"] == 4


def test_macau_time_checks(B):
    """what is looked at again when macau() runs: a relation that is not the first, more than one rank, a model changed behind the
    setter's back, an F_new whose rows no longer hold the table, test cells of another entity"""
    from bdf_amd.relation_data import check_new_rows
    rel, (u, v) = _relation(B)
    B.setNewRows(u, np.ones((4, 5)))
    B.setNewObserved(rel, u, _known())
    B.setNewTest(rel, u, _cells())
    rd = B.RelationData(rel)
    assert check_new_rows(rd) is rel
    with pytest.raises(B.ArgumentError, match=r"known cells of new rows \(setNewObserved\): one rank only"):
        check_new_rows(rd, world=2)
    second = B.Relation({"u": [1, 2], "v": [1, 2], "y": [0.0, 1.0]}, "second", [u, v], dims=[9, 7])
    second.model.new_observed = dict(rel.model.new_observed)
    rd2 = B.RelationData(rel)
    B.addRelation(rd2, second)
    with pytest.raises(B.ArgumentError, match=r"\(setNewObserved\) but is not the first relation"):
        check_new_rows(rd2)
    B.setNewRows(u, np.ones((3, 5)))                                # fewer new rows than the table addresses
    with pytest.raises(B.ArgumentError, match=r"outside 1 \.\.\. 3, the rows of F_new \(setNewObserved\)"):
        check_new_rows(rd)
    B.setNewRows(u, np.ones((4, 5)))
    rel.model.robust = {"nu": 4.0}                                  # (behind the setter's back)
    with pytest.raises(B.ArgumentError, match="setRobust"):
        check_new_rows(rd)
    rel.model.robust = None
    rel.model.new_test = dict(rel.model.new_test, mode=2)
    with pytest.raises(B.ArgumentError, match="another entity's"):
        check_new_rows(rd)
    # without setNewTest there is nothing to predict: the known cells are checked, no relation comes back
    rel.model.new_test = None
    assert check_new_rows(rd) is None


# ---- the conditional --------------------------------------------------------------------------------------------------------------
def test_the_closed_form_is_the_marginal_over_the_conditioned_factor():
    """For one fixed draw (mu, Lambda, V, alpha), two new rows with three and one known cells and six cells to predict: 400,000 factors
    u* ~ N(uhat_i, P_i^-1) (seeded).  The mean and the variance of mean_value + u* . v over them against the restatement's m and q,
    and the variance of a value with its noise against q + 1 / alpha: each within four Monte-Carlo standard errors (of a mean:
    sd / sqrt n; of a variance of Gaussian values: var sqrt(2 / (n - 1))) -- section 24's check.  And uhat_i, P_i are the conditional
    that Bayes' rule gives: the posterior of u under the prior N(mu_i, Lambda^-1) and the known cells' Gaussian likelihood, checked
    through its normal equations."""
    rng = np.random.default_rng(12)
    D, M, n = 5, 8, 400_000
    A = rng.standard_normal((D, D))
    Lam = A @ A.T / D + np.eye(D)
    mu_rows, V = rng.standard_normal((2, D)) * 0.3, rng.standard_normal((M, D))
    alpha, mean = 3.0, 0.25
    kid, ky = np.array([[1, 2], [1, 5], [2, 7], [1, 8]]), np.array([0.4, -1.1, 0.9, 0.2])
    ids = np.array([[1, 1], [1, 4], [2, 2], [2, 6], [1, 2], [2, 5]])          # (1, 2) is also a known cell
    P, b = FR.systems(Lam, mu_rows, V, alpha, kid, ky, mean)
    uh, m, q = FR.solve(P, b, ids, V, mean)
    for i in range(2):
        at = kid[:, 0] == i + 1
        Vk, r = V[kid[at, 1] - 1], ky[at] - mean
        grad = Lam @ (uh[i] - mu_rows[i]) - alpha * Vk.T @ (r - Vk @ uh[i])       # the log posterior's gradient at its mode
        assert np.abs(grad).max() <= 1e-12 and np.allclose(P[i], Lam + alpha * Vk.T @ Vk, rtol=1e-14)
    worst = 0.0
    for k, (i, j) in enumerate(ids - 1):
        Lc = np.linalg.cholesky(np.linalg.inv(P[i]))
        u = uh[i][None, :] + rng.standard_normal((n, D)) @ Lc.T
        f = mean + u @ V[j]
        y = f + rng.standard_normal(n) / math.sqrt(alpha)
        errs = (abs(f.mean() - m[k]) / math.sqrt(q[k] / n), abs(f.var(ddof=1) - q[k]) / (q[k] * math.sqrt(2.0 / (n - 1))),
                abs(y.var(ddof=1) - (q[k] + 1.0 / alpha)) / ((q[k] + 1.0 / alpha) * math.sqrt(2.0 / (n - 1))))
        worst = max(worst, *errs)
        assert max(errs) <= 4.0, (k, errs)
    print(f"conditional against 400,000 sampled factors: worst deviation {worst:.2f} Monte-Carlo standard errors (asserted: 4)")


def test_an_empty_known_table_is_the_cold_row():
    """no known cell: P_i = Lambda, uhat_i = mu_i, and (m, q) are newrows_restatement's on the same draw"""
    rng = np.random.default_rng(2)
    D, numF, M, n_new = 6, 3, 9, 4
    A = rng.standard_normal((D, D))
    Lam = A @ A.T / D + np.eye(D)
    mu, beta, V, F = rng.standard_normal(D), rng.standard_normal((numF, D)), rng.standard_normal((M, D)), rng.standard_normal((n_new, numF))
    ids = np.stack([rng.integers(1, n_new + 1, 20), rng.integers(1, M + 1, 20)], axis=1)
    mu_rows = NR.uhat(mu, beta, F)
    uh, m, q = FR.cells(Lam, mu_rows, V, 2.0, np.zeros((0, 2), dtype=np.int64), np.zeros(0), ids, 0.3)
    m0, q0 = NR.cells(ids, mu_rows, V, NR.quad(Lam, V), 0.3)
    assert np.allclose(uh, mu_rows, rtol=1e-12, atol=1e-14) and np.allclose(m, m0, rtol=1e-12, atol=1e-14) and np.allclose(q, q0, rtol=1e-12)


def test_split_known_takes_k_cells_per_row():
    sh, train, (kid, ky), (tid, ty) = FR.quality_data()
    _, _, _, new = NR.planted(**sh)
    assert len(ky) + len(ty) == len(new[1]) and np.all(np.bincount(kid[:, 0])[1:] == FR.QUALITY_KNOWN) and len(np.unique(kid[:, 0])) == sh["n_new"]
    both = np.concatenate([kid, tid])
    assert len(np.unique(both, axis=0)) == len(both)
    again = FR.quality_data()
    assert np.array_equal(again[2][0], kid) and np.array_equal(again[3][1], ty)


def test_quality_figures_are_the_recorded_ones():
    """the first of the five recorded CPU chains recomputed; and the known cells matter: every recorded ratio is below a quarter of
    the cold chain's, which predicts the new rows at the prior mean"""
    sh, train, known, test = FR.quality_data()
    g = FR.gibbs(train, known, test, sh["n_train"], sh["M"], sh["D"], NR.QUALITY_ALPHA, *NR.QUALITY_ITERS, NR.QUALITY_SEEDS[0])
    assert abs(g["ratio"] - FR.QUALITY_CPU_RATIOS[0]) <= 5e-6 and abs(g["coverage"] - FR.QUALITY_CPU_COVERAGE[0]) <= 5e-6
    assert len(FR.QUALITY_CPU_RATIOS) == len(FR.QUALITY_CPU_COVERAGE) == len(NR.QUALITY_SEEDS) == 5
    assert max(FR.QUALITY_CPU_RATIOS) < 0.25 * FR.QUALITY_CPU_COLD_RATIO and 0.85 < min(FR.QUALITY_CPU_COVERAGE) and max(FR.QUALITY_CPU_COVERAGE) < 0.95


# ---- the resource listing and the bindings ----------------------------------------------------------------------------------------
def _resources(unit):
    path = os.path.join(ROOT, "bayesiandatafusion.jl_amd", "csrc", unit + ".o.res")
    assert os.path.exists(path), "no csrc/%s.o.res: build with __graft_entry__.build() (make)" % unit
    res, name = {}, None
    for line in open(path):
        mt = re.search(r"remark: \s*(Function Name|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
        if not mt:
            continue
        if mt.group(1) == "Function Name":
            name = mt.group(2).replace("_ZN12_GLOBAL__N_1", "")
            res[name] = {}
        elif name is not None:
            res[name][mt.group(1).split(" ")[0]] = int(mt.group(2))
    return res


def test_foldin_kernels_use_no_scratch():
    """k_foldin.hip: the three instantiations of k_foldin_cells (DP = 16, 32, 64) and the gather of a chunk's prior means -- no scratch
    memory in any of them (the one-wave factorisation by its compile-time recursion, the substitution likewise); LDS: the packed
    factor with its 64 parking slots, 1 / p, uhat and the flag of a bad pivot.  And the fold's sibling in k_newrows.hip"""
    res = _resources("k_foldin")
    cells = {k: v for k, v in res.items() if "k_foldin_cellsI" in k}
    assert len(cells) == 3 and sum("k_foldin_mu" in k for k in res) == 1 and len(res) == 4, sorted(res)
    for k, v in res.items():
        assert v["ScratchSize"] == 0, (k, v)
    for k, v in cells.items():
        dp = int(re.search(r"cellsILi(\d+)E", k).group(1))
        assert v["LDS"] == (dp * (dp + 1) // 2 + 64 + 2 * dp + 1) * 8 and v["Occupancy"] >= 1 and v["VGPRs"] <= 256, (k, v)
    sib = [v for k, v in _resources("k_newrows").items() if "k_newrows_cells" in k]
    assert len(sib) == 1 and sib[0]["ScratchSize"] == 0 and sib[0]["LDS"] == 256 and sib[0]["Occupancy"] >= 4


def test_the_c_abi_is_bound_and_documented(B):
    """bdf.h's new declarations in the ctypes table, in julia/BDFHip.jl and in INTEGRATION.md"""
    h = open(os.path.join(ROOT, "include", "bdf.h")).read()
    jl = open(os.path.join(ROOT, "julia", "BDFHip.jl")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("bdf_foldin_cells", "bdf_foldin_solve", "bdf_newrows_update_cells"):
        assert "int " + name + "(" in h and name in B.declared_symbols() and (":" + name) in jl and name in doc, name
