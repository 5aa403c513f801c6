"""The entry points through which the step-by-step path drives the library's own description of the iteration
(bdf_gibbs_step_relations, bdf_gibbs_step_rows) and its two parity hooks (bdf_gibbs_terms, bdf_gibbs_row_prior): what fill_terms()
of csrc/bdf_gibbs.hip hands a row launch for every kind of relation, that the library's buffer rotation and the engine's stay
together step by step, and that bad arguments are refused.  That the step path computes what the native one does is the business
of the both-paths tests; nothing here depends on a kernel's size: 30 x 40 cells at most, D = 3.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NU, NV, NW, D, NNZ = 30, 12, 40, 3, 400
ALPHA = 2.5


def _cells(n_rows, n_cols, nnz, seed, binary=False):
    """nnz distinct cells of an n_rows x n_cols relation, 1-based, with values"""
    rng = np.random.default_rng(seed)
    cells = rng.choice(n_rows * n_cols, size=nnz, replace=False)
    ids = np.stack([cells // n_cols + 1, cells % n_cols + 1], axis=1).astype(np.int64)
    y = rng.standard_normal(nnz)
    return ids, ((y > 0).astype(np.float64) if binary else y)


def _relation(B, name, a, b, dims, nnz, seed, binary=False):
    ids, y = _cells(dims[0], dims[1], nnz, seed, binary)
    return B.Relation({a.name: ids[:, 0], b.name: ids[:, 1], "y": y}, name, [a, b], alpha=ALPHA, dims=list(dims))


def _engine(B, *rels):
    rd = B.RelationData()
    for r in rels:
        B.addRelation(rd, r)
    return rd, B.GibbsEngine(rd, D, seed=3)


def _single(B, kind):
    u, w = B.Entity("u"), B.Entity("w")
    r = _relation(B, "r", u, w, (NU, NW), NNZ, 1, binary=kind == "probit")
    if kind == "sampled":
        r.model.alpha_sample = True
    elif kind == "probit":
        B.setProbit(r)
    elif kind == "weights":
        B.setWeights(r, 0.5 + np.random.default_rng(2).random(NNZ))
    return _engine(B, r)


def _check_factors(eng, rd, j, terms):
    """factors[k] of every term: the current sample of the entity that is the relation's mode k, NULL behind the last mode"""
    en = rd.entities[j]
    assert len(terms) == len(en.relations)
    for t, r in zip(terms, en.relations):
        want = [eng.ent[eng._entity_index(e)].sample.data_ptr() for e in r.entities]
        got = list(t.factors)
        assert got[:len(want)] == want and all(p is None for p in got[len(want):]), (r.name, got, want)
        assert t.rel == r._dev.handle.value and t.mode == [e is en for e in r.entities].index(True)


@pytest.mark.parametrize("kind", ["fixed", "sampled", "probit", "weights"])
def test_terms_of_one_relation(B, kind):
    rd, eng = _single(B, kind)
    try:
        r, dr = rd.relations[0], eng.rel[0]
        for j in (0, 1):
            terms = eng._terms(j)
            _check_factors(eng, rd, j, terms)
            t = terms[0]
            assert t.mean_value == r.model.mean_value
            if kind == "fixed":
                assert t.alpha == ALPHA == r.model.alpha
                assert t.alpha_dev is None and t.linear_values is None and t.obs_precision is None
            elif kind == "sampled":
                assert t.alpha_dev == dr.alpha_dev.data_ptr() and t.linear_values is None and t.obs_precision is None
            elif kind == "probit":
                assert t.alpha == 1.0 and t.alpha_dev is None and t.obs_precision is None
                assert t.linear_values == dr.linear.data_ptr()
            else:
                assert t.obs_precision == dr.omega.data_ptr() and t.linear_values is None
    finally:
        eng.close()


def test_terms_of_a_dense_and_a_background_relation(B):
    """u takes part in a dense relation (its first term) and in one with background cells, unit weights and a sampled alpha (its
    second): both are folded into u's prior, so the background term reads alpha (1 - c0) from the SECOND slot of bg_alpha_rows.  w
    has the background term alone: the first slot.  The dense term lists no cell: it has no linear_values and no obs_precision, and
    whatever alpha it names no observation reads."""
    u, v, w = B.Entity("u"), B.Entity("v"), B.Entity("w")
    Y = np.random.default_rng(5).standard_normal((NU, NV))
    dense = B.denseRelation(Y, "panel", [u, v], alpha=ALPHA)
    bg = _relation(B, "plays", u, w, (NU, NW), NNZ, 6)
    bg.model.alpha_sample = True
    B.setBackground(bg, 0.25, 0.5)
    rd, eng = _engine(B, dense, bg)
    try:
        names = [en.name for en in rd.entities]
        ju, jv, jw = (names.index(n) for n in "uvw")
        assert [r.name for r in rd.entities[ju].relations] == ["panel", "plays"]
        for j in (ju, jv, jw):
            _check_factors(eng, rd, j, eng._terms(j))
        dr_dense, dr_bg = (r._dev for r in (dense, bg))
        assert dr_dense.nnz == 0 and dr_dense.dense is not None and dr_bg.omega is None
        tu = eng._terms(ju)
        for t in (tu[0], eng._terms(jv)[0]):                    # the dense term, from either side
            assert t.linear_values is None and t.obs_precision is None
            assert t.alpha_dev in (None, dr_dense.alpha_dev.data_ptr())
        assert tu[1].alpha_dev == eng.ent[ju].bg_alpha_rows.data_ptr() + 8
        assert tu[1].linear_values is None and tu[1].obs_precision is None
        tw = eng._terms(jw)
        assert tw[0].alpha_dev == eng.ent[jw].bg_alpha_rows.data_ptr()
        assert tw[0].linear_values is None and tw[0].obs_precision is None
    finally:
        eng.close()


def test_rotation_stays_with_the_engine_step_by_step(B, monkeypatch):
    from bdf_amd._lib import check, lib
    monkeypatch.setenv("BDF_NO_NATIVE", "1")
    rd, eng = _single(B, "sampled")
    try:
        assert eng.native is False and eng.gibbs is None
        for i in (1, 2):
            eng.sweep(i)
        eng.sync()
        for j, st in enumerate(eng.ent):
            cur = C.c_int(-1)
            check(lib().bdf_gibbs_current(eng._gibbs, j, C.byref(cur)))
            assert cur.value == st.cur == 2
            assert np.isfinite(st.host("sample")).all() and np.abs(st.host("sample")).max() > 0
            _check_factors(eng, rd, j, eng._terms(j))
        assert rd.relations[0].model.alpha == float(eng.rel[0].alpha_dev.item()) != ALPHA      # (the host scalar of the reporting steps)
    finally:
        eng.close()


def test_entry_points_refuse_bad_arguments(B):
    from bdf_amd._lib import Term, lib
    rd, eng = _single(B, "fixed")
    try:
        L, g, ERR_ARG = lib(), eng._gibbs, -1
        terms = (Term * 1)()
        mu, Lam, pack, ism = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int(0)
        prior = (C.byref(mu), C.byref(ism), C.byref(Lam), C.byref(pack))
        assert L.bdf_gibbs_step_relations(None) == ERR_ARG
        for h, j in ((None, 0), (g, -1), (g, len(eng.ent))):
            assert L.bdf_gibbs_step_rows(h, j, 0) == ERR_ARG
            assert L.bdf_gibbs_terms(h, j, terms) == ERR_ARG
            assert L.bdf_gibbs_row_prior(h, j, 0, *prior) == ERR_ARG
        # (nothing was enqueued and nothing rotated)
        cur = C.c_int(-1)
        assert L.bdf_gibbs_current(g, 0, C.byref(cur)) == 0 and cur.value == eng.ent[0].cur == 0
        # a plain entity's prior is the draw's own: no fold, and no pack before the first draw
        assert L.bdf_gibbs_row_prior(g, 0, 0, *prior) == 0
        st = eng.ent[0]
        assert (mu.value, ism.value, Lam.value, pack.value) == (st.mu.data_ptr(), 0, st.Lambda.data_ptr(), None)
        assert L.bdf_gibbs_row_prior(g, 0, 1, *prior) == 0 and pack.value == st.prior_pack.data_ptr()
    finally:
        eng.close()
