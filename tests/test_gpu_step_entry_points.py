"""The entry points through which the step-by-step path drives the library's own description of the iteration
(bdf_gibbs_step_relations, _rows, _draws, _hyper, _beta) and its two parity hooks (bdf_gibbs_terms, bdf_gibbs_row_prior): what
fill_terms() of csrc/bdf_gibbs.hip hands a row launch for every kind of relation, that the library's buffer rotation and the engine's
stay together step by step, that the hyperprior and the beta step equal the sequences of public entry points they replaced, that
they leave the object's bookkeeping alone, and that bad arguments are refused.  That the step path computes what the native one does
is the business of the both-paths tests; nothing here depends on a kernel's size: 30 x 40 cells at most, D = 3 but where the
hyperprior kernels' three widths are meant.
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


def _engine(B, *rels, **kw):
    rd = B.RelationData()
    for r in rels:
        B.addRelation(rd, r)
    return rd, B.GibbsEngine(rd, kw.pop("num_latent", D), seed=3, **kw)


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
            assert L.bdf_gibbs_step_draws(h, j) == ERR_ARG
            assert L.bdf_gibbs_step_hyper(h, j, 0) == ERR_ARG
            assert L.bdf_gibbs_step_beta(h, j) == ERR_ARG
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


# ---- the hyperprior and the beta step against the sequences of public entry points they replaced ---------------------------------------
NNZ_STEP = 600


def _pair_of_engines(B, monkeypatch, num_latent=D, features=False, spike=False, **kw):
    """two step-by-step engines on the same model with the same seed, one full iteration behind them (so that beta, lambda_beta and
    the hyperprior are no longer their initial values); entity 0 (u) carries the features / the spike-and-slab prior"""
    monkeypatch.setenv("BDF_NO_NATIVE", "1")
    out = []
    for _ in range(2):
        F = np.random.default_rng(9).standard_normal((NU, 5)) if features else None
        u, w = B.Entity("u", F=F), B.Entity("w")
        if spike:
            B.setSpikeAndSlab(u, 2.0, 3.0, 1.5, 0.5)
        rd, eng = _engine(B, _relation(B, "r", u, w, (NU, NW), NNZ_STEP, 1), num_latent=num_latent, **kw)
        assert eng.native is False and eng.ctx_h is not eng.ctx
        eng.sweep(1)
        eng.sync()
        out.append((rd, eng))
    return out


def _rows_of(eng, j, i):
    """iteration i up to and including entity j's rows"""
    eng.ctx.set_sweep(i)
    eng.ctx_h.set_sweep(i)
    eng.update_relations()
    eng.sample_entity(j)
    eng.sync()


def _bits(eng, j, names):
    return {n: getattr(eng.ent[j], n).cpu().numpy().tobytes() for n in names}


def _old_update_prior(eng, j, prepared):
    """GibbsEngine.update_prior (and prepare_prior) as they stood before bdf_gibbs_step_hyper: the public entry points on eng.ctx_h"""
    from bdf_amd._lib import check, lib
    from bdf_amd.engine import _ptr
    L, h, st, Dn = lib(), eng.ctx_h.handle, eng.ent[j], eng.D
    if st.spike is not None:
        sp = st.spike
        check(L.bdf_spike_hyper(h, Dn, st.n_real, _ptr(st.sample), sp["incl_a"], sp["incl_b"], sp["shape"], sp["rate"], st.tag, _ptr(st.spike_state)))
        return
    nu, Tinv = st.nu0, st.WI
    if st.F is not None and eng.full_lambda_u:
        nu += st.numF
    if prepared:
        check(L.bdf_hyper_draws(h, Dn, st.n_real, nu, st.tag, _ptr(st.draws)))
    check(L.bdf_hyper_sums(h, Dn, st.N, _ptr(st.sample), _ptr(st.uhat) if st.F is not None else None, _ptr(st.sumU), _ptr(st.UUt)))
    if st.F is not None and eng.full_lambda_u:
        check(L.bdf_hyper_feature_terms(h, Dn, st.numF, _ptr(st.beta), _ptr(st.WI), _ptr(st.lambda_beta), _ptr(st.Tinv)))
        Tinv = st.Tinv
    check(L.bdf_hyper_sample(h, Dn, st.n_real, _ptr(st.sumU), _ptr(st.UUt), _ptr(st.mu0), st.b0, _ptr(Tinv), nu, st.tag, _ptr(st.mu), _ptr(st.Lambda),
                             _ptr(st.params), _ptr(st.prior_pack), _ptr(st.draws) if prepared else None))


@pytest.mark.parametrize("case", ["plain", "features", "features_wi"])
@pytest.mark.parametrize("num_latent", [3, 17, 33])
def test_hyper_step_equals_the_entry_points_it_replaced(B, monkeypatch, num_latent, case):
    """update_prior(j, i) -- bdf_gibbs_step_hyper -- against bdf_hyper_draws, bdf_hyper_sums, bdf_hyper_feature_terms, bdf_hyper_sample
    on the same context, bit for bit: with the draws prepared (iteration 2) and without (iteration 3), at one D per width of the
    hyperprior kernels, without side information and with it (full_lambda_u or not: nu and Tinv differ)"""
    feats = case != "plain"
    (_, a), (_, b) = _pair_of_engines(B, monkeypatch, num_latent, features=feats, full_lambda_u=case != "features_wi")
    try:
        names = ["mu", "Lambda", "sumU", "UUt", "prior_pack", "params"] + (["Tinv"] if feats else [])
        for i, prepared in ((2, True), (3, False)):
            for eng in (a, b):
                _rows_of(eng, 0, i)
            before = _bits(a, 0, names)
            assert before == _bits(b, 0, names)
            if prepared:
                a.prepare_prior(0, i)
            a.update_prior(0, i)
            _old_update_prior(b, 0, prepared)
            a.sync(), b.sync()
            got, want = _bits(a, 0, names), _bits(b, 0, names)
            for n in names:
                assert got[n] == want[n], (n, i)
            assert all(got[n] != before[n] for n in ("mu", "Lambda", "sumU", "UUt", "prior_pack"))
            if feats and i == 2:      # (T^-1 is made only with full_lambda_u; the first iteration made it from beta = 0)
                assert (got["Tinv"] != before["Tinv"]) == (case == "features")
    finally:
        a.close(), b.close()


def test_hyper_step_of_a_spike_and_slab_entity(B, monkeypatch):
    (_, a), (_, b) = _pair_of_engines(B, monkeypatch, spike=True)
    try:
        for eng in (a, b):
            _rows_of(eng, 0, 2)
        before = _bits(a, 0, ["spike_state"])
        a.prepare_prior(0, 2)                                   # (nothing to prepare: no launch)
        a.update_prior(0, 2)
        _old_update_prior(b, 0, False)
        a.sync(), b.sync()
        assert _bits(a, 0, ["spike_state", "draws"]) == _bits(b, 0, ["spike_state", "draws"])
        assert _bits(a, 0, ["spike_state"]) != before
    finally:
        a.close(), b.close()


@pytest.mark.parametrize("solver", ["direct", "cg"])
def test_beta_step_equals_the_entry_point_it_replaced(B, monkeypatch, solver):
    """update_beta(j) -- bdf_gibbs_step_beta -- against bdf_sample_beta_ranks with the arguments the engine passed, bit for bit"""
    from bdf_amd._lib import check, lib
    from bdf_amd.engine import _ptr
    (rd, a), (_, b) = _pair_of_engines(B, monkeypatch, features=True, compute_ff_size=6500 if solver == "direct" else 0)
    try:
        assert rd.entities[0].use_FF is (solver == "direct")
        names = ["beta", "lambda_beta", "cg_iters"]
        for eng in (a, b):
            _rows_of(eng, 0, 2)
            eng.update_prior(0)
            eng.sync()
        before = _bits(a, 0, names)
        assert before == _bits(b, 0, names)
        a.update_beta(0)
        en, st = b.data.entities[0], b.ent[0]
        check(lib().bdf_sample_beta_ranks(b.ctx.handle, None, st.F.handle, b.D, _ptr(st.sample), _ptr(st.mu), _ptr(st.Lambda), _ptr(st.lambda_beta),
                                          int(en.use_FF), b.tol, 0, int(en.lambda_beta_sample), en.nu, en.mu, st.tag, _ptr(st.beta), None,
                                          _ptr(st.cg_iters)))
        a.sync(), b.sync()
        got = _bits(a, 0, names)
        assert got == _bits(b, 0, names)
        assert got["beta"] != before["beta"] and got["lambda_beta"] != before["lambda_beta"]
        if solver == "cg":
            assert (a.ent[0].cg_iters.cpu().numpy() > 0).all()
        # the entity without features: the call returns and nothing changes
        watch = ["sample", "mu", "Lambda", "beta", "sumU", "UUt"]
        before = _bits(a, 1, watch)
        a.update_beta(1)
        a.sync()
        assert _bits(a, 1, watch) == before and a.ent[1].beta.numel() == 0
    finally:
        a.close(), b.close()


def test_step_entry_points_leave_the_bookkeeping_alone(B):
    """bdf_gibbs_step_draws / _hyper / _beta change neither what bdf_gibbs_recorded reports nor the current buffer -- on the native
    path's object, after an iteration of bdf_gibbs_sweep and before one"""
    from bdf_amd._lib import check, lib
    u, w = B.Entity("u", F=np.random.default_rng(9).standard_normal((NU, 5))), B.Entity("w")
    rd, eng = _engine(B, _relation(B, "r", u, w, (NU, NW), NNZ_STEP, 1))
    L, g = lib(), eng._gibbs

    def books():
        out = []
        for j in range(len(eng.ent)):
            hy, be, cur = C.c_int(-1), C.c_int(-1), C.c_int(-1)
            check(L.bdf_gibbs_recorded(g, j, C.byref(hy), C.byref(be)))
            check(L.bdf_gibbs_current(g, j, C.byref(cur)))
            out.append((hy.value, be.value, cur.value))
        return out

    try:
        assert eng.native
        for want in ([(0, 0, 0), (0, 0, 0)], [(1, 1, 1), (1, 0, 1)]):
            assert books() == want
            for j in range(len(eng.ent)):
                check(L.bdf_gibbs_step_draws(g, j))
                check(L.bdf_gibbs_step_hyper(g, j, 1))
                check(L.bdf_gibbs_step_hyper(g, j, 0))
                check(L.bdf_gibbs_step_beta(g, j))
            eng.sync()
            assert books() == want
            eng.sweep(1)
            eng.sync()
    finally:
        eng.close()
