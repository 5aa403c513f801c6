"""The spike-and-slab prior of an entity's rows on the GPU: the row launch (k_rows_ss) and the hyper step
against the restatement (tests/spike_restatement.py), whole macau() iterations against the restated chain on both iteration
paths, the Gaussian chain untouched by a spike engine in the same process, the C ABI's errors and a planted run."""
import ctypes as C
import os
import textwrap

import numpy as np
import pytest

from both_paths import child
import spike_restatement as SR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


@pytest.fixture(scope="module")
def sctx(B):
    """a context of this module's own (the session's seed): its item size is 64 observations, so that the planted rows of 65 and
    300 observations are split and finished by the last wave to arrive"""
    c = B.Context(seed=SR.ROW_SEED)
    c.set_item_size(64)
    yield c
    c.close()


# ---- (a) the row launch ---------------------------------------------------------------------------------------------------------
def _launch(B, ctx, case, D, mode, weights="own", general=False, decoy=False):
    """-> (out, out of a rerun, P, c, z, U) of the case's launch; weights: "own" (the case's) or None (dropped); general: the
    general gather forced (bdf_ctx_set_gather); decoy: alpha through alpha_dev with another scalar in its place"""
    from bdf_amd._lib import Term, check, lib
    N, dims = case["N"], case["dims"]
    drs, keep = [], []
    terms = (Term * len(case["rels"]))()
    ft = [ctx.tensor(f) for f in case["facs"]]
    for t, (ids, vals, w, alpha) in enumerate(case["rels"]):
        dr = B.DeviceRelation(ctx, B.IndexedDF((ids, vals), dims))
        drs.append(dr)
        terms[t].rel, terms[t].mode, terms[t].alpha, terms[t].mean_value = dr.handle, mode, alpha, float(np.mean(vals))
        if decoy:
            a_t = ctx.tensor([alpha])
            keep.append(a_t)
            terms[t].alpha, terms[t].alpha_dev = 1e6, a_t.data_ptr()
        if w is not None and weights == "own":
            w_t = ctx.tensor(w)
            keep.append(w_t)
            terms[t].obs_precision = w_t.data_ptr()
        for k, f in enumerate(ft):
            terms[t].factors[k] = f.data_ptr() if k != mode else None
    nt = len(case["rels"])
    ctx.set_sweep(case["sweep"])
    ctx.set_gather(1 if general else 0)
    st_t, u_t = ctx.tensor(case["state"].reshape(-1)), ctx.tensor(case["u_current"])
    Lam_t, mu_t = ctx.tensor(np.diag(case["state"][1])), ctx.zeros(D)
    P_t, c_t, z_t = ctx.zeros(N, D, D), ctx.zeros(N, D), ctx.zeros(N, D)
    check(lib().bdf_row_system(ctx.handle, D, N, nt, terms, _p(mu_t), 0, _p(Lam_t), _p(P_t), _p(c_t)))
    check(lib().bdf_normals(ctx.handle, SR.P_ROW, SR.ROW_TAG, 0, N, D, _p(z_t)))
    outs = []
    for rep in range(2):
        out_t = ctx.tensor(np.full((N, D), np.nan))
        check(lib().bdf_sample_rows_spike(ctx.handle, D, N, nt, terms, _p(st_t), _p(u_t), SR.ROW_TAG, 0, 1, _p(out_t)))
        ctx.sync()
        outs.append(out_t.cpu().numpy())
    U = np.zeros((N, D))
    w4 = (C.c_uint32 * 4)()
    for i in range(N):
        for d in range(D):
            check(lib().bdf_philox(ctx.handle, SR.P_SPIKE, SR.ROW_TAG, i, d, w4))
            U[i, d] = SR._u01(w4[0], w4[1])
    assert ctx.rows_unfinished() == 0
    ctx.set_gather(0)
    got = (outs[0], outs[1], P_t.cpu().numpy(), c_t.cpu().numpy(), z_t.cpu().numpy(), U)
    for dr in drs:
        dr.close()
    return got


@pytest.mark.parametrize("D,n_modes,mode,variant", SR.row_cases())
def test_row_launch_matches_the_restatement(B, sctx, D, n_modes, mode, variant):
    """The device's own P, c (bdf_row_system with Lambda = diag tau, mu = 0), normals and Philox blocks through the restated sweep:
    the same inclusion pattern (no decision of the restatement nearer a tie than 1e-9), excluded loadings exactly +0.0, included
    ones within 1e-9 (1 + |ref|); a rerun gives the same bits.  No case has needed the extended-precision fallback: where one
    does, the device's error may be 4 x the float64 restatement's own error against np.longdouble + 1e-12."""
    case = SR.row_case(D, n_modes, mode, variant)
    out, again, P, c, z, U = _launch(B, sctx, case, D, mode, decoy=variant == "alpha_dev")
    assert np.all(np.isfinite(out)) and np.array_equal(out, again) and np.array_equal(np.signbit(out), np.signbit(again))
    np.testing.assert_allclose(U, SR.uniforms(SR.ROW_SEED, case["sweep"], SR.ROW_TAG, case["N"], D), rtol=0, atol=0)
    ref, margin = SR.row_case_reference(case, D, mode, P, c, z, U)
    print(f"spike rows D={D} modes={n_modes} mode={mode} {variant}: near-tie margin {margin:.3e}, "
          f"max |device - ref| / (1 + |ref|) {np.max(np.abs(out - ref) / (1 + np.abs(ref))):.3e}, zeros {np.mean(ref == 0):.2f}")
    assert margin >= 1e-9
    assert np.array_equal(out != 0, ref != 0)
    assert not np.any(np.signbit(out[ref == 0]))                        # an excluded loading is +0.0
    assert np.any(ref == 0) and np.any(ref != 0)
    err = np.abs(out - ref)
    bad = err > 1e-9 * (1 + np.abs(ref))
    if np.any(bad):
        ext, _ = SR.row_case_reference(case, D, mode, P, c, z, U, dtype=np.longdouble)
        own = np.abs(ref - ext).astype(np.float64)
        assert np.all(np.abs(out - ext).astype(np.float64)[bad] <= 4 * own[bad] + 1e-12), (D, n_modes, mode, variant)
    if variant == "unit":
        # unit weights are no weights: the bits of the unweighted launch on the same (general) gather
        plain, _, _, _, _, _ = _launch(B, sctx, case, D, mode, weights=None, general=True)
        assert np.array_equal(out, plain)


# ---- (b) the hyper step ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 63, 64, 65, 1003])
@pytest.mark.parametrize("D", [1, 7, 32, 64])
def test_hyper_step_matches_the_restatement(B, sctx, D, N):
    from bdf_amd._lib import check, lib
    rng = np.random.default_rng(3000 + 70 * D + N)
    S = rng.standard_normal((N, D)) * (rng.random((N, D)) < rng.random(D)[None, :])
    if D > 1:
        S[:, 0], S[:, 1] = 0.0, rng.standard_normal(N) + 3.0            # a column that is all zero and one with no zero
    else:
        S[:, 0] = 0.0 if N % 2 else rng.standard_normal(N) + 3.0        # (one column: all zero at odd N, no zero at even N)
    n = np.count_nonzero(S, axis=0)
    S_t = sctx.tensor(S)
    sweep, tag = 40 + D, 9
    sctx.set_sweep(sweep)
    shape, rate, b = 1.5, 0.7, 2.0
    worst = 0.0
    pinned = np.zeros(D, dtype=bool)
    for a in (1.0, 2.0):                                                # the second draw: incl_a changed
        got = []
        for rep in range(2):
            st_t = sctx.tensor(np.full(4 * D, np.nan))
            check(lib().bdf_spike_hyper(sctx.handle, D, N, _p(S_t), a, b, shape, rate, tag, _p(st_t)))
            sctx.sync()
            got.append(st_t.cpu().numpy().reshape(4, D))
        assert np.array_equal(got[0], got[1])                           # bit for bit across reruns
        ref = SR.hyper_draw(S, a, b, shape, rate, SR.ROW_SEED, sweep, tag)
        worst = max(worst, float(np.max(np.abs(got[0] - ref) / np.maximum(np.abs(ref), 1e-300))))
        np.testing.assert_allclose(got[0], ref, rtol=1e-12, atol=1e-300)
        # n_d is recovered exactly: a count off by one draws pi from another Gamma pair -- somewhere else in one of the two draws
        q = np.sum(S * S, axis=0)
        for dn in (-1, 1):
            nn = np.clip(n + dn, 0, N)
            other = SR.hyper_draw_nq(nn, q, N, a, b, shape, rate, SR.ROW_SEED, sweep, tag)
            pinned |= (np.abs(other[0] - got[0][0]) > 1e-6 * got[0][0]) | (nn == n)
    assert np.all(pinned)
    assert (0 in n and N in n) if D > 1 else n[0] == (0 if N % 2 else N)
    print(f"spike hyper D={D} N={N}: max rel. error {worst:.3e}")


# ---- (c) whole iterations -------------------------------------------------------------------------------------------------------
CHILD = textwrap.dedent('''
    import sys
    import numpy as np
    sys.path.insert(0, %r); sys.path.insert(0, %r)
    import bdf_amd as B
    import spike_restatement as SR
    out, d = sys.argv[1], {}
    for name in SR.CHAIN_MODELS:
        dims, rels, spike, feats, n_test = SR.chain_model(name)
        feats = feats or [None] * len(dims)
        ents = [B.Entity("e%%d" %% k, F=feats[k]) for k in range(len(dims))]
        rd = B.RelationData()
        for ri, r in enumerate(rels):
            table = {"e%%d" %% k: r["ids"][:, m] for m, k in enumerate(r["entities"])}
            table["y"] = r["values"]
            rel = B.Relation(table, "r%%d" %% ri, [ents[k] for k in r["entities"]], alpha=r["alpha"], dims=[dims[k] for k in r["entities"]])
            rel.model.alpha_sample = bool(r["alpha_sample"])
            if ri == 0:
                B.assignToTest(rel, np.arange(1, n_test + 1))
            B.addRelation(rd, rel)
        for j, prm in spike.items():
            B.setSpikeAndSlab(ents[j], *prm)
        res = B.macau(rd, num_latent=SR.CHAIN_D, burnin=3, psamples=3, verbose=False, seed=SR.CHAIN_SEED)
        key = name + "_"
        d[key + "native"], d[key + "pred"] = np.array(int(rd._engine.native)), res["predictions"]["pred"].to_numpy()
        d[key + "alpha"] = np.array([r.model.alpha for r in rd.relations])
        d[key + "order"] = np.array([ents.index(e) for e in rd.entities])
        assert sorted(res["spike"]) == sorted(ents[j].name for j in spike)
        for k, en in enumerate(ents):
            d[key + "S%%d" %% k] = en.model.sample.T
            if k in spike:
                for f, v in res["spike"][en.name].items():
                    d[key + "%%s%%d" %% (f, k)] = v
                d[key + "state%%d" %% k] = en.model._dev.spike_state.cpu().numpy()
            else:
                d[key + "mu%%d" %% k], d[key + "Lam%%d" %% k] = en.model.mu, en.model.Lambda
        rd._engine.close()
    np.savez(out, **d)
''') % (ROOT, os.path.join(ROOT, "tests"))


@pytest.fixture(scope="module")
def chains():
    """3 + 3 iterations of every model of SR.CHAIN_MODELS on the native and on the step-by-step path: one child process per path"""
    return child(CHILD, no_native=False), child(CHILD, no_native=True)


@pytest.mark.parametrize("name", SR.CHAIN_MODELS)
def test_whole_iterations_match_the_restated_chain_on_both_paths(chains, name):
    dims, rels, spike, feats, n_test = SR.chain_model(name)
    key = name + "_"
    nat, step = ({k[len(key):]: v for k, v in ch.items() if k.startswith(key)} for ch in chains)
    assert nat["native"] == 1 and step["native"] == 0
    assert sorted(nat) == sorted(step)
    for k in nat:
        if k != "native":
            assert np.array_equal(nat[k], step[k]), k       # the two paths enqueue the same launches: the same bits
    assert np.array_equal(nat["order"], np.arange(len(dims)))
    train = [dict(r, ids=r["ids"][n_test:], values=r["values"][n_test:]) if i == 0 else r for i, r in enumerate(rels)]
    ref = SR.run_chain(train, dims, SR.CHAIN_D, SR.CHAIN_SEED, 6, spike, feats=feats, burnin=3, test_ids=rels[0]["ids"][:n_test])
    assert ref["margin"] >= 1e-9
    tol = dict(rtol=1e-9, atol=1e-6)
    np.testing.assert_allclose(nat["alpha"], ref["alpha"], **tol)
    assert bool(np.any(nat["alpha"] != 2.5)) == (name == "alpha")
    for k in range(len(dims)):
        np.testing.assert_allclose(nat["S%d" % k], ref["S"][k], err_msg="sample of entity %d" % k, **tol)
        if k in spike:
            assert np.array_equal(nat["S%d" % k] != 0, ref["S"][k] != 0)
            np.testing.assert_allclose(nat["state%d" % k].reshape(4, -1), ref["state"][k], **tol)
            for f, v in ref["spike"][k].items():
                np.testing.assert_allclose(nat["%s%d" % (f, k)], v, err_msg=f, **tol)
            assert np.any(ref["S"][k] == 0)
        else:
            np.testing.assert_allclose(nat["mu%d" % k], ref["mu"][k], **tol)
            np.testing.assert_allclose(nat["Lam%d" % k], ref["Lam"][k], **tol)
    np.testing.assert_allclose(nat["pred"], ref["pred"], **tol)


# ---- (d) nothing else moved -----------------------------------------------------------------------------------------------------
def test_gaussian_chain_is_untouched_by_a_spike_engine_in_the_process(B):
    ids, y, n_test = SR.planted(seed=5, N1=120, N2=60)
    n = len(y)

    def gaussian():
        rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "g", [B.Entity("u"), B.Entity("v")], dims=[120, 60])
        B.assignToTest(rel, np.arange(n - n_test + 1, n + 1))
        rd = B.RelationData(rel)
        res = B.macau(rd, num_latent=16, burnin=2, psamples=2, verbose=False, seed=17)
        assert "spike" not in res
        out = [en.model.sample.copy() for en in rd.entities] + [res["predictions"]["pred"].to_numpy().copy()]
        rd._engine.close()
        return out

    alone = gaussian()
    ents = [B.Entity("u"), B.Entity("v")]
    rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "s", ents, dims=[120, 60])
    B.assignToTest(rel, np.arange(n - n_test + 1, n + 1))
    B.setSpikeAndSlab(ents[1])
    rds = B.RelationData(rel)
    res = B.macau(rds, num_latent=16, burnin=1, psamples=1, verbose=False, seed=17)
    assert res["spike"]["v"]["row_inclusion"].shape == (60, 16)
    assert B.toStr(ents[1]).endswith("]") and " on:" in B.toStr(ents[1]) and " on:" not in B.toStr(ents[0])
    beside = gaussian()                                     # the spike engine is alive
    for a, b in zip(alone, beside):
        assert np.array_equal(a, b)
    rds._engine.close()


# ---- (e) errors through the C ABI -----------------------------------------------------------------------------------------------
def test_spike_c_abi_errors(B, sctx):
    from bdf_amd._lib import Term, lib
    D, mode = 5, 0
    case = SR.row_case(D, 2, mode, "plain")
    ids, vals, _, alpha = case["rels"][0]
    dr = B.DeviceRelation(sctx, B.IndexedDF((ids, vals), case["dims"]))
    ft = [sctx.tensor(f) for f in case["facs"]]
    terms = (Term * 1)()
    terms[0].rel, terms[0].mode, terms[0].alpha, terms[0].mean_value = dr.handle, mode, alpha, 0.0
    terms[0].factors[1] = ft[1].data_ptr()
    N = case["N"]
    st, u, out = sctx.tensor(case["state"].reshape(-1)), sctx.tensor(case["u_current"]), sctx.zeros(N, D)
    L = lib()
    h = sctx.handle
    assert L.bdf_sample_rows_spike(h, D, N, 1, terms, _p(st), _p(u), 1, 0, 1, _p(out)) == 0
    assert L.bdf_sample_rows_spike(h, 65, N, 1, terms, _p(st), _p(u), 1, 0, 1, _p(out)) == -1 and b"num_latent" in L.bdf_last_error()
    assert L.bdf_sample_rows_spike(h, 0, N, 1, terms, _p(st), _p(u), 1, 0, 1, _p(out)) == -1
    assert L.bdf_sample_rows_spike(h, D, N, 1, terms, None, _p(u), 1, 0, 1, _p(out)) == -1 and b"NULL" in L.bdf_last_error()
    assert L.bdf_sample_rows_spike(h, D, N, 1, terms, _p(st), None, 1, 0, 1, _p(out)) == -1
    assert L.bdf_sample_rows_spike(h, D, N, 1, terms, _p(st), _p(u), 1, 0, 1, None) == -1
    assert L.bdf_sample_rows_spike(h, D, N, 1, terms, _p(st), _p(u), 1, 0, 1, _p(u)) == -1 and b"aliases u_current" in L.bdf_last_error()
    assert L.bdf_sample_rows_spike(h, D, N, 1, terms, _p(st), _p(u), 1, 0, 1, _p(ft[1])) == -1 and b"aliases terms[0].factors[1]" in L.bdf_last_error()
    assert L.bdf_sample_rows_spike(h, D, N + 1, 1, terms, _p(st), _p(u), 1, 0, 1, _p(out)) == -1
    assert L.bdf_sample_rows_spike(h, D, N, 1, terms, _p(st), _p(u), 1, 2, 2, _p(out)) == -1
    assert L.bdf_spike_hyper(h, 65, N, _p(u), 1.0, 1.0, 1.0, 1.0, 1, _p(st)) == -1
    assert L.bdf_spike_hyper(h, D, N, _p(u), 1.0, 1.0, 1.0, 1.0, 1, None) == -1 and b"NULL" in L.bdf_last_error()
    assert L.bdf_spike_hyper(h, D, N, _p(u), 0.25, 1.0, 1.0, 1.0, 1, _p(st)) == -1 and b"incl_a" in L.bdf_last_error()
    assert L.bdf_spike_hyper(h, D, N, _p(u), 1.0, 1.0, float("inf"), 1.0, 1, _p(st)) == -1
    assert L.bdf_spike_hyper(h, D, N, _p(u), 1.0, 1.0, 1.0, 0.0, 1, _p(st)) == -1 and b"rate" in L.bdf_last_error()
    assert L.bdf_spike_accumulate(h, D, N, _p(u), _p(st), None, _p(st)) == -1
    sctx.sync()
    dr.close()


# ---- (f) a planted run ----------------------------------------------------------------------------------------------------------
PLANTED_RMSE_WORST = 0.3546              # the restated chain's worst seed of eight (the docstring below)
PLANTED_MIN_ACTIVITY = 0.3787            # ... and the largest of the eight seeds' smallest activities


def test_planted_run(B):
    """The sketch's shape: rank 3, D = 8, 150 x 40 with half the cells observed (a fifth of those held out), noise sd 0.3, alpha fixed
    at 1 / 0.09, the prior on the 40-row entity with its defaults, 200 + 100 iterations.
    The bounds come from the restated chain (spike_restatement.run_chain) on the CPU over chain seeds 1 .. 8 of this planted data:
    held-out RMSE 0.3531, 0.3503, 0.3522, 0.3480, 0.3546, 0.3525, 0.3474, 0.3523 (range 0.3474 .. 0.3546; the noise floor is 0.3), and
    the smallest posterior activity of a component 0.0095, 0.2692, 0.0063, 0.0022, 0.0093, 0.0213, 0.3787, 0.0053.
    So: RMSE <= 1.1 x 0.3546 = 0.3901 (the chain's seed-to-seed spread), and at least one component with an activity below
    2 x 0.3787 = 0.7574.  No claim on accuracy is made: the Gaussian prior does as well on this data."""
    ids, y, n_test = SR.planted()
    n = len(y)
    ents = [B.Entity("u"), B.Entity("v")]
    rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "planted", ents, alpha=1.0 / 0.09, dims=[150, 40])
    B.assignToTest(rel, np.arange(n - n_test + 1, n + 1))
    B.setSpikeAndSlab(ents[1])
    rd = B.RelationData(rel)
    res = B.macau(rd, num_latent=8, burnin=200, psamples=100, verbose=False, seed=1)
    rd._engine.close()
    sp = res["spike"]["v"]
    assert sorted(res["spike"]) == ["v"] and sorted(sp) == ["activity", "inclusion", "precision", "row_inclusion"]
    assert sp["inclusion"].shape == sp["precision"].shape == sp["activity"].shape == (8,) and sp["row_inclusion"].shape == (40, 8)
    assert np.all(sp["row_inclusion"] >= 0) and np.all(sp["row_inclusion"] <= 1)
    assert np.all((sp["inclusion"] > 0) & (sp["inclusion"] < 1)) and np.all(sp["precision"] > 0)
    np.testing.assert_allclose(sp["activity"], sp["row_inclusion"].mean(axis=0), rtol=0, atol=1e-12)
    rmse = float(res["RMSE"])
    print(f"planted run: held-out RMSE {rmse:.4f}, activity {np.sort(sp['activity'])}")
    assert rmse <= 1.1 * PLANTED_RMSE_WORST
    assert sp["activity"].min() < 2.0 * PLANTED_MIN_ACTIVITY
