"""The non-negative prior of an entity's rows on the GPU: the sweep kernel alone on crafted systems, the row
launch (K1's system dump, then the sweep) and the hyper step against the restatement (tests/nonneg_restatement.py), whole macau()
iterations against the restated chain on both iteration paths, the Gaussian chain untouched by a non-negative engine in the same
process, the C ABI's errors and a planted run."""
import ctypes as C
import os
import textwrap

import numpy as np
import pytest

from both_paths import child
import nonneg_restatement as NR
import spike_restatement as SR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


@pytest.fixture(scope="module")
def nctx(B):
    """a context of this module's own (the session's seed): its item size is 64 observations, so that the planted rows of 65 and
    300 observations are split and finished by the last wave to arrive"""
    c = B.Context(seed=SR.ROW_SEED)
    c.set_item_size(64)
    yield c
    c.set_nonneg_chunk(0)
    c.close()


def _close(out, ref):
    return np.abs(out - ref) <= 1e-9 * (1.0 + np.abs(ref))


# ---- (a) the sweep alone --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", NR.SWEEP_ROWS)
@pytest.mark.parametrize("D", NR.SWEEP_DS)
def test_sweep_matches_the_restatement(B, nctx, D, n_rows):
    """bdf_nonneg_sweep on crafted P = diag + A A' and c whose elements between them meet t > 8, |t| < 1, t in (-36, -5) and
    t < -37 (asserted per case from 8 elements on, and over all cases in tests/test_nonneg_host.py, which also holds every case's
    branch margin above 1e-9): every element within 1e-9 (1 + |ref|), finite and >= 0; a rerun gives the same bits, and so do
    chunks of 64 rows (n_rows = 200: four, the last of 8)."""
    from bdf_amd._lib import check, lib
    case = NR.sweep_case(D, n_rows)
    nctx.set_sweep(case["sweep"])
    P_t, c_t, u_t = nctx.tensor(case["P"]), nctx.tensor(case["c"]), nctx.tensor(case["u_current"])
    outs = []
    for chunk in (0, 0, 64):
        nctx.set_nonneg_chunk(chunk)
        out_t = nctx.tensor(np.full((n_rows, D), np.nan))
        check(lib().bdf_nonneg_sweep(nctx.handle, D, n_rows, _p(P_t), _p(c_t), _p(u_t), NR.SWEEP_TAG, NR.SWEEP_ROW_BEGIN, _p(out_t)))
        nctx.sync()
        outs.append(out_t.cpu().numpy())
    nctx.set_nonneg_chunk(0)
    out = outs[0]
    assert np.array_equal(out, outs[1]) and np.array_equal(out, outs[2])
    U = NR.uniforms(SR.ROW_SEED, case["sweep"], NR.SWEEP_TAG, n_rows, D, NR.SWEEP_ROW_BEGIN)
    if n_rows == 1:                                        # the stream's blocks as the library itself draws them
        w4 = (C.c_uint32 * 4)()
        for d in range(D):
            check(lib().bdf_philox(nctx.handle, NR.P_NONNEG, NR.SWEEP_TAG, NR.SWEEP_ROW_BEGIN, d, w4))
            assert U[0, d] == NR._u01(w4[0], w4[1])
    ref, margin, t = NR.sweep_rows(case["P"], case["c"], case["u_current"], U, with_t=True)
    k = NR.t_classes(t)
    print(f"nonneg sweep D={D} rows={n_rows}: branch margin {margin:.3e}, classes {k}, "
          f"max |device - ref| / (1 + |ref|) {np.max(np.abs(out - ref) / (1 + np.abs(ref))):.3e}")
    assert margin >= 1e-9
    assert n_rows * D < 8 or all(x > 0 for x in k)
    assert np.all(np.isfinite(out)) and np.all(out >= 0.0)
    assert np.all(_close(out, ref)), (D, n_rows)


# ---- (b) the row launch ---------------------------------------------------------------------------------------------------------
def _launch(B, ctx, case, D, mode, weights="own", general=False, decoy=False):
    """-> (out, out of a rerun, out in chunks of 16 rows, P, c) of the case's launch; weights: "own" (the case's) or None
    (dropped); general: the general gather forced (bdf_ctx_set_gather); decoy: alpha through alpha_dev with another scalar in its
    place"""
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
    tau_t, u_t = ctx.tensor(case["tau"]), ctx.tensor(case["u_current"])
    Lam_t, mu_t = ctx.tensor(np.diag(case["tau"])), ctx.zeros(D)
    P_t, c_t = ctx.zeros(N, D, D), ctx.zeros(N, D)
    check(lib().bdf_row_system(ctx.handle, D, N, nt, terms, _p(mu_t), 0, _p(Lam_t), _p(P_t), _p(c_t)))
    outs = []
    for chunk in (0, 0, 16):
        ctx.set_nonneg_chunk(chunk)
        out_t = ctx.tensor(np.full((N, D), np.nan))
        check(lib().bdf_sample_rows_nonneg(ctx.handle, D, N, nt, terms, _p(tau_t), _p(u_t), NR.ROW_TAG, 0, 1, _p(out_t)))
        ctx.sync()
        outs.append(out_t.cpu().numpy())
    ctx.set_nonneg_chunk(0)
    assert ctx.rows_unfinished() == 0
    ctx.set_gather(0)
    got = (outs[0], outs[1], outs[2], P_t.cpu().numpy(), c_t.cpu().numpy())
    for dr in drs:
        dr.close()
    return got


@pytest.mark.parametrize("D,n_modes,mode,variant", SR.row_cases())
def test_row_launch_matches_the_restatement(B, nctx, D, n_modes, mode, variant):
    """The device's own P and c (bdf_row_system with Lambda = diag tau, mu = 0) through the restated sweep with the restated
    uniforms: every element within 1e-9 (1 + |ref|), finite and >= 0; a rerun gives the same bits, and so do chunks of 16 rows
    (three, two or one chunk for the 37, 23 and 11 rows of the cases' entities)."""
    case = NR.row_case(D, n_modes, mode, variant)
    out, again, chunked, P, c = _launch(B, nctx, case, D, mode, decoy=variant == "alpha_dev")
    assert np.all(np.isfinite(out)) and np.all(out >= 0.0)
    assert np.array_equal(out, again) and np.array_equal(out, chunked)
    U = NR.uniforms(SR.ROW_SEED, case["sweep"], NR.ROW_TAG, case["N"], D)
    ref, margin = NR.sweep_rows(P, c, case["u_current"], U)
    print(f"nonneg rows D={D} modes={n_modes} mode={mode} {variant}: branch margin {margin:.3e}, "
          f"max |device - ref| / (1 + |ref|) {np.max(np.abs(out - ref) / (1 + np.abs(ref))):.3e}")
    assert margin >= 1e-9
    assert np.all(_close(out, ref)), (D, n_modes, mode, variant)
    if variant == "unit":
        # unit weights are no weights: the bits of the unweighted launch on the same (general) gather
        plain = _launch(B, nctx, case, D, mode, weights=None, general=True)[0]
        assert np.array_equal(out, plain)


def test_row_launch_takes_shards(B, nctx):
    """two shards of the rows between them give the bits of the one launch (each launch writes its own rows only)"""
    from bdf_amd._lib import Term, check, lib
    D, mode = 17, 0
    case = NR.row_case(D, 2, mode, "plain")
    ids, vals, _, alpha = case["rels"][0]
    dr = B.DeviceRelation(nctx, B.IndexedDF((ids, vals), case["dims"]))
    ft = [nctx.tensor(f) for f in case["facs"]]
    terms = (Term * 1)()
    terms[0].rel, terms[0].mode, terms[0].alpha, terms[0].mean_value = dr.handle, mode, alpha, float(np.mean(vals))
    terms[0].factors[1] = ft[1].data_ptr()
    N = case["N"]
    nctx.set_sweep(case["sweep"])
    tau_t, u_t = nctx.tensor(case["tau"]), nctx.tensor(case["u_current"])
    whole, parts = nctx.tensor(np.full((N, D), np.nan)), nctx.tensor(np.full((N, D), np.nan))
    check(lib().bdf_sample_rows_nonneg(nctx.handle, D, N, 1, terms, _p(tau_t), _p(u_t), NR.ROW_TAG, 0, 1, _p(whole)))
    nctx.set_nonneg_chunk(8)
    for s in range(2):
        check(lib().bdf_sample_rows_nonneg(nctx.handle, D, N, 1, terms, _p(tau_t), _p(u_t), NR.ROW_TAG, s, 2, _p(parts)))
    nctx.set_nonneg_chunk(0)
    nctx.sync()
    assert np.array_equal(whole.cpu().numpy(), parts.cpu().numpy()) and np.all(np.isfinite(parts.cpu().numpy()))
    dr.close()


# ---- (c) the hyper step ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 255, 256, 257, 1003])
@pytest.mark.parametrize("D", [1, 7, 32, 64])
def test_hyper_step_matches_the_restatement(B, nctx, D, N):
    from bdf_amd._lib import check, lib
    rng = np.random.default_rng(3100 + 70 * D + N)
    S = np.abs(rng.standard_normal((N, D))) * np.exp(rng.uniform(-3.0, 1.0, D))[None, :]
    S[:, 0] = 0.0                                                       # a component that is switched off altogether
    S_t = nctx.tensor(S)
    sweep, tag = 50 + D, 9
    nctx.set_sweep(sweep)
    worst = 0.0
    for shape, rate in ((1.0, 1.0), (0.5, 0.07)):
        got = []
        for rep in range(2):
            tau_t = nctx.tensor(np.full(D, np.nan))
            check(lib().bdf_nonneg_hyper(nctx.handle, D, N, _p(S_t), shape, rate, tag, _p(tau_t)))
            nctx.sync()
            got.append(tau_t.cpu().numpy())
        assert np.array_equal(got[0], got[1])                           # bit for bit across reruns
        ref = NR.hyper_draw(S, shape, rate, SR.ROW_SEED, sweep, tag)
        worst = max(worst, float(np.max(np.abs(got[0] - ref) / ref)))
        np.testing.assert_allclose(got[0], ref, rtol=1e-12, atol=0)
    print(f"nonneg hyper D={D} N={N}: max rel. error {worst:.3e}")


def test_accumulate_adds_the_rows_and_tau(B, nctx):
    from bdf_amd._lib import check, lib
    rng = np.random.default_rng(4)
    N, D = 300, 7
    S, tau = np.abs(rng.standard_normal((N, D))), rng.uniform(0.5, 2.0, D)
    rs, hs = rng.standard_normal((N, D)), rng.standard_normal(D)
    S_t, tau_t, rs_t, hs_t = nctx.tensor(S), nctx.tensor(tau), nctx.tensor(rs), nctx.tensor(hs)
    check(lib().bdf_nonneg_accumulate(nctx.handle, D, N, _p(S_t), _p(tau_t), _p(rs_t), _p(hs_t)))
    nctx.sync()
    assert np.array_equal(rs_t.cpu().numpy(), rs + S) and np.array_equal(hs_t.cpu().numpy(), hs + tau)


# ---- (d) whole iterations -------------------------------------------------------------------------------------------------------
CHILD = textwrap.dedent('''
    import sys
    import numpy as np
    sys.path.insert(0, %r); sys.path.insert(0, %r)
    import bdf_amd as B
    import nonneg_restatement as NR
    out, d = sys.argv[1], {}
    for name in NR.CHAIN_MODELS:
        dims, rels, nonneg, spike, feats, n_test = NR.chain_model(name)
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
        for j, prm in nonneg.items():
            B.setNonNegative(ents[j], *prm)
        res = B.macau(rd, num_latent=NR.CHAIN_D, burnin=3, psamples=3, verbose=False, seed=NR.CHAIN_SEED)
        key = name + "_"
        d[key + "native"], d[key + "pred"] = np.array(int(rd._engine.native)), res["predictions"]["pred"].to_numpy()
        d[key + "alpha"] = np.array([r.model.alpha for r in rd.relations])
        d[key + "mean"] = np.array([r.model.mean_value for r in rd.relations])
        d[key + "order"] = np.array([ents.index(e) for e in rd.entities])
        assert sorted(res["nonneg"]) == sorted(ents[j].name for j in nonneg)
        assert ("spike" in res) == bool(spike)
        for k, en in enumerate(ents):
            d[key + "S%%d" %% k] = en.model.sample.T
            assert (" nn" in B.toStr(en)) == (k in nonneg)
            if k in nonneg:
                for f, v in res["nonneg"][en.name].items():
                    d[key + "%%s%%d" %% (f, k)] = v
                d[key + "tau%%d" %% k] = en.model._dev.nonneg_tau.cpu().numpy()
            elif k in spike:
                d[key + "state%%d" %% k] = en.model._dev.spike_state.cpu().numpy()
            else:
                d[key + "mu%%d" %% k], d[key + "Lam%%d" %% k] = en.model.mu, en.model.Lambda
        rd._engine.close()
    np.savez(out, **d)
''') % (ROOT, os.path.join(ROOT, "tests"))


@pytest.fixture(scope="module")
def chains():
    """3 + 3 iterations of every model of NR.CHAIN_MODELS on the native and on the step-by-step path: one child process per path"""
    return child(CHILD, no_native=False), child(CHILD, no_native=True)


@pytest.mark.parametrize("name", NR.CHAIN_MODELS)
def test_whole_iterations_match_the_restated_chain_on_both_paths(chains, name):
    dims, rels, nonneg, spike, feats, n_test = NR.chain_model(name)
    key = name + "_"
    nat, step = ({k[len(key):]: v for k, v in ch.items() if k.startswith(key)} for ch in chains)
    assert nat["native"] == 1 and step["native"] == 0
    assert sorted(nat) == sorted(step)
    for k in nat:
        if k != "native":
            assert np.array_equal(nat[k], step[k]), k       # the two paths enqueue the same launches: the same bits
    assert np.array_equal(nat["order"], np.arange(len(dims)))
    train = [dict(r, ids=r["ids"][n_test:], values=r["values"][n_test:]) if i == 0 else r for i, r in enumerate(rels)]
    ref = NR.run_chain(train, dims, NR.CHAIN_D, NR.CHAIN_SEED, 6, nonneg, spike=spike, feats=feats, burnin=3, test_ids=rels[0]["ids"][:n_test])
    assert ref["margin"] >= 1e-9 and ref["spike_margin"] >= 1e-9
    tol = dict(rtol=1e-9, atol=1e-6)
    np.testing.assert_allclose(nat["alpha"], ref["alpha"], **tol)
    assert bool(np.any(nat["alpha"] != 2.5)) == (name == "alpha")
    # a relation ALL of whose entities are non-negative is not centred; every other one is
    np.testing.assert_allclose(nat["mean"], ref["mean"], rtol=1e-12, atol=0)
    assert (nat["mean"][0] == 0.0) == (name == "both")
    for k in range(len(dims)):
        np.testing.assert_allclose(nat["S%d" % k], ref["S"][k], err_msg="sample of entity %d" % k, **tol)
        if k in nonneg:
            assert np.all(nat["S%d" % k] >= 0) and np.all(nat["factors%d" % k] >= 0)
            np.testing.assert_allclose(nat["tau%d" % k], ref["tau"][k], **tol)
            for f, v in ref["nonneg"][k].items():
                np.testing.assert_allclose(nat["%s%d" % (f, k)], v, err_msg=f, **tol)
        elif k in spike:
            assert np.array_equal(nat["S%d" % k] != 0, ref["S"][k] != 0)
            np.testing.assert_allclose(nat["state%d" % k].reshape(4, -1), ref["state"][k], **tol)
        else:
            np.testing.assert_allclose(nat["mu%d" % k], ref["mu"][k], **tol)
            np.testing.assert_allclose(nat["Lam%d" % k], ref["Lam"][k], **tol)
    np.testing.assert_allclose(nat["pred"], ref["pred"], **tol)


# ---- (e) nothing else moved -----------------------------------------------------------------------------------------------------
def test_gaussian_chain_is_untouched_by_a_nonneg_engine_in_the_process(B):
    ids, y, n_test = NR.planted(seed=5, N1=120, N2=60)
    n = len(y)

    def gaussian():
        rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "g", [B.Entity("u"), B.Entity("v")], dims=[120, 60])
        B.assignToTest(rel, np.arange(n - n_test + 1, n + 1))
        rd = B.RelationData(rel)
        res = B.macau(rd, num_latent=16, burnin=2, psamples=2, verbose=False, seed=17)
        assert "nonneg" not in res and all(st.nonneg_tau is None for st in rd._engine.ent)
        out = [en.model.sample.copy() for en in rd.entities] + [res["predictions"]["pred"].to_numpy().copy()]
        rd._engine.close()
        return out

    alone = gaussian()
    ents = [B.Entity("u"), B.Entity("v")]
    rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "s", ents, dims=[120, 60])
    B.assignToTest(rel, np.arange(n - n_test + 1, n + 1))
    B.setNonNegative(ents[1])
    rds = B.RelationData(rel)
    res = B.macau(rds, num_latent=16, burnin=1, psamples=1, verbose=False, seed=17)
    assert res["nonneg"]["v"]["factors"].shape == (60, 16) and res["nonneg"]["v"]["precision"].shape == (16,)
    assert rel.model.mean_value != 0.0                      # one free entity: centred
    assert B.toStr(ents[1]).endswith(" nn]") and " nn" not in B.toStr(ents[0])
    beside = gaussian()                                     # the non-negative engine is alive
    for a, b in zip(alone, beside):
        assert np.array_equal(a, b)
    rds._engine.close()


# ---- (f) errors through the C ABI -----------------------------------------------------------------------------------------------
def test_nonneg_c_abi_errors(B, nctx):
    from bdf_amd._lib import Term, lib
    D, mode = 5, 0
    case = NR.row_case(D, 2, mode, "plain")
    ids, vals, _, alpha = case["rels"][0]
    dr = B.DeviceRelation(nctx, B.IndexedDF((ids, vals), case["dims"]))
    ft = [nctx.tensor(f) for f in case["facs"]]
    terms = (Term * 1)()
    terms[0].rel, terms[0].mode, terms[0].alpha, terms[0].mean_value = dr.handle, mode, alpha, 0.0
    terms[0].factors[1] = ft[1].data_ptr()
    N = case["N"]
    tau, u, out = nctx.tensor(case["tau"]), nctx.tensor(case["u_current"]), nctx.zeros(N, D)
    P, c = nctx.tensor(np.broadcast_to(np.eye(D), (N, D, D)).copy()), nctx.zeros(N, D)
    L = lib()
    h = nctx.handle
    assert L.bdf_sample_rows_nonneg(h, D, N, 1, terms, _p(tau), _p(u), 1, 0, 1, _p(out)) == 0
    assert L.bdf_sample_rows_nonneg(h, 65, N, 1, terms, _p(tau), _p(u), 1, 0, 1, _p(out)) == -1 and b"num_latent" in L.bdf_last_error()
    assert L.bdf_sample_rows_nonneg(h, 0, N, 1, terms, _p(tau), _p(u), 1, 0, 1, _p(out)) == -1
    assert L.bdf_sample_rows_nonneg(h, D, N, 1, terms, None, _p(u), 1, 0, 1, _p(out)) == -1 and b"NULL" in L.bdf_last_error()
    assert L.bdf_sample_rows_nonneg(h, D, N, 1, terms, _p(tau), None, 1, 0, 1, _p(out)) == -1
    assert L.bdf_sample_rows_nonneg(h, D, N, 1, terms, _p(tau), _p(u), 1, 0, 1, None) == -1
    assert L.bdf_sample_rows_nonneg(h, D, N, 1, terms, _p(tau), _p(u), 1, 0, 1, _p(u)) == -1 and b"aliases u_current" in L.bdf_last_error()
    assert L.bdf_sample_rows_nonneg(h, D, N, 1, terms, _p(tau), _p(u), 1, 0, 1, _p(ft[1])) == -1 and b"aliases terms[0].factors[1]" in L.bdf_last_error()
    assert L.bdf_sample_rows_nonneg(h, D, N + 1, 1, terms, _p(tau), _p(u), 1, 0, 1, _p(out)) == -1
    assert L.bdf_sample_rows_nonneg(h, D, N, 1, terms, _p(tau), _p(u), 1, 2, 2, _p(out)) == -1
    assert L.bdf_nonneg_sweep(h, D, N, _p(P), _p(c), _p(u), 1, 0, _p(out)) == 0
    assert L.bdf_nonneg_sweep(h, 65, N, _p(P), _p(c), _p(u), 1, 0, _p(out)) == -1 and b"num_latent" in L.bdf_last_error()
    assert L.bdf_nonneg_sweep(h, D, 0, _p(P), _p(c), _p(u), 1, 0, _p(out)) == -1
    assert L.bdf_nonneg_sweep(h, D, N, None, _p(c), _p(u), 1, 0, _p(out)) == -1 and b"NULL" in L.bdf_last_error()
    assert L.bdf_nonneg_sweep(h, D, N, _p(P), None, _p(u), 1, 0, _p(out)) == -1
    assert L.bdf_nonneg_sweep(h, D, N, _p(P), _p(c), _p(u), 1, -1, _p(out)) == -1
    assert L.bdf_nonneg_sweep(h, D, N, _p(P), _p(c), _p(u), 1, 0, _p(u)) == -1 and b"aliases u_current" in L.bdf_last_error()
    assert L.bdf_nonneg_hyper(h, 65, N, _p(u), 1.0, 1.0, 1, _p(tau)) == -1
    assert L.bdf_nonneg_hyper(h, D, 0, _p(u), 1.0, 1.0, 1, _p(tau)) == -1
    assert L.bdf_nonneg_hyper(h, D, N, _p(u), 1.0, 1.0, 1, None) == -1 and b"NULL" in L.bdf_last_error()
    assert L.bdf_nonneg_hyper(h, D, N, _p(u), 0.25, 1.0, 1, _p(tau)) == -1 and b"shape" in L.bdf_last_error()
    assert L.bdf_nonneg_hyper(h, D, N, _p(u), float("inf"), 1.0, 1, _p(tau)) == -1
    assert L.bdf_nonneg_hyper(h, D, N, _p(u), 1.0, 0.0, 1, _p(tau)) == -1 and b"rate" in L.bdf_last_error()
    assert L.bdf_nonneg_hyper(h, D, N, _p(u), 1.0, float("inf"), 1, _p(tau)) == -1
    assert L.bdf_nonneg_accumulate(h, D, N, _p(u), _p(tau), None, _p(tau)) == -1
    assert L.bdf_nonneg_accumulate(h, 0, N, _p(u), _p(tau), _p(out), _p(tau)) == -1
    assert L.bdf_ctx_set_nonneg_chunk(h, -1) == -1
    assert L.bdf_ctx_set_nonneg_chunk(None, 0) == -1
    nctx.sync()
    dr.close()


# ---- (g) a planted run ----------------------------------------------------------------------------------------------------------
PLANTED_RMSE_WORST = 0.3433              # the restated chain's worst seed of eight (the docstring below)
PLANTED_FOURTH_MS = 0.0799               # ... and the largest of the eight seeds' fourth-smallest mean squares


def test_planted_run(B):
    """The sketch's shape: planted rank-3 NON-NEGATIVE factors (nonneg_restatement.planted), D = 8, 150 x 40 with half the cells
    observed (a fifth of those held out), noise sd 0.3, alpha fixed at 1 / 0.09, both entities non-negative with the defaults (so the
    relation is not centred), 200 + 100 iterations.
    The bounds come from the restated chain (nonneg_restatement.planted_chain) on the CPU over chain seeds 1 .. 8 of this planted
    data: held-out RMSE 0.3391, 0.3400, 0.3380, 0.3433, 0.3405, 0.3356, 0.3382, 0.3412 (the noise floor is 0.3), and the
    fourth-smallest mean square of a component of the 40-row entity's posterior-mean factors 0.0655, 0.0707, 0.0652, 0.0600,
    0.0731, 0.0726, 0.0583, 0.0799 (the largest components: 0.25 .. 3.2).
    So: RMSE <= 1.1 x 0.3433 = 0.3776 (the chain's seed-to-seed spread), every factor >= 0, and at least four components with a
    mean square below 2 x 0.0799 = 0.1598: the per-component precision switches the surplus components off by itself.  No claim
    on accuracy over the Gaussian prior is made."""
    ids, y, n_test = NR.planted()
    n = len(y)
    ents = [B.Entity("u"), B.Entity("v")]
    rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "planted", ents, alpha=1.0 / 0.09, dims=[150, 40])
    B.assignToTest(rel, np.arange(n - n_test + 1, n + 1))
    B.setNonNegative(ents[0])
    B.setNonNegative(ents[1])
    rd = B.RelationData(rel)
    res = B.macau(rd, num_latent=8, burnin=200, psamples=100, verbose=False, seed=1)
    samples = [en.model.sample.copy() for en in ents]
    rd._engine.close()
    assert rel.model.mean_value == 0.0
    assert sorted(res["nonneg"]) == ["u", "v"] and sorted(res["nonneg"]["v"]) == ["factors", "precision"]
    fu, fv = res["nonneg"]["u"]["factors"], res["nonneg"]["v"]["factors"]
    assert fu.shape == (150, 8) and fv.shape == (40, 8) and res["nonneg"]["v"]["precision"].shape == (8,)
    assert np.all(fu >= 0) and np.all(fv >= 0) and all(np.all(s >= 0) for s in samples)
    assert np.all(res["nonneg"]["u"]["precision"] > 0) and np.all(res["nonneg"]["v"]["precision"] > 0)
    rmse = float(res["RMSE"])
    ms = np.sort(np.mean(fv * fv, axis=0))
    print(f"planted run: held-out RMSE {rmse:.4f}, mean squares of the components {np.round(ms, 4)}")
    assert rmse <= 1.1 * PLANTED_RMSE_WORST
    assert np.sum(ms < 2.0 * PLANTED_FOURTH_MS) >= 4
