"""The probit noise model on the GPU: bdf_probit_draw and the probit link of the prediction kernels
against the numpy restatement (tests/probit_restatement.py), whole macau() iterations on probit relations against the CPU
oracle on both iteration paths, the Gaussian chain untouched by a probit engine in the same process, the quality of the
posterior probabilities on planted data, and the errors of the C ABI."""
import ctypes as C
import os
import textwrap

import numpy as np
import pytest
from scipy.special import ndtr

from both_paths import child
import probit_restatement as PR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _facs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _case(rng, dims, n, D, reach=None):
    """random cells (duplicates included: far more pairs than distinct cells of the first two modes would need), 0/1 values and
    factors; reach: rescale the first factor so that max |udot| is that"""
    ids = np.stack([rng.integers(1, d + 1, n) for d in dims], axis=1)
    ids[1::7] = ids[0]                                    # the same cell many times over
    y = (rng.random(n) < 0.5).astype(np.float64)
    S = [rng.standard_normal((d, D)) for d in dims]
    if reach is not None:
        S[0] *= reach / np.abs(PR.udot(ids, S)).max()
    return ids, y, S


# ---- (a) the draw ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sort", [False, True])
@pytest.mark.parametrize("n_modes", [2, 3])
@pytest.mark.parametrize("D", [1, 7, 10, 32, 64])
def test_probit_draw_matches_the_restatement(B, ctx, D, n_modes, sort):
    from bdf_amd._lib import check, lib
    rng = np.random.default_rng(100 * D + 10 * n_modes + sort)
    dims = [37, 23, 11][:n_modes]
    n = 1003                                               # not a multiple of 8: the last group of lanes is partly idle
    for reach, mean, sweep, tag in ((None, 0.0, 5, 1), (40.0, 0.0, 6, 2), (3.0, 0.3, 7, 3)):
        ids, y, S = _case(rng, dims, n, D, reach)
        pairs = B.DevicePairs(ctx, ids, y)
        if sort:
            pairs.sort(n_modes - 1)
        St = [ctx.tensor(s) for s in S]
        lin, z = ctx.tensor(np.full(n, np.nan)), ctx.tensor(np.full(n, np.nan))
        ctx.set_sweep(sweep)
        check(lib().bdf_probit_draw(ctx.handle, pairs.handle, D, _facs(St), mean, tag, _p(lin), _p(z)))
        lin2 = ctx.tensor(np.full(n, np.nan))
        check(lib().bdf_probit_draw(ctx.handle, pairs.handle, D, _facs(St), mean, tag, _p(lin2), None))      # z_out is optional
        ctx.sync()
        z, lin, lin2 = z.cpu().numpy(), lin.cpu().numpy(), lin2.cpu().numpy()
        m = PR.udot(ids, S) + mean
        if reach == 40.0:
            assert 39.0 < np.abs(m).max() <= 40.0 + 1e-9
        z_ref = PR.draw_z(m, y, PR.uniforms(1234, sweep, tag, n))
        assert np.all(np.isfinite(z)) and np.all((z > 0) == (y > 0.5)) and np.all(z != 0)
        err = np.abs(z - z_ref).max()
        print(f"probit draw D={D} modes={n_modes} sort={sort} reach={reach}: max |z_dev - z_ref| = {err:.3e}")
        assert err <= 1e-9
        assert np.array_equal(lin, y - z) and np.array_equal(lin2, lin)
        pairs.close()


# ---- (b) the link -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_modes,D,sort", [(2, 32, True), (2, 10, False), (3, 8, False), (2, 64, True), (3, 7, True)])
def test_probit_link_of_the_prediction_kernels(B, ctx, n_modes, D, sort):
    rng = np.random.default_rng(7 * D + n_modes)
    dims = [41, 19, 9][:n_modes]
    n, mean, cut = 777, -0.2, 0.5
    ids, y, _ = _case(rng, dims, n, D)
    pairs, plain, back = (B.DevicePairs(ctx, ids, y) for _ in range(3))
    for pr in (pairs, plain, back):
        if sort:
            pr.sort(0)
    pairs.set_link(1)
    back.set_link(1).set_link(0)
    with pytest.raises(B.ArgumentError):
        pairs.set_link(2)
    avg = sq = None
    for phase in (0, 1, 2):
        S = [0.6 * rng.standard_normal((d, D)) for d in dims]
        St = [ctx.tensor(s) for s in S]
        p = ndtr(PR.udot(ids, S) + mean)
        got = pairs.predict(D, St, mean).cpu().numpy()
        assert np.abs(got - p).max() <= 1e-9 and got.min() >= 0.0 and got.max() <= 1.0
        stats = pairs.update(D, St, mean, phase, [], cut)
        ctx.sync()
        stats = stats.cpu().numpy().copy()
        if phase == 0:
            avg, sq = p, np.zeros(n)
        elif phase == 1:
            avg, sq = p, p * p
        else:
            avg, sq = (1.0 * avg + p) / 2.0, sq + p * p
        a, s = pairs.state()
        assert np.abs(a - avg).max() <= 1e-9
        if phase >= 1:
            assert np.abs(s - sq).max() <= 1e-9
        label = y < cut
        want = [np.sum((y - avg) ** 2), np.sum((y - p) ** 2), np.sum(label == (avg < cut)), np.sum(label == (p < cut))]
        np.testing.assert_allclose(stats[:2], want[:2], rtol=1e-9, atol=1e-9)
        assert stats[2] == want[2] and stats[3] == want[3]
        # link 0 after link 1 is the pairs object that never had the call, bit for bit
        g0, g1 = plain.predict(D, St, mean).cpu().numpy(), back.predict(D, St, mean).cpu().numpy()
        s0 = plain.update(D, St, mean, phase, [], cut).cpu().numpy().copy()
        s1 = back.update(D, St, mean, phase, [], cut).cpu().numpy().copy()
        assert np.array_equal(g0, g1) and np.array_equal(s0, s1)
        assert all(np.array_equal(x, w) for x, w in zip(plain.state(), back.state()))
        assert np.abs(g0 - (PR.udot(ids, S) + mean)).max() <= 1e-9
    for pr in (pairs, plain, back):
        pr.close()


# ---- (c) whole iterations ---------------------------------------------------------------------------------------------------
CHILD = textwrap.dedent('''
    import sys
    import numpy as np
    sys.path.insert(0, %r); sys.path.insert(0, %r)
    import bdf_amd as B
    import probit_restatement as PR
    out, n_modes, with_feat = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    ids, y, dims, D, feats, n_test = PR.iteration_case(n_modes, with_feat)
    names = ["a", "b", "c"][:n_modes]
    ents = [B.Entity(nm, F=feats[k]) for k, nm in enumerate(names)]
    table = {nm: ids[:, k] for k, nm in enumerate(names)}
    table["y"] = y
    rel = B.Relation(table, "bin", ents, dims=list(dims))
    B.setProbit(rel)
    B.assignToTest(rel, np.arange(1, n_test + 1))
    rd = B.RelationData(rel)
    res = B.macau(rd, num_latent=D, burnin=1, psamples=1, verbose=False, seed=91)
    d = {"native": np.array(int(rd._engine.native)), "pred": res["predictions"]["pred"].to_numpy(), "mean_value": np.array(rel.model.mean_value)}
    for k, en in enumerate(rd.entities):
        d["S%%d" %% k], d["mu%%d" %% k], d["Lam%%d" %% k] = en.model.sample.T, en.model.mu, en.model.Lambda
        if feats[k] is not None:
            d["beta%%d" %% k], d["lb%%d" %% k] = en.model.beta, np.array(en.lambda_beta)
    np.savez(out, **d)
''') % (ROOT, os.path.join(ROOT, "tests"))


@pytest.mark.parametrize("n_modes,with_feat", [(2, False), (2, True), (3, False), (3, True)])
def test_probit_whole_iterations_match_the_oracle_on_both_paths(n_modes, with_feat):
    ids, y, dims, D, feats, n_test = PR.iteration_case(n_modes, with_feat)
    nat, step = child(CHILD, n_modes, int(with_feat), no_native=False), child(CHILD, n_modes, int(with_feat), no_native=True)
    assert nat["native"] == 1 and step["native"] == 0
    assert sorted(nat) == sorted(step)
    for k in nat:
        if k != "native":
            assert np.array_equal(nat[k], step[k]), k       # the two paths enqueue the same launches: the same bits
    assert nat["mean_value"] == 0.0
    ref = PR.run_chain(ids[n_test:], y[n_test:], dims, D, 91, 2, feats=feats, test_ids=ids[:n_test], burnin=1)
    tol = dict(rtol=1e-6, atol=1e-6)
    for k in range(n_modes):
        np.testing.assert_allclose(nat["S%d" % k], ref["S"][k], err_msg="sample of entity %d" % k, **tol)
        np.testing.assert_allclose(nat["mu%d" % k], ref["mu"][k], **tol)
        np.testing.assert_allclose(nat["Lam%d" % k], ref["Lam"][k], **tol)
        if feats[k] is not None:
            np.testing.assert_allclose(nat["beta%d" % k], ref["beta"][k], rtol=1e-5, atol=1e-6, err_msg="beta of entity %d" % k)
            assert abs(nat["lb%d" % k] - ref["lb"][k]) <= 1e-5 * ref["lb"][k]
    np.testing.assert_allclose(nat["pred"], ref["prob"], **tol)


# ---- (d) nothing else moved --------------------------------------------------------------------------------------------------
def test_gaussian_chain_is_untouched_by_a_probit_engine_in_the_process(B):
    ids, y, n_test = PR.planted(seed=5, N1=120, N2=90, n_cells=4000, n_test=500)

    def gaussian():
        rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y + 0.25 * ids[:, 0] % 3}, "g", [B.Entity("u"), B.Entity("v")], dims=[120, 90])
        B.assignToTest(rel, np.arange(1, n_test + 1))
        rd = B.RelationData(rel)
        res = B.macau(rd, num_latent=16, burnin=2, psamples=2, verbose=False, seed=17)
        out = [en.model.sample.copy() for en in rd.entities] + [res["predictions"]["pred"].to_numpy().copy()]
        rd._engine.close()
        return out

    alone = gaussian()
    rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "p", [B.Entity("u"), B.Entity("v")], dims=[120, 90])
    B.setProbit(rel)
    B.assignToTest(rel, np.arange(1, n_test + 1))
    rdp = B.RelationData(rel)
    B.macau(rdp, num_latent=16, burnin=1, psamples=1, verbose=False, seed=17)
    beside = gaussian()                                     # the probit engine is alive: its pairs carry the link, its relation the model
    assert rdp._engine.gibbs is not None or not rdp._engine.native
    for a, b in zip(alone, beside):
        assert np.array_equal(a, b)
    rdp._engine.close()


# ---- (e) quality --------------------------------------------------------------------------------------------------------------
def test_probit_quality_on_planted_data(B):
    """Planted probit data (rank 4, 300 x 200, 12,000 cells, 3,000 held out).  The yardstick for the held-out ROC of macau()
    (D = 8, 50 + 100 iterations) is the CPU restatement of the same sampler with three other seeds: the device's ROC must be at
    least the smallest of the three minus their spread (max - min), the seed-to-seed noise of the estimator."""
    ids, y, n_test = PR.planted()
    D, burnin, psamples = 8, 50, 100

    def data():
        rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "planted", [B.Entity("u"), B.Entity("v")], dims=[300, 200])
        B.assignToTest(rel, np.arange(12000 - n_test + 1, 12001))
        return rel

    rel = data()
    B.setProbit(rel)
    res = B.macau(B.RelationData(rel), num_latent=D, burnin=burnin, psamples=psamples, verbose=False, seed=1)
    pred, stdev = res["predictions"]["pred"].to_numpy(), res["predictions"]["stdev"].to_numpy()
    assert pred.min() >= 0.0 and pred.max() <= 1.0 and stdev.min() >= 0.0 and np.all(np.isfinite(stdev))
    label = y[-n_test:] < 0.5
    assert np.array_equal(rel.test_label, label)
    roc_dev = B.AUC_ROC(label, -pred)
    assert abs(res["ROC"] - roc_dev) <= 1e-12
    assert abs(res["RMSE"] - np.sqrt(np.mean((y[-n_test:] - pred) ** 2))) <= 1e-9            # the root Brier score
    assert abs(res["accuracy"] - np.mean(label == (pred < 0.5))) <= 1e-12
    cpu = []
    for seed in (2, 3, 4):
        ref = PR.run_chain(ids[:-n_test], y[:-n_test], [300, 200], D, seed, burnin + psamples, test_ids=ids[-n_test:], burnin=burnin)
        cpu.append(B.AUC_ROC(label, -ref["prob"]))
    g = data()
    res_g = B.macau(B.RelationData(g), num_latent=D, burnin=burnin, psamples=psamples, verbose=False, seed=1)
    roc_gauss = B.AUC_ROC(label, -res_g["predictions"]["pred"].to_numpy())
    print(f"probit quality: device ROC {roc_dev:.4f} (Brier RMSE {res['RMSE']:.4f}, accuracy {res['accuracy']:.4f}); CPU restatement ROC "
          f"{cpu[0]:.4f} {cpu[1]:.4f} {cpu[2]:.4f}; Gaussian macau() on the same 0/1 data: ROC {roc_gauss:.4f} (information only)")
    assert roc_dev >= min(cpu) - (max(cpu) - min(cpu)), (roc_dev, cpu)


# ---- (f) errors through the C ABI ---------------------------------------------------------------------------------------------
def test_probit_c_abi_errors(B, ctx):
    from bdf_amd._lib import GibbsRelation, check, lib
    ids, y, n_test = PR.planted(seed=9, N1=60, N2=50, n_cells=1500, n_test=100)
    rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "e", [B.Entity("u"), B.Entity("v")], dims=[60, 50])
    eng = B.GibbsEngine(B.RelationData(rel), 8, seed=3)
    assert eng.native
    train = B.DevicePairs(eng.ctx, ids, y)
    op = B.FeatOperator(eng.ctx, np.ones((len(y), 2)))
    lin, beta, alpha = eng.ctx.zeros(len(y)), eng.ctx.zeros(2), eng.ctx.tensor([1.0])

    def record(**kw):
        arr = (GibbsRelation * 1)()
        g = arr[0]
        g.rel, g.mean_value, g.alpha_dev, g.rel_tag, g.nnz = eng.rel[0].handle, 0.0, alpha.data_ptr(), 1, len(y)
        g.entity_of_mode[0], g.entity_of_mode[1] = 0, 1
        g.train, g.first_obs, g.obs_block, g.linear, g.probit = train.handle, 0, len(y), lin.data_ptr(), 1
        for k, v in kw.items():
            setattr(g, k, v)
        return arr

    def register(arr):
        check(lib().bdf_gibbs_set_relations(eng.gibbs, 1, C.cast(arr, C.c_void_p)))

    with pytest.raises(B.ArgumentError, match="probit"):
        register(record(feat=op.handle, beta=beta.data_ptr()))
    with pytest.raises(B.ArgumentError, match="probit"):
        register(record(alpha_sample=1))
    with pytest.raises(B.ArgumentError, match="probit"):
        register(record(linear=None))
    with pytest.raises(B.ArgumentError, match="probit"):
        register(record(train=None))
    with pytest.raises(B.ArgumentError, match="link"):
        check(lib().bdf_pairs_set_link(train.handle, 2))
    with pytest.raises(B.ArgumentError):
        check(lib().bdf_pairs_set_link(train.handle, -1))
    with pytest.raises(B.ArgumentError):
        check(lib().bdf_probit_draw(eng.ctx.handle, train.handle, 8, _facs(eng.factors_of(rel)), 0.0, 1, None, None))
    register(record())                                       # and the well-formed record is accepted: one iteration runs
    eng.sweep(1)
    eng.sync()
    assert np.all(np.isfinite(rel.entities[0].model.sample))
    op.close()
    train.close()
    eng.close()
