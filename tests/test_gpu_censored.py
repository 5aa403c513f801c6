"""The censored (Tobit) noise model on the GPU: bdf_censored_draw against the numpy restatement
(tests/censored_restatement.py), whole macau() iterations on censored relations against the CPU oracle on both iteration paths,
all-zero flags against no flags, the Gaussian chain untouched by a censored engine in the same process, the held-out error on
planted data, and the errors of the C ABI."""
import ctypes as C
import os
import textwrap

import numpy as np
import pytest

from both_paths import child
import censored_restatement as CR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _facs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _flags(rng, n, kind):
    """mixed: about 30 % +1 and 10 % -1; exact: none; all: every observation censored; group: all censored but the 8 consecutive
    observations 16 .. 23, one group of eight lanes of unsorted pairs"""
    if kind == "exact":
        return np.zeros(n, dtype=np.int8)
    if kind == "mixed":
        pick = rng.random(n)
        return np.where(pick < 0.3, 1, np.where(pick < 0.4, -1, 0)).astype(np.int8)
    c = np.where(rng.random(n) < 0.6, 1, -1).astype(np.int8)
    if kind == "group":
        c[16:24] = 0
    return c


# ---- (a) the draw -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sort", [False, True])
@pytest.mark.parametrize("n_modes", [2, 3])
@pytest.mark.parametrize("D", [1, 7, 10, 32, 64])
def test_censored_draw_matches_the_restatement(B, ctx, D, n_modes, sort):
    import torch
    from bdf_amd._lib import check, lib
    rng = np.random.default_rng(1000 + 100 * D + 10 * n_modes + sort)
    dims = [37, 23, 11][:n_modes]
    n = 1003                                               # not a multiple of 8: the last group of lanes is partly idle
    ids = np.stack([rng.integers(1, d + 1, n) for d in dims], axis=1)
    ids[1::7] = ids[0]                                     # the same cell many times over
    y = rng.standard_normal(n)
    pairs = B.DevicePairs(ctx, ids, y)
    if sort:
        pairs.sort(n_modes - 1)
    past, worst = 0, 0.0
    sweep = 3
    for reach, mean in ((None, 0.3), (40.0, -0.2)):
        S = [rng.standard_normal((d, D)) for d in dims]
        if reach is not None:                              # rescale the first factor so that max |udot| is `reach`
            S[0] *= reach / np.abs(CR.udot(ids, S)).max()
        St = [ctx.tensor(s) for s in S]
        m = CR.udot(ids, S) + mean
        for kind in ("mixed", "exact", "all", "group"):
            c = _flags(rng, n, kind)
            cd = ctx.tensor(c, dtype=torch.int8)
            for alpha in (0.04, 5.0, 900.0):
                for through_dev in (False, True):
                    sweep += 1
                    tag = 1 + sweep % 3
                    # through alpha_dev the scalar argument is a decoy: the device value wins
                    a_arg, a_dev = (alpha, None) if not through_dev else (123.0, ctx.tensor([alpha]))
                    lin, z, lin2 = (ctx.tensor(np.full(n, np.nan)) for _ in range(3))
                    ctx.set_sweep(sweep)
                    check(lib().bdf_censored_draw(ctx.handle, pairs.handle, _p(cd), D, _facs(St), mean, a_arg, _p(a_dev), tag, _p(lin), _p(z)))
                    check(lib().bdf_censored_draw(ctx.handle, pairs.handle, _p(cd), D, _facs(St), mean, a_arg, _p(a_dev), tag, _p(lin2), None))
                    ctx.sync()
                    z, lin, lin2 = z.cpu().numpy(), lin.cpu().numpy(), lin2.cpu().numpy()
                    z_ref = CR.draw_z(m, y, c, alpha, CR.uniforms(1234, sweep, tag, n))
                    assert np.all(np.isfinite(z)) and np.all(c * (z - y) >= 0)           # never on the wrong side of the bound
                    assert np.array_equal(z[c == 0], y[c == 0])
                    err = np.abs(z - z_ref).max()
                    worst = max(worst, err)
                    assert err <= 1e-9, (kind, alpha, through_dev, reach, err)
                    assert np.array_equal(lin, mean + (y - z)) and np.array_equal(lin2, lin)      # z_out is optional
                    assert np.all(lin[c == 0] == mean)
                    t = c * (m - y) * np.sqrt(alpha)
                    if alpha == 900.0 and kind != "exact":
                        assert t.min() < -37.5 and t.max() > 37.5                        # both sides of the underflow of Phi(t)
                        past += 1
    print(f"censored draw D={D} modes={n_modes} sort={sort}: max |z_dev - z_ref| = {worst:.3e} over 48 launches")
    assert past > 0
    pairs.close()


# ---- (b) whole iterations ---------------------------------------------------------------------------------------------------
CASES = [(n_modes, with_feat, alpha_sample) for n_modes in (2, 3) for with_feat in (0, 1) for alpha_sample in (0, 1)]

CHILD = textwrap.dedent('''
    import sys
    import numpy as np
    sys.path.insert(0, %r); sys.path.insert(0, %r)
    import bdf_amd as B
    import censored_restatement as CR
    out, d = sys.argv[1], {}
    for n_modes in (2, 3):
        for with_feat in (0, 1):
            for alpha_sample in (0, 1):
                ids, y, c, dims, D, feats, n_test, alpha, _ = CR.iteration_case(n_modes, with_feat, alpha_sample)
                names = ["a", "b", "c"][:n_modes]
                ents = [B.Entity(nm, F=feats[k]) for k, nm in enumerate(names)]
                table = {nm: ids[:, k] for k, nm in enumerate(names)}
                table["y"] = y
                rel = B.Relation(table, "cens", ents, alpha=alpha, dims=list(dims))
                rel.model.alpha_sample = bool(alpha_sample)
                B.assignToTest(rel, np.arange(1, n_test + 1))
                B.setCensored(rel, c[n_test:])
                rd = B.RelationData(rel)
                res = B.macau(rd, num_latent=D, burnin=1, psamples=1, verbose=False, seed=91)
                key = "%%d%%d%%d_" %% (n_modes, with_feat, alpha_sample)
                d[key + "native"], d[key + "pred"] = np.array(int(rd._engine.native)), res["predictions"]["pred"].to_numpy()
                d[key + "mean"], d[key + "alpha"] = np.array(rel.model.mean_value), np.array(rel.model.alpha)
                for k, en in enumerate(rd.entities):
                    d[key + "S%%d" %% k], d[key + "mu%%d" %% k], d[key + "Lam%%d" %% k] = en.model.sample.T, en.model.mu, en.model.Lambda
                    if feats[k] is not None:
                        d[key + "beta%%d" %% k], d[key + "lb%%d" %% k] = en.model.beta, np.array(en.lambda_beta)
                rd._engine.close()
    np.savez(out, **d)
''') % (ROOT, os.path.join(ROOT, "tests"))


@pytest.fixture(scope="module")
def chains():
    """two iterations of every case of CASES on the native and on the step-by-step path: one child process per path"""
    return child(CHILD, no_native=False), child(CHILD, no_native=True)


@pytest.mark.parametrize("n_modes,with_feat,alpha_sample", CASES)
def test_censored_whole_iterations_match_the_oracle_on_both_paths(chains, n_modes, with_feat, alpha_sample):
    ids, y, c, dims, D, feats, n_test, alpha, _ = CR.iteration_case(n_modes, with_feat, alpha_sample)
    key = "%d%d%d_" % (n_modes, with_feat, alpha_sample)
    nat, step = ({k[len(key):]: v for k, v in ch.items() if k.startswith(key)} for ch in chains)
    assert nat["native"] == 1 and step["native"] == 0
    assert sorted(nat) == sorted(step) and len(nat) >= 4 + 3 * n_modes
    for k in nat:
        if k != "native":
            assert np.array_equal(nat[k], step[k]), k       # the two paths enqueue the same launches: the same bits
    ref = CR.run_chain(ids[n_test:], y[n_test:], c[n_test:], dims, D, 91, 2, alpha=alpha, alpha_sample=alpha_sample, feats=feats,
                       test_ids=ids[:n_test], burnin=1)
    tol = dict(rtol=1e-6, atol=1e-6)
    assert abs(nat["mean"] - ref["mean"]) <= 1e-12
    np.testing.assert_allclose(nat["alpha"], ref["alpha"], rtol=1e-6)
    assert (nat["alpha"] != alpha) == bool(alpha_sample)
    for k in range(n_modes):
        np.testing.assert_allclose(nat["S%d" % k], ref["S"][k], err_msg="sample of entity %d" % k, **tol)
        np.testing.assert_allclose(nat["mu%d" % k], ref["mu"][k], **tol)
        np.testing.assert_allclose(nat["Lam%d" % k], ref["Lam"][k], **tol)
        if feats[k] is not None:
            np.testing.assert_allclose(nat["beta%d" % k], ref["beta"][k], rtol=1e-5, atol=1e-6, err_msg="beta of entity %d" % k)
            assert abs(nat["lb%d" % k] - ref["lb"][k]) <= 1e-5 * ref["lb"][k]
    np.testing.assert_allclose(nat["pred"], ref["pred"], **tol)
    # and the flags matter: the Gaussian chain on the same data is somewhere else
    gauss = CR.run_chain(ids[n_test:], y[n_test:], None, dims, D, 91, 2, alpha=alpha, alpha_sample=alpha_sample, feats=feats)
    assert np.abs(gauss["S"][0] - ref["S"][0]).max() > 1e-3


# ---- (c) all-zero flags are no flags -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha_sample", [False, True])
def test_all_zero_flags_run_the_chain_without_flags(B, alpha_sample):
    """With every flag 0 the rows see linear_values == mean_value, through the general row kernel k_rows' general gather instead
    of its lean one.  Both chains are forced onto that same path (Context.set_gather(1); D = 8 and entities this small take
    neither k_rows_small nor K1c), so they are compared at 1e-12, not at the 1e-9 two different row kernels would need."""
    ids, y, _, dims, D, _, n_test, alpha, _ = CR.iteration_case(2, False, alpha_sample)

    def run(flags):
        rel = B.Relation({"a": ids[:, 0], "b": ids[:, 1], "y": y}, "z", [B.Entity("a"), B.Entity("b")], alpha=alpha, dims=list(dims))
        rel.model.alpha_sample = alpha_sample
        B.assignToTest(rel, np.arange(1, n_test + 1))
        if flags:
            B.setCensored(rel, np.zeros(len(y) - n_test, dtype=np.int8))
        rd = B.RelationData(rel)
        eng = B.GibbsEngine(rd, D, seed=23)
        eng.ctx.set_gather(1)
        for it in (1, 2, 3):
            eng.sweep(it)
        eng.sync()
        eng.sync_host_scalars()
        out = [en.model.sample.copy() for en in rd.entities] + [np.array(rel.model.alpha)]
        lin = None if eng.rel[0].linear is None else eng.rel[0].linear.cpu().numpy()
        mean = rel.model.mean_value
        eng.close()
        return out, lin, mean

    with_flags, lin, mean = run(True)
    without, none, _ = run(False)
    assert none is None and np.all(lin == mean)             # exact observations: linear is mean_value bit for bit
    for a, b in zip(with_flags, without):
        assert np.abs(a - b).max() <= 1e-12
    assert (with_flags[2] != alpha) == alpha_sample


# ---- (d) nothing else moved --------------------------------------------------------------------------------------------------
def test_gaussian_chain_is_untouched_by_a_censored_engine_in_the_process(B):
    ids, y, c, n_test = CR.planted(seed=5, N1=120, N2=90, n_cells=4000, n_test=500)

    def gaussian():
        rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y + 0.25 * ids[:, 0] % 3}, "g", [B.Entity("u"), B.Entity("v")], dims=[120, 90])
        B.assignToTest(rel, np.arange(4000 - n_test + 1, 4001))
        rd = B.RelationData(rel)
        res = B.macau(rd, num_latent=16, burnin=2, psamples=2, verbose=False, seed=17)
        out = [en.model.sample.copy() for en in rd.entities] + [res["predictions"]["pred"].to_numpy().copy()]
        rd._engine.close()
        return out

    alone = gaussian()
    rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "p", [B.Entity("u"), B.Entity("v")], dims=[120, 90])
    B.assignToTest(rel, np.arange(4000 - n_test + 1, 4001))
    B.setCensored(rel, c[:-n_test])
    rdc = B.RelationData(rel)
    B.macau(rdc, num_latent=16, burnin=1, psamples=1, verbose=False, seed=17)
    beside = gaussian()                                     # the censored engine is alive: its pairs carry the baseline, its relation the flags
    assert rdc._engine.gibbs is not None or not rdc._engine.native
    for a, b in zip(alone, beside):
        assert np.array_equal(a, b)
    rdc._engine.close()


# ---- (e) quality --------------------------------------------------------------------------------------------------------------
def test_censored_quality_on_planted_data(B):
    """Planted data (rank 4, 300 x 200, 12,000 cells, noise precision 4, 3,000 exact cells held out; training values above 0.5
    reported as ">= 0.5", below -3 as "<= -3": 47 % of the training cells are bounds).  macau() with D = 8, 30 + 30 iterations and
    alpha = 4.  The yardstick for the held-out RMSE is the CPU restatement of the same sampler with three other seeds: the
    device's RMSE must be at most the largest of the three plus their spread (max - min), the seed-to-seed noise of the
    estimator, and below the device's own RMSE with the flags left off (bounds taken as values)."""
    ids, y, c, n_test = CR.planted()
    D, burnin, psamples, alpha = 8, 30, 30, 4.0
    held = y[-n_test:]

    def device(flags):
        rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "planted", [B.Entity("u"), B.Entity("v")], alpha=alpha, dims=[300, 200])
        B.assignToTest(rel, np.arange(12000 - n_test + 1, 12001))
        if flags:
            B.setCensored(rel, c[:-n_test])
        rd = B.RelationData(rel)
        res = B.macau(rd, num_latent=D, burnin=burnin, psamples=psamples, verbose=False, seed=1)
        pred = res["predictions"]["pred"].to_numpy()
        rd._engine.close()
        assert abs(res["RMSE"] - np.sqrt(np.mean((held - pred) ** 2))) <= 1e-9
        return float(res["RMSE"])

    assert 0.45 <= np.mean(c[:-n_test] != 0) <= 0.48
    rmse_dev, rmse_off = device(True), device(False)
    cpu = []
    for seed in (2, 3, 4):
        ref = CR.run_chain(ids[:-n_test], y[:-n_test], c[:-n_test], [300, 200], D, seed, burnin + psamples, alpha=alpha,
                           test_ids=ids[-n_test:], burnin=burnin)
        cpu.append(float(np.sqrt(np.mean((held - ref["pred"]) ** 2))))
    print(f"censored quality: device RMSE {rmse_dev:.4f}; CPU restatement RMSE {cpu[0]:.4f} {cpu[1]:.4f} {cpu[2]:.4f}; "
          f"device with the flags left off: RMSE {rmse_off:.4f}")
    assert rmse_dev <= max(cpu) + (max(cpu) - min(cpu)), (rmse_dev, cpu)
    assert rmse_dev < rmse_off, (rmse_dev, rmse_off)


# ---- (f) errors through the C ABI ---------------------------------------------------------------------------------------------
def test_censored_c_abi_errors(B, ctx):
    import torch
    from bdf_amd._lib import GibbsRelation, check, lib
    ids, y, c, n_test = CR.planted(seed=9, N1=60, N2=50, n_cells=1500, n_test=0)
    rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "e", [B.Entity("u"), B.Entity("v")], dims=[60, 50])
    eng = B.GibbsEngine(B.RelationData(rel), 8, seed=3)
    assert eng.native
    train = B.DevicePairs(eng.ctx, ids, y)
    op = B.FeatOperator(eng.ctx, np.ones((len(y), 2)))
    lin, beta, alpha = eng.ctx.tensor(np.full(len(y), rel.model.mean_value)), eng.ctx.zeros(2), eng.ctx.tensor([1.0])
    cd = eng.ctx.tensor(c, dtype=torch.int8)
    check(lib().bdf_pairs_set_baseline(train.handle, _p(lin)))

    def record(**kw):
        arr = (GibbsRelation * 1)()
        g = arr[0]
        g.rel, g.mean_value, g.alpha_dev, g.rel_tag, g.nnz = eng.rel[0].handle, rel.model.mean_value, alpha.data_ptr(), 1, len(y)
        g.entity_of_mode[0], g.entity_of_mode[1] = 0, 1
        g.train, g.first_obs, g.obs_block, g.linear, g.censor = train.handle, 0, len(y), lin.data_ptr(), cd.data_ptr()
        for k, v in kw.items():
            setattr(g, k, v)
        return arr

    def register(arr):
        check(lib().bdf_gibbs_set_relations(eng.gibbs, 1, C.cast(arr, C.c_void_p)))

    with pytest.raises(B.ArgumentError, match="censored"):
        register(record(probit=1))
    with pytest.raises(B.ArgumentError, match="censored"):
        register(record(feat=op.handle, beta=beta.data_ptr()))
    with pytest.raises(B.ArgumentError, match="censored"):
        register(record(linear=None))
    with pytest.raises(B.ArgumentError, match="censored"):
        register(record(train=None))
    facs = _facs(eng.factors_of(rel))

    def draw(train_h=train.handle, censor=cd, D=8, fp=facs, a=1.0, a_dev=None, out=lin):
        check(lib().bdf_censored_draw(eng.ctx.handle, train_h, _p(censor), D, fp, 0.0, a, _p(a_dev), 1, _p(out), None))

    for bad in (dict(train_h=None), dict(censor=None), dict(fp=None), dict(out=None), dict(D=0), dict(D=65), dict(a=0.0), dict(a=-1.0),
                dict(a=float("nan")), dict(a=float("inf"))):
        with pytest.raises(B.ArgumentError, match="bdf_censored_draw"):
            draw(**bad)
    draw(a=0.0, a_dev=alpha)                                 # alpha_dev wins over the scalar
    register(record())                                       # and the well-formed record is accepted: one iteration runs
    eng.sweep(1)
    eng.sync()
    assert np.all(np.isfinite(rel.entities[0].model.sample))
    l = lin.cpu().numpy()
    assert np.all(l[c == 0] == rel.model.mean_value) and np.all((l - rel.model.mean_value)[c > 0] <= 0) and np.all((l - rel.model.mean_value)[c < 0] >= 0)
    op.close()
    train.close()
    eng.close()
