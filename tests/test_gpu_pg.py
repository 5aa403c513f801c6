"""The Polya-Gamma noise models on the GPU: bdf_pg_draw against the restatement (tests/pg_restatement.py), the
logistic and the count link of the prediction kernels against numpy, whole macau() iterations against the restated chain on both
iteration paths, the Gaussian chain untouched by a logit / count engine in the same process, planted counts and planted 0/1 data,
and the errors of the C ABI."""
import ctypes as C
import os
import textwrap

import numpy as np
import pytest

from both_paths import child
import pg_restatement as PG

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1234                      # the seed of the shared context (conftest.py)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _facs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


# ---- (a) the draw ---------------------------------------------------------------------------------------------------------------
def _draw_problem(rng, n_modes, D):
    """N = 40 rows, other modes 23 (and 11), n = 1003 observations (not a multiple of 8), some cells many times over; the factors
    scaled so that |udot| reaches 45: psi runs from ~0 to beyond 40 in both directions"""
    dims = [40, 23, 11][:n_modes]
    n = 1003
    ids = np.stack([rng.integers(1, d + 1, n) for d in dims], axis=1)
    ids[1::7] = ids[0]
    S = [rng.standard_normal((d, D)) for d in dims]
    S[0] *= 45.0 / np.abs(PG.udot(ids, S)).max()
    return dims, n, ids, S


def _count_values(rng, n, r):
    """counts with mean ~3, and among them 0, b = y + r on both sides of 170, 1e4 and 1e6"""
    y = rng.poisson(rng.gamma(3.0, 1.0, n)).astype(np.float64)
    y[:8] = [0.0, 169.0 - r, 170.0 - r, 171.0 - r, 1e4, 1e6, 0.0, 172.0 - r]
    y[500:503] = [170.0 - r, 171.0 - r, 1e4]
    return y


@pytest.mark.parametrize("sort", [False, True])
@pytest.mark.parametrize("n_modes", [2, 3])
@pytest.mark.parametrize("D", [1, 7, 10, 32, 64])
def test_pg_draw_matches_the_restatement(B, ctx, D, n_modes, sort):
    """omega at 1e-9 relative and linear_out at 1e-9 relative / 1e-6, no cell excluded, and the same bits from two launches.  A flipped
    accept / reject decision would give another omega outright: every case draws at the first sweep number (from a fixed start) at
    which the restatement's smallest decision margin over all cells is above 1e-6 -- found here, on the CPU, before the launch."""
    from bdf_amd._lib import check, lib
    rng = np.random.default_rng(3000 + 100 * D + 10 * n_modes + sort)
    dims, n, ids, S = _draw_problem(rng, n_modes, D)
    St = [ctx.tensor(s) for s in S]
    mean = 0.3
    psi = PG.udot(ids, S) + mean
    assert np.abs(psi).max() >= 40.0
    sweep, worst, worst_l = 10, 0.0, 0.0
    for model, r in ((1, 0), (2, 1), (2, 5)):
        y = (rng.random(n) < 0.5).astype(np.float64) if model == 1 else _count_values(rng, n, r)
        pairs = B.DevicePairs(ctx, ids, y)
        if sort:
            pairs.sort(n_modes - 1)
        b, kappa = PG.b_of(model, y, r), PG.kappa_of(model, y, r)
        tag = 1 + model
        for sweep in range(sweep + 1, sweep + 40):
            ref, mg = PG.draw_pg(psi, b, SEED, sweep, tag)
            if mg.min() > 1e-6:
                break
        else:
            raise AssertionError("no sweep with every decision margin above 1e-6")
        om, om2, lin, lin2 = (ctx.tensor(np.full(n, np.nan)) for _ in range(4))
        ctx.set_sweep(sweep)
        check(lib().bdf_pg_draw(ctx.handle, pairs.handle, D, _facs(St), mean, model, float(r), tag, _p(om), _p(lin)))
        check(lib().bdf_pg_draw(ctx.handle, pairs.handle, D, _facs(St), mean, model, float(r), tag, _p(om2), _p(lin2)))
        ctx.sync()
        om, om2, lin, lin2 = (t.cpu().numpy() for t in (om, om2, lin, lin2))
        assert np.all(np.isfinite(om)) and np.all(om > 0) and np.all(np.isfinite(lin))
        err = np.abs(om / ref - 1.0)
        ref_l = PG.linear_of(mean, y, kappa, ref)
        err_l = np.abs(lin - ref_l) / (1e-9 * np.abs(ref_l) + 1e-6)
        worst, worst_l = max(worst, err.max()), max(worst_l, err_l.max())
        assert err.max() <= 1e-9, (model, r, sweep, int(np.argmax(err)), err.max(), float(mg.min()))
        assert err_l.max() <= 1.0, (model, r, sweep, int(np.argmax(err_l)))
        assert np.array_equal(om, om2) and np.array_equal(lin, lin2)
        pairs.close()
    print(f"pg draw D={D} modes={n_modes} sort={sort}: max rel. error of omega {worst:.3e}, linear at {worst_l:.3e} of its tolerance, 3 models")


def test_pg_draw_is_finite_at_the_extremes(B, ctx):
    """psi in {0, +-1e-8, +-40, +-100, +-2000, +-1e4} through the kernel: omega finite and positive, linear finite, for the logit
    model, counts below and above b = 170"""
    from bdf_amd._lib import check, lib
    psi = np.array([0.0, 1e-8, -1e-8, 40.0, -40.0, 100.0, -100.0, 2000.0, -2000.0, 1e4, -1e4])
    n = len(psi)
    ids = np.stack([np.arange(1, n + 1), np.ones(n, dtype=np.int64)], axis=1)
    St = [ctx.tensor(psi[:, None]), ctx.tensor(np.ones((1, 1)))]
    ctx.set_sweep(8)
    for model, r, y in ((1, 0, 1.0), (1, 0, 0.0), (2, 3, 0.0), (2, 3, 166.0), (2, 3, 1e6)):
        pairs = B.DevicePairs(ctx, ids, np.full(n, y))
        om, lin = ctx.tensor(np.full(n, np.nan)), ctx.tensor(np.full(n, np.nan))
        check(lib().bdf_pg_draw(ctx.handle, pairs.handle, 1, _facs(St), 0.0, model, float(r), 1, _p(om), _p(lin)))
        ctx.sync()
        om, lin = om.cpu().numpy(), lin.cpu().numpy()
        assert np.all(np.isfinite(om)) and np.all(om > 0) and np.all(np.isfinite(lin)), (model, y, om, lin)
        ref, mg = PG.draw_pg(psi, PG.b_of(model, np.full(n, y), r), SEED, 8, 1)
        ok = mg > 1e-6
        np.testing.assert_allclose(om[ok], ref[ok], rtol=1e-9)
        pairs.close()


# ---- (b) the links ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_modes,D,sort", [(2, 32, True), (2, 10, False), (3, 8, False), (2, 64, True), (3, 7, True)])
def test_links_of_the_prediction_kernels(B, ctx, n_modes, D, sort):
    """links 2 and 3 against numpy at 1e-12 through bdf_predict and the running update, psi = +-800 included; links 0 and 1 are what
    they were: a set of pairs that carried the new links and went back predicts the bits of one that never had a link set.

    How "against numpy at 1e-12" is read here: the bound of 1e-12 is on the link itself -- numpy's link applied to the psi that the
    identity link's kernel returns for the same pairs (`base`) -- and `base` in turn is held to numpy's own psi at 1e-12 (relative and
    absolute).  numpy's link of numpy's own psi is held at 1e-9 only: psi is a sum of D products whose rounding differs between the
    kernel's order of summation and numpy's by a few ulp of the largest term, and r e^psi carries an ABSOLUTE error d of psi over as
    the RELATIVE error d -- one ulp of psi at |psi| = 800 is 1.1e-13, a handful reach 1e-12 -- so 1e-12 on that path would
    test the order of a dot product's additions, not the link."""
    from bdf_amd._lib import check, lib
    rng = np.random.default_rng(4000 + 10 * D + n_modes)
    dims = [40, 23, 11][:n_modes]
    n = 1003
    ids = np.stack([rng.integers(1, d + 1, n) for d in dims], axis=1)
    S = [0.5 * rng.standard_normal((d, D)) for d in dims]
    # two cells whose udot is exactly +-800: rows of their own with one non-zero entry
    for k in range(n_modes):
        S[k][0] = 0.0
        S[k][1] = 0.0
        S[k][0, 0] = S[k][1, 0] = 1.0
    S[0][0, 0], S[0][1, 0] = 800.0, -800.0
    ids[0], ids[1] = 1, 2
    ids[2:, :] = np.maximum(ids[2:, :], 3)
    St = [ctx.tensor(s) for s in S]
    y = rng.poisson(3.0, n).astype(np.float64)
    mean, r = 0.2, 5.0
    psi = PG.udot(ids, S) + mean
    assert psi[0] == 800.2 and psi[1] == -799.8

    def pairs_of(link):
        p = B.DevicePairs(ctx, ids, y)
        if sort:
            p.sort(n_modes - 1)
        if link in (2, 3):
            p.set_pg_link(link - 1, r)
        elif link is not None:
            p.set_link(link)
        return p

    plain = pairs_of(None)
    base = plain.predict(D, St, mean).cpu().numpy()
    np.testing.assert_allclose(base, psi, rtol=1e-12, atol=1e-12)
    for link, model in ((2, 1), (3, 2)):
        p = pairs_of(link)
        got = p.predict(D, St, mean).cpu().numpy()
        ref = PG.link(model, base, r)                          # (the link of the kernel's own psi: the gather is k_predict's)
        assert np.all(np.isfinite(got))
        np.testing.assert_allclose(got, ref, rtol=1e-12, atol=0)
        np.testing.assert_allclose(got, PG.link(model, psi, r), rtol=1e-9, atol=0)
        assert got[1] == 0.0 and (got[0] == 1.0 if link == 2 else got[0] > 1e300)
        # the running update: the average of two updates and the statistics of the last sample
        for phase in (0, 1, 2):
            st = p.update(D, St, mean, phase, [], 0.5)
            ctx.sync()
            st = st.cpu().numpy().copy()
        avg, sq = p.state()
        np.testing.assert_allclose(avg, ref, rtol=1e-12)
        with np.errstate(over="ignore"):
            np.testing.assert_allclose(sq[2:], 2.0 * ref[2:] ** 2, rtol=1e-12)
        if link == 2:                                          # (the squared error of the count link at psi = 800 is e^1400: not finite)
            np.testing.assert_allclose(st[1], np.sum((y - ref) ** 2), rtol=1e-10)
        # back to the identity, and to the probit link: what a set of pairs without this history gives, bit for bit
        p.set_link(0)
        assert np.array_equal(p.predict(D, St, mean).cpu().numpy(), base)
        p.set_link(1)
        probit = pairs_of(1)
        assert np.array_equal(p.predict(D, St, mean).cpu().numpy(), probit.predict(D, St, mean).cpu().numpy())
        probit.close()
        p.close()
    plain.close()


# ---- (c) whole iterations ---------------------------------------------------------------------------------------------------------
CASES = [(model, n_modes, with_feat) for model in (1, 2) for n_modes in (2, 3) for with_feat in (0, 1)]
CHAIN_SEED = 91

CHILD = textwrap.dedent('''
    import sys
    import numpy as np
    sys.path.insert(0, %r); sys.path.insert(0, %r)
    import bdf_amd as B
    import pg_restatement as PG
    out, d = sys.argv[1], {}
    for model in (1, 2):
        for n_modes in (2, 3):
            for with_feat in (0, 1):
                ids, y, dims, D, feats, n_test, r, offset = PG.iteration_case(n_modes, with_feat, model)
                names = ["a", "b", "c"][:n_modes]
                ents = [B.Entity(nm, F=feats[k]) for k, nm in enumerate(names)]
                table = {nm: ids[:, k] for k, nm in enumerate(names)}
                table["y"] = y
                rel = B.Relation(table, "pg", ents, dims=list(dims))
                B.assignToTest(rel, np.arange(1, n_test + 1))
                B.setLogit(rel, offset=offset) if model == 1 else B.setCounts(rel, r, offset=offset)
                rd = B.RelationData(rel)
                res = B.macau(rd, num_latent=D, burnin=3, psamples=3, verbose=False, seed=%d)
                key = "m%%d%%d%%d_" %% (model, n_modes, with_feat)
                eng = rd._engine
                d[key + "native"], d[key + "pred"] = np.array(int(eng.native)), res["predictions"]["pred"].to_numpy()
                d[key + "mean"], d[key + "alpha"] = np.array(rel.model.mean_value), np.array(rel.model.alpha)
                d[key + "k1"] = np.array([eng.rows_dispatch(j)["k1"] for j in range(n_modes)])
                d[key + "omega"], d[key + "linear"] = eng.rel[0].omega.cpu().numpy(), eng.rel[0].linear.cpu().numpy()
                d[key + "rmse"], d[key + "roc"] = np.array(res["RMSE"]), np.array(res["ROC"])
                for k, en in enumerate(rd.entities):
                    d[key + "S%%d" %% k], d[key + "mu%%d" %% k], d[key + "Lam%%d" %% k] = en.model.sample.T, en.model.mu, en.model.Lambda
                    if feats[k] is not None:
                        d[key + "beta%%d" %% k], d[key + "lb%%d" %% k] = en.model.beta, np.array(en.lambda_beta)
                eng.close()
    np.savez(out, **d)
''') % (ROOT, os.path.join(ROOT, "tests"), CHAIN_SEED)


@pytest.fixture(scope="module")
def chains():
    """six iterations of every case of CASES on the native and on the step-by-step path: one child process per path"""
    return child(CHILD, no_native=False), child(CHILD, no_native=True)


@pytest.mark.parametrize("model,n_modes,with_feat", CASES)
def test_whole_iterations_match_the_restated_chain_on_both_paths(chains, model, n_modes, with_feat):
    ids, y, dims, D, feats, n_test, r, offset = PG.iteration_case(n_modes, with_feat, model)
    key = "m%d%d%d_" % (model, n_modes, with_feat)
    nat, step = ({k[len(key):]: v for k, v in ch.items() if k.startswith(key)} for ch in chains)
    assert nat["native"] == 1 and step["native"] == 0
    assert sorted(nat) == sorted(step) and len(nat) >= 9 + 3 * n_modes
    for k in nat:
        if k != "native":
            assert np.array_equal(nat[k], step[k], equal_nan=True), k       # the two paths enqueue the same launches: the same bits (counts have no class: ROC is NaN)
    assert np.array_equal(nat["k1"], dims)                  # every row of every entity by the wave-per-row kernel (k_rows_w)
    ref = PG.run_chain(ids[n_test:], y[n_test:], dims, D, CHAIN_SEED, 6, model, r=r, offset=offset, feats=feats, test_ids=ids[:n_test], burnin=3)
    assert ref["margin"] > 1e-6, ref["margin"]              # (no decision of the restated chain was a close call)
    tol = dict(rtol=1e-6, atol=1e-6)
    assert nat["mean"] == offset and nat["alpha"] == 1.0
    for k in range(n_modes):
        np.testing.assert_allclose(nat["S%d" % k], ref["S"][k], err_msg="sample of entity %d" % k, **tol)
        np.testing.assert_allclose(nat["mu%d" % k], ref["mu"][k], **tol)
        np.testing.assert_allclose(nat["Lam%d" % k], ref["Lam"][k], **tol)
        if feats[k] is not None:
            np.testing.assert_allclose(nat["beta%d" % k], ref["beta"][k], rtol=1e-5, atol=1e-6, err_msg="beta of entity %d" % k)
            assert abs(nat["lb%d" % k] - ref["lb"][k]) <= 1e-5 * ref["lb"][k]
    np.testing.assert_allclose(nat["pred"], ref["pred"], **tol)
    n_train = len(y) - n_test
    np.testing.assert_allclose(nat["omega"][:n_train], ref["omega"], rtol=1e-6)
    np.testing.assert_allclose(nat["linear"][:n_train], ref["linear"], **tol)
    assert abs(nat["rmse"] - np.sqrt(np.mean((y[:n_test] - ref["pred"]) ** 2))) <= 1e-6
    if model == 1:
        assert np.all((nat["pred"] > 0.0) & (nat["pred"] < 1.0)) and 0.0 <= nat["roc"] <= 1.0


# ---- (d) nothing else moved --------------------------------------------------------------------------------------------------------
def test_gaussian_chain_is_untouched_by_a_pg_engine_in_the_process(B):
    ids, y, psi, n_test = PG.planted("counts", seed=5, N1=120, N2=90, n_cells=4000, n_test=500)

    def gaussian():
        rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y + 0.25 * ids[:, 0] % 3}, "g", [B.Entity("u"), B.Entity("v")], dims=[120, 90])
        B.assignToTest(rel, np.arange(4000 - n_test + 1, 4001))
        rd = B.RelationData(rel)
        res = B.macau(rd, num_latent=16, burnin=2, psamples=2, verbose=False, seed=17)
        out = [en.model.sample.copy() for en in rd.entities] + [res["predictions"]["pred"].to_numpy().copy()]
        assert rd._engine.rel[0].omega is None and rd._engine.rel[0].linear is None and rd._engine.rel[0].pg_model == 0
        rd._engine.close()
        return out

    alone = gaussian()
    engines = []
    for kind in ("counts", "logit"):
        rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y if kind == "counts" else (y > 2).astype(float)}, "p",
                         [B.Entity("u"), B.Entity("v")], dims=[120, 90])
        B.assignToTest(rel, np.arange(4000 - n_test + 1, 4001))
        B.setCounts(rel, 5) if kind == "counts" else B.setLogit(rel)
        rd = B.RelationData(rel)
        res = B.macau(rd, num_latent=16, burnin=1, psamples=1, verbose=False, seed=17, rmse_train=True)
        om = rd._engine.rel[0].omega.cpu().numpy()
        assert np.all(np.isfinite(om)) and np.all(om > 0) and np.isfinite(res["RMSE"])
        engines.append(rd._engine)
    beside = gaussian()                                     # the logit and the count engine are alive
    for a, b in zip(alone, beside):
        assert np.array_equal(a, b)
    for e in engines:
        e.close()


# ---- (e) planted data ---------------------------------------------------------------------------------------------------------------
def _auc(p, lab):
    order = np.argsort(p, kind="stable")
    ranks = np.empty(len(p))
    ranks[order] = np.arange(1, len(p) + 1)
    return (ranks[lab].sum() - lab.sum() * (lab.sum() + 1) / 2) / (lab.sum() * (~lab).sum())


PLANTED_COUNTS = dict(scale=0.7, shift=-0.5)
PLANTED_LOGIT = dict(scale=1.5, shift=0.0)
CPU_WORST_RATIO = 0.395         # the restated chains' worst RMSE(counts) / RMSE(Gaussian) over planted seeds 0, 1, 2
CPU_WORST_AUC = 0.7945          # ... and their worst held-out AUC on the planted 0/1 data


def test_planted_counts(B):
    """150 x 100, rank 3, negative-binomial counts with r = 5 and mean 5 e^psi*, 5,000 cells of which 1,500 are held out and scored
    against the true mean 5 e^psi*.  D = 4, 30 + 50 iterations, the same seed for both models; the Gaussian model on the raw counts
    samples its precision.  The bound: twice the worst ratio RMSE(counts) / RMSE(Gaussian) that the restated chains gave on the CPU
    for planted seeds 0, 1, 2 (DESIGN.md section 19 has the table)."""
    ids, y, psi, n_test = PG.planted("counts", seed=0, **PLANTED_COUNTS)
    n = len(y)
    truth = 5.0 * np.exp(psi[-n_test:])

    def run(counts):
        rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "planted", [B.Entity("u"), B.Entity("v")], dims=[150, 100])
        B.assignToTest(rel, np.arange(n - n_test + 1, n + 1))
        if counts:
            B.setCounts(rel, 5)
        else:
            rel.model.alpha_sample = True
        rd = B.RelationData(rel)
        res = B.macau(rd, num_latent=4, burnin=30, psamples=50, verbose=False, seed=1)
        pred = res["predictions"]["pred"].to_numpy()
        rd._engine.close()
        assert abs(res["RMSE"] - np.sqrt(np.mean((y[-n_test:] - pred) ** 2))) <= 1e-9 * max(res["RMSE"], 1.0)
        return float(np.sqrt(np.mean((pred - truth) ** 2)))

    rmse_c, rmse_g = run(True), run(False)
    print(f"planted counts: RMSE against the true mean: count model {rmse_c:.4f}, Gaussian {rmse_g:.4f}, ratio {rmse_c / rmse_g:.3f}")
    assert CPU_WORST_RATIO <= 0.5
    assert rmse_c <= 2.0 * CPU_WORST_RATIO * rmse_g, (rmse_c, rmse_g)


def test_planted_logit(B):
    """planted logistic data of the same shape: y ~ Bernoulli(sigma(psi*)).  Held-out AUC at least the worst of the restated chains on
    the CPU (planted seeds 0, 1, 2) minus 0.02, and a Brier score below that of the constant predictor (the training base rate)"""
    ids, y, psi, n_test = PG.planted("logit", seed=0, **PLANTED_LOGIT)
    n = len(y)
    rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "planted", [B.Entity("u"), B.Entity("v")], dims=[150, 100])
    B.assignToTest(rel, np.arange(n - n_test + 1, n + 1))
    B.setLogit(rel)
    rd = B.RelationData(rel)
    res = B.macau(rd, num_latent=4, burnin=30, psamples=50, verbose=False, seed=1)
    pred = res["predictions"]["pred"].to_numpy()
    rd._engine.close()
    held = y[-n_test:]
    auc = _auc(pred, held > 0.5)
    brier, const = np.mean((pred - held) ** 2), np.mean((y[:n - n_test].mean() - held) ** 2)
    print(f"planted logit: held-out AUC {auc:.4f} (the library's ROC {res['ROC']:.4f}), Brier {brier:.4f} against {const:.4f} of the constant predictor")
    assert np.all((pred >= 0.0) & (pred <= 1.0))
    assert abs(res["ROC"] - auc) <= 1e-6
    assert auc >= CPU_WORST_AUC - 0.02
    assert brier < const


# ---- (f) errors through the C ABI ---------------------------------------------------------------------------------------------------
def test_pg_c_abi_errors(B, ctx):
    import torch
    from bdf_amd._lib import GibbsRelation, check, lib
    ids, y, psi, n_test = PG.planted("counts", seed=9, N1=60, N2=50, n_cells=1500, n_test=0)
    rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "e", [B.Entity("u"), B.Entity("v")], dims=[60, 50])
    eng = B.GibbsEngine(B.RelationData(rel), 8, seed=3)
    assert eng.native
    n = len(y)
    train = B.DevicePairs(eng.ctx, ids, y)
    op = B.FeatOperator(eng.ctx, np.ones((n, 2)))
    lin, beta, alpha = eng.ctx.tensor(np.zeros(n)), eng.ctx.zeros(2), eng.ctx.tensor([1.0])
    om = eng.ctx.tensor(np.ones(n))
    flags = eng.ctx.tensor(np.zeros(n, dtype=np.int8), dtype=torch.int8)
    bounds = eng.ctx.tensor(np.stack([y, y], axis=1))

    def record(**kw):
        arr = (GibbsRelation * 1)()
        g = arr[0]
        g.rel, g.mean_value, g.alpha_dev, g.rel_tag, g.nnz = eng.rel[0].handle, 0.0, alpha.data_ptr(), 1, n
        g.entity_of_mode[0], g.entity_of_mode[1] = 0, 1
        g.train, g.first_obs, g.obs_block, g.obs_precision, g.linear = train.handle, 0, n, om.data_ptr(), lin.data_ptr()
        g.pg_model, g.pg_r = 2, 5.0
        for k, v in kw.items():
            setattr(g, k, v)
        return arr

    def register(arr):
        check(lib().bdf_gibbs_set_relations(eng.gibbs, 1, C.cast(arr, C.c_void_p)))

    for bad in (dict(probit=1), dict(censor=flags.data_ptr()), dict(interval=bounds.data_ptr()), dict(robust_nu=4.0),
                dict(feat=op.handle, beta=beta.data_ptr()), dict(alpha_sample=1, alpha_lambda0=1.0, alpha_nu0=2.0)):
        for model in (1, 2):
            with pytest.raises(B.ArgumentError):
                register(record(pg_model=model, **bad))
    # ... the ordinal model: a whole ordinal record (edges, levels, the interval model's bounds), and the edges alone
    edges = B.DeviceOrdinal(eng.ctx, 5)
    codes = eng.ctx.tensor(np.ones(n, dtype=np.int8), dtype=torch.int8)
    for bad in (dict(ordinal=edges.handle, ordinal_codes=codes.data_ptr(), interval=bounds.data_ptr()), dict(ordinal=edges.handle),
                dict(ordinal=edges.handle, ordinal_codes=codes.data_ptr())):
        for model in (1, 2):
            with pytest.raises(B.ArgumentError):
                register(record(pg_model=model, **bad))
    # ... and a communicator on the sampler (one rank of one, over a host exchange that is never called)
    from bdf_amd._lib import EXCHANGE_FN
    exchange = EXCHANGE_FN(lambda user, send, recv, nbytes: 1)
    comm = C.c_void_p()
    check(lib().bdf_comm_create_host(eng.ctx.handle, 0, 1, exchange, None, C.byref(comm)))
    check(lib().bdf_gibbs_set_comm(eng.gibbs, comm))
    try:
        for model in (1, 2):
            with pytest.raises(B.ArgumentError, match="rank|communicator"):
                register(record(pg_model=model))
    finally:
        check(lib().bdf_gibbs_set_comm(eng.gibbs, None))
        check(lib().bdf_comm_destroy(comm))
    for bad in (dict(pg_model=3), dict(pg_model=-1), dict(pg_r=0.0), dict(pg_r=2.5), dict(pg_r=-1.0), dict(pg_r=float("nan")),
                dict(obs_precision=None), dict(linear=None), dict(train=None)):
        with pytest.raises(B.ArgumentError, match="pg_|Polya-Gamma"):
            register(record(**bad))
    facs = _facs(eng.factors_of(rel))

    def draw(train_h=train.handle, D=8, fp=facs, model=2, r=5.0, out=om, lout=lin, mean=0.0):
        check(lib().bdf_pg_draw(eng.ctx.handle, train_h, D, fp, mean, model, r, 1, _p(out), _p(lout)))

    for bad in (dict(train_h=None), dict(fp=None), dict(out=None), dict(lout=None), dict(D=0), dict(D=65), dict(model=0), dict(model=3),
                dict(model=-1), dict(r=0.0), dict(r=0.5), dict(r=2.5), dict(r=-1.0), dict(r=float("nan")), dict(r=float("inf")),
                dict(mean=float("nan"))):
        with pytest.raises(B.ArgumentError, match="bdf_pg_draw"):
            draw(**bad)
    draw(model=1, r=0.0)                                     # the logit model does not read r
    with pytest.raises(B.ArgumentError, match="link"):
        check(lib().bdf_pairs_set_link(train.handle, 3))     # the count link and the logistic link have setters of their own
    with pytest.raises(B.ArgumentError, match="link"):
        check(lib().bdf_pairs_set_link(train.handle, 2))
    with pytest.raises(B.ArgumentError, match="bdf_pairs_set_logistic_link"):
        check(lib().bdf_pairs_set_logistic_link(None))
    with pytest.raises(B.ArgumentError, match="link"):
        check(lib().bdf_pairs_set_link(train.handle, 4))
    for r in (0.0, 1.5, -2.0, float("nan")):
        with pytest.raises(B.ArgumentError, match="bdf_pairs_set_count_link"):
            check(lib().bdf_pairs_set_count_link(train.handle, r))
    with pytest.raises(B.ArgumentError, match="bdf_pairs_set_count_link"):
        check(lib().bdf_pairs_set_count_link(None, 2.0))
    # lpd and WAIC refuse pairs with the new links
    fs = eng.factors_of(rel)
    for setter in (lambda: train.set_pg_link(1), lambda: train.set_pg_link(2, 5.0)):
        setter()
        with pytest.raises(B.ArgumentError, match="not scored yet"):
            train.lpd_update(8, fs, 0.0, 1.0, 0)
        with pytest.raises(B.ArgumentError, match="not scored yet"):
            train.waic_update(8, fs, 0.0, 1.0, 0)
    train.set_link(0)
    register(record())                                       # and the well-formed record is accepted: one iteration runs
    eng.sweep(1)
    eng.sync()
    assert np.all(np.isfinite(rel.entities[0].model.sample))
    w, l = om.cpu().numpy(), lin.cpu().numpy()
    assert np.all(np.isfinite(w)) and np.all(w > 0) and w.std() > 0 and np.all(np.isfinite(l)) and float(alpha.item()) == 1.0
    op.close()
    train.close()
    eng.close()
