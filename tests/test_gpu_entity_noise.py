"""The per-row noise model on the GPU (setEntityNoise): bdf_entity_noise_draw against the restatement
(tests/entity_noise_restatement.py) with rows planted on the group boundaries of both widths, bdf_pairs_lpd_update with a precision
scale against tests/lpd_restatement.py fed a precision per cell, whole macau(lpd=True) iterations against the restated chain on both
iteration paths, the Gaussian chain untouched by a noise engine in the same process, the errors of the C ABI, and planted column
noise."""
import ctypes as C
import math
import os
import textwrap

import numpy as np
import pytest

from both_paths import child
import entity_noise_restatement as ER
import lpd_restatement as LR
from test_gpu_lpd import _bounds

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1234
COUNTS = (0, 1, 7, 8, 9, 63, 64, 65, 300)          # cells of the planted rows 0 .. 8: the group boundaries of the widths 8 and 64
N_CELLS = 1003                                       # not a multiple of 8 or of 256


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _facs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _planted_ids(rng, dims, mode):
    """N_CELLS cells; row r < 9 of `mode` has exactly COUNTS[r] of them, the other rows share the rest; in random order"""
    rest = N_CELLS - sum(COUNTS)
    col = np.concatenate([np.repeat(np.arange(1, len(COUNTS) + 1), COUNTS), rng.integers(len(COUNTS) + 1, dims[mode] + 1, rest)])
    col = rng.permutation(col)
    ids = np.stack([col if k == mode else rng.integers(1, d + 1, N_CELLS) for k, d in enumerate(dims)], axis=1).astype(np.int64)
    assert tuple(np.bincount(ids[:, mode] - 1, minlength=dims[mode])[:len(COUNTS)]) == COUNTS
    return ids


def _width(n, N):
    """the rule of the header: 8 lanes per row when the mean degree is at most 32, else 64"""
    return 8 if n <= 32 * N else 64


def _draw(ctx, dr, mode, pairs, D, St, mean, alpha, a_dev, shape, rate, tag, N, n, wsse=True):
    from bdf_amd._lib import check, lib
    tau, om = ctx.tensor(np.full(N, np.nan)), ctx.tensor(np.full(n, np.nan))
    s = ctx.tensor([np.nan]) if wsse else None
    check(lib().bdf_entity_noise_draw(ctx.handle, dr.handle, mode, pairs.handle, D, _facs(St), mean, alpha, _p(a_dev), shape, rate, tag,
                                      _p(tau), _p(om), _p(s)))
    ctx.sync()
    return tau.cpu().numpy(), om.cpu().numpy(), (float(s.item()) if wsse else None)


# ---- (a) the draw ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sort", [False, True])
@pytest.mark.parametrize("n_modes,mode", [(2, 0), (2, 1), (3, 0), (3, 1), (3, 2)])
@pytest.mark.parametrize("D", [1, 7, 32, 64])
def test_entity_noise_draw_matches_the_restatement(B, ctx, D, n_modes, mode, sort):
    """Two relations per case: dims [37, 23, 11][:n_modes], and the same with the noise mode's size changed so that the mean degree
    falls on the other side of 32 -- every (modes, mode, D) runs the 8-wide and the 64-wide row pass, each over rows of exactly 0, 1,
    7, 8, 9, 63, 64, 65 and 300 cells.  shape in {0.5, 2} (0.5: a row without cells draws through the boost branch), alpha as a
    scalar and through alpha_dev with a decoy scalar.

    Residuals are the device's own: e = y - bdf_predict on the same pairs (test_gpu_lpd.py argues why), which the first launch
    forms in that very order.  S_j is not an output; it is read off two draws of the same sweep -- the same G_j -- with rate = 2:
    alpha = 1e-300 gives tau = G / 2 exactly (alpha S / 2 vanishes beside 2), alpha = 2^40 gives tau = G / (2 + 2^39 S), so
    S = (G / tau - 2) / 2^39 with three roundings, amplified by 1 + 2 / (2^39 S) -- S_j >= 1e-9 is asserted, so by less than 1.004.
    It is held to math.fsum of the row's e^2 within 1e-13 relative (at most 300 non-negative terms: any order is within 300 ulp / 2).
    tau_j within 1e-12 of G_ref / (rate + alpha S_ref / 2), precision_out bit for bit tau_out of the cell's row, sum tau_j S_j
    within 1e-12, reruns and the call without wsse_out bit for bit."""
    rng = np.random.default_rng(4000 + 100 * D + 10 * n_modes + 2 * mode + sort)
    base = [37, 23, 11][:n_modes]
    other = list(base)
    other[mode] = 20 if _width(N_CELLS, base[mode]) == 8 else 40
    widths = set()
    sweep, worst_S, worst_t, worst_w = 10, 0.0, 0.0, 0.0
    for dims in (base, other):
        N = dims[mode]
        widths.add(_width(N_CELLS, N))
        ids = _planted_ids(rng, dims, mode)
        y = rng.standard_normal(N_CELLS)
        dr = B.DeviceRelation(ctx, B.IndexedDF((ids, y), dims))
        pairs = B.DevicePairs(ctx, ids, y)
        if sort:
            pairs.sort(n_modes - 1)
        S = [rng.standard_normal((d, D)) for d in dims]
        St = [ctx.tensor(s) for s in S]
        mean = 0.3
        e = y - pairs.predict(D, St, mean).cpu().numpy()
        rows0 = ids[:, mode] - 1
        n_j = np.bincount(rows0, minlength=N)
        S_ref = np.array([math.fsum((e[rows0 == j] ** 2).tolist()) for j in range(N)])
        assert np.all(S_ref[n_j > 0] >= 1e-9) and np.all(S_ref[n_j == 0] == 0.0)
        # S_j from two draws of one sweep
        ctx.set_sweep(sweep)
        t_lo, _, _ = _draw(ctx, dr, mode, pairs, D, St, mean, 1e-300, None, 2.0, 2.0, 1, N, N_CELLS)
        t_hi, _, _ = _draw(ctx, dr, mode, pairs, D, St, mean, 2.0 ** 40, None, 2.0, 2.0, 1, N, N_CELLS)
        S_dev = ((2.0 * t_lo) / t_hi - 2.0) / 2.0 ** 39
        assert np.all(S_dev[n_j == 0] == 0.0)
        err = np.abs(S_dev - S_ref)[n_j > 0] / S_ref[n_j > 0]
        worst_S = max(worst_S, err.max())
        assert err.max() <= 1e-13, (dims, int(np.argmax(err)), err.max())
        for shape in (0.5, 2.0):
            for rate, alpha in ((2.0, 1.7), (0.7, 40.0)):
                for through_dev in (False, True):
                    sweep += 1
                    tag = 1 + sweep % 3
                    a_arg, a_dev = (alpha, None) if not through_dev else (123.0, ctx.tensor([alpha]))      # the decoy loses
                    ctx.set_sweep(sweep)
                    tau, om, s = _draw(ctx, dr, mode, pairs, D, St, mean, a_arg, a_dev, shape, rate, tag, N, N_CELLS)
                    tau2, om2, s2 = _draw(ctx, dr, mode, pairs, D, St, mean, a_arg, a_dev, shape, rate, tag, N, N_CELLS)
                    tau3, om3, _ = _draw(ctx, dr, mode, pairs, D, St, mean, a_arg, a_dev, shape, rate, tag, N, N_CELLS, wsse=False)
                    G = ER.gamma_variates(SEED, sweep, tag, np.arange(N), shape + 0.5 * n_j)
                    ref = ER.draw_tau(G, S_ref, alpha, rate)
                    ref_s = math.fsum((ref * S_ref).tolist())
                    assert np.all(np.isfinite(tau)) and np.all(tau > 0)
                    et, ew = np.abs(tau / ref - 1.0).max(), abs(s / ref_s - 1.0)
                    worst_t, worst_w = max(worst_t, et), max(worst_w, ew)
                    assert et <= 1e-12, (dims, shape, rate, alpha, through_dev, int(np.argmax(np.abs(tau / ref - 1.0))), et)
                    assert np.array_equal(om, tau[rows0])                        # in the caller's order, sorted or not: the same bits
                    assert ew <= 1e-12, (dims, shape, rate, alpha, through_dev, s, ref_s)
                    assert s == s2 and np.array_equal(tau, tau2) and np.array_equal(om, om2)
                    assert np.array_equal(tau, tau3) and np.array_equal(om, om3)  # wsse_out is optional
        pairs.close()
        dr.close()
    assert widths == {8, 64}
    print(f"entity noise draw D={D} modes={n_modes} mode={mode} sort={sort}: max rel. error of S {worst_S:.3e}, of tau {worst_t:.3e}, "
          f"of sum tau S {worst_w:.3e} over 16 draws")


# ---- (b) the held-out density with a scale ------------------------------------------------------------------------------------
@pytest.mark.parametrize("sort", [False, True])
@pytest.mark.parametrize("n_modes,mode", [(2, 0), (2, 1), (3, 0), (3, 1), (3, 2)])
@pytest.mark.parametrize("D", [1, 7, 32, 64])
def test_lpd_update_with_a_precision_scale(B, ctx, D, n_modes, mode, sort):
    """The draw test's pairs; Gaussian and mixed-bounds records x alpha in {0.04, 5, 900} x alpha as a scalar and through alpha_dev,
    each through the phases 0, 1, 2, 2 on two factor sets, against lpd_restatement fed alpha tau of the cell's row (tau log-uniform
    on 0.05 .. 20), with the predictive mean the device forms -- test_gpu_lpd.py's method and tolerances: 1e-9 per pair, 1e-9 n on
    the two sums.  Before the scale is set and after it is cleared the update gives the same bits."""
    from bdf_amd._lib import check, lib
    rng = np.random.default_rng(6000 + 100 * D + 10 * n_modes + 2 * mode + sort)
    dims = [37, 23, 11][:n_modes]
    n = N_CELLS
    ids = _planted_ids(rng, dims, mode)
    y = rng.standard_normal(n)
    pairs = B.DevicePairs(ctx, ids, y)
    if sort:
        pairs.sort(n_modes - 1)
    mean = 0.3
    sets = []
    for _ in range(2):
        St = [ctx.tensor(rng.standard_normal((d, D))) for d in dims]
        sets.append((St, pairs.predict(D, St, mean).cpu().numpy()))
    tau = np.exp(rng.uniform(np.log(0.05), np.log(20.0), dims[mode]))
    tau[0], tau[1] = 0.05, 20.0
    tau_t = ctx.tensor(tau)
    scale = tau[ids[:, mode] - 1]
    stats, out = ctx.zeros(4), ctx.tensor(np.full(n, np.nan))

    def plain():
        check(lib().bdf_pairs_lpd_update(ctx.handle, pairs.handle, None, D, _facs(sets[0][0]), mean, 5.0, None, 1, _p(stats)))
        check(lib().bdf_pairs_lpd(ctx.handle, pairs.handle, _p(out)))
        ctx.sync()
        return out.cpu().numpy(), stats.cpu().numpy()

    before = plain()
    assert abs(before[1][0] - math.fsum(LR.cell_loglik(y, sets[0][1], 5.0))) <= 1e-9 * n
    pairs.set_precision_scale(tau_t, mode)
    worst_l = worst_s = 0.0
    for kind in ("gauss", "mixed"):
        for alpha in (0.04, 5.0, 900.0):
            bd = _bounds(rng, y, kind, math.sqrt(alpha)) if kind == "mixed" else None
            bdev = ctx.tensor(bd) if bd is not None else None
            for through_dev in (False, True):
                a_arg, a_dev = (alpha, None) if not through_dev else (123.0, ctx.tensor([alpha]))
                st = LR.Stream()
                for phase, (St, m) in zip((0, 1, 2, 2), (sets[0], sets[0], sets[1], sets[0])):
                    check(lib().bdf_pairs_lpd_update(ctx.handle, pairs.handle, _p(bdev), D, _facs(St), mean, a_arg, _p(a_dev), phase, _p(stats)))
                    if phase:
                        check(lib().bdf_pairs_lpd(ctx.handle, pairs.handle, _p(out)))
                    ctx.sync()
                    s = stats.cpu().numpy()
                    l_ref = LR.cell_loglik(y, m, alpha * scale, bd)
                    lpd_ref = st.update(l_ref, phase)
                    assert np.all(np.isfinite(l_ref)) and np.all(np.isfinite(s)) and s[2] == 0.0 and s[3] == 0.0
                    es = max(abs(s[0] - math.fsum(l_ref)), abs(s[1] - math.fsum(lpd_ref)))
                    worst_s = max(worst_s, es)
                    assert es <= 1e-9 * n, (kind, alpha, through_dev, phase, s, math.fsum(l_ref), math.fsum(lpd_ref))
                    if phase == 0:
                        assert s[0] == s[1]
                        continue
                    lpd = out.cpu().numpy()
                    el = np.abs(lpd - lpd_ref).max()
                    worst_l = max(worst_l, el)
                    assert el <= 1e-9, (kind, alpha, through_dev, phase, el, int(np.argmax(np.abs(lpd - lpd_ref))))
        # the scale matters: unscaled records are somewhere else
        assert np.abs(LR.cell_loglik(y, sets[0][1], 5.0 * scale) - LR.cell_loglik(y, sets[0][1], 5.0)).max() > 0.1
    # WAIC refuses pairs with a scale; the probit link takes none
    with pytest.raises(B.ArgumentError, match="bdf_pairs_waic_update"):
        check(lib().bdf_pairs_waic_update(ctx.handle, pairs.handle, None, D, _facs(sets[0][0]), mean, 5.0, None, 0, _p(stats)))
    with pytest.raises(B.ArgumentError, match="bdf_pairs_set_precision_scale"):
        check(lib().bdf_pairs_set_precision_scale(pairs.handle, _p(tau_t), n_modes))
    with pytest.raises(B.ArgumentError, match="bdf_pairs_set_precision_scale"):
        check(lib().bdf_pairs_set_precision_scale(pairs.handle, _p(tau_t), -1))
    pairs.set_precision_scale(None)
    after = plain()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    check(lib().bdf_pairs_waic_update(ctx.handle, pairs.handle, None, D, _facs(sets[0][0]), mean, 5.0, None, 0, _p(stats)))
    ctx.sync()
    print(f"scaled lpd update D={D} modes={n_modes} mode={mode} sort={sort}: max |lpd_dev - lpd_ref| = {worst_l:.3e}, "
          f"max |stat_dev - stat_ref| / n = {worst_s / n:.3e} over 48 launches")
    pairs.close()


def test_probit_pairs_take_no_scale(B, ctx):
    from bdf_amd._lib import check, lib
    pairs = B.DevicePairs(ctx, np.array([[1, 1], [2, 1]]), np.array([0.0, 1.0]))
    tau = ctx.tensor(np.ones(2))
    pairs.set_link(1)
    with pytest.raises(B.ArgumentError, match="probit"):
        pairs.set_precision_scale(tau, 0)
    pairs.set_link(0)
    pairs.set_precision_scale(tau, 0)
    pairs.set_link(1)
    St = [ctx.tensor(np.ones((2, 3))), ctx.tensor(np.ones((1, 3)))]
    with pytest.raises(B.ArgumentError, match="probit"):
        check(lib().bdf_pairs_lpd_update(ctx.handle, pairs.handle, None, 3, _facs(St), 0.0, 1.0, None, 0, _p(ctx.zeros(4))))
    pairs.close()


# ---- (c) whole iterations -------------------------------------------------------------------------------------------------------
CASES = [(n_modes, with_feat, alpha_sample) for n_modes in (2, 3) for with_feat in (0, 1) for alpha_sample in (0, 1)]
SHAPE, RATE = 1.5, 2.5

CHILD = textwrap.dedent('''
    import sys
    import numpy as np
    sys.path.insert(0, %r); sys.path.insert(0, %r)
    import bdf_amd as B
    import entity_noise_restatement as ER
    out, d = sys.argv[1], {}
    for n_modes, with_feat, alpha_sample in [(m, f, a) for m in (2, 3) for f in (0, 1) for a in (0, 1)]:
        ids, y, dims, D, feats, n_test, alpha, _, mode = ER.iteration_case(n_modes, with_feat, alpha_sample)
        names = ["a", "b", "c"][:n_modes]
        ents = [B.Entity(nm, F=feats[k]) for k, nm in enumerate(names)]
        table = {nm: ids[:, k] for k, nm in enumerate(names)}
        table["y"] = y
        rel = B.Relation(table, "noise", ents, alpha=alpha, dims=list(dims))
        rel.model.alpha_sample = bool(alpha_sample)
        B.assignToTest(rel, np.arange(1, n_test + 1))
        B.setEntityNoise(rel, [ents[mode], names[mode], mode + 1][(n_modes + with_feat + alpha_sample) %% 3], %r, %r)      # by object, name or mode
        rd = B.RelationData(rel)
        res = B.macau(rd, num_latent=D, burnin=1, psamples=2, verbose=False, seed=91, lpd=True)
        key = "%%d%%d%%d_" %% (n_modes, with_feat, alpha_sample)
        d[key + "native"], d[key + "pred"] = np.array(int(rd._engine.native)), res["predictions"]["pred"].to_numpy()
        d[key + "lpd"], d[key + "LPD"] = res["predictions"]["lpd"].to_numpy(), np.array(res["LPD"])
        d[key + "mean"], d[key + "alpha"] = np.array(rel.model.mean_value), np.array(rel.model.alpha)
        d[key + "k1"] = np.array([rd._engine.rows_dispatch(j)["k1"] for j in range(n_modes)])
        assert res["noise"]["entity"] == names[mode] and res["noise"]["shape"] == %r and res["noise"]["rate"] == %r and "robust" not in res
        d[key + "tau"] = res["noise"]["precision"]
        for k, en in enumerate(rd.entities):
            d[key + "S%%d" %% k], d[key + "mu%%d" %% k], d[key + "Lam%%d" %% k] = en.model.sample.T, en.model.mu, en.model.Lambda
            if feats[k] is not None:
                d[key + "beta%%d" %% k], d[key + "lb%%d" %% k] = en.model.beta, np.array(en.lambda_beta)
        rd._engine.close()
    np.savez(out, **d)
''') % (ROOT, os.path.join(ROOT, "tests"), SHAPE, RATE, SHAPE, RATE)


@pytest.fixture(scope="module")
def chains():
    """three iterations of every case of CASES on the native and on the step-by-step path: one child process per path"""
    return child(CHILD, no_native=False), child(CHILD, no_native=True)


@pytest.mark.parametrize("n_modes,with_feat,alpha_sample", CASES)
def test_whole_iterations_match_the_restated_chain_on_both_paths(chains, n_modes, with_feat, alpha_sample):
    """macau(lpd=True), burnin 1 + 2 draws: the tolerances are test_gpu_robust.py's for its whole iterations (1e-6 relative and
    absolute; beta 1e-5 / 1e-6; alpha and the posterior mean weights 1e-6 relative) and test_gpu_lpd.py's for lpd (1e-6)"""
    ids, y, dims, D, feats, n_test, alpha, _, mode = ER.iteration_case(n_modes, with_feat, alpha_sample)
    key = "%d%d%d_" % (n_modes, with_feat, alpha_sample)
    nat, step = ({k[len(key):]: v for k, v in ch.items() if k.startswith(key)} for ch in chains)
    assert nat["native"] == 1 and step["native"] == 0
    assert sorted(nat) == sorted(step) and len(nat) >= 8 + 3 * n_modes
    for k in nat:
        if k != "native":
            assert np.array_equal(nat[k], step[k]), k       # the two paths enqueue the same launches: the same bits
    assert np.array_equal(nat["k1"], dims)                  # every row of every entity by the wave-per-row kernel
    ref = ER.run_chain(ids[n_test:], y[n_test:], dims, D, 91, 3, mode=mode, shape=SHAPE, rate=RATE, alpha=alpha, alpha_sample=alpha_sample,
                       feats=feats, test_ids=ids[:n_test], test_values=y[:n_test], burnin=1)
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
    assert len(nat["tau"]) == dims[mode] and np.all(nat["tau"] > 0)
    np.testing.assert_allclose(nat["tau"], ref["tau_mean"], rtol=1e-6)
    assert np.all(np.isfinite(nat["lpd"])) and len(nat["lpd"]) == n_test
    np.testing.assert_allclose(nat["lpd"], ref["lpd"], **tol)
    np.testing.assert_allclose(nat["LPD"], ref["LPD"], **tol)
    # and the model matters: the Gaussian chain on the same data is somewhere else, in its rows and in its score
    gauss = ER.run_chain(ids[n_test:], y[n_test:], dims, D, 91, 3, alpha=alpha, alpha_sample=alpha_sample, feats=feats,
                         test_ids=ids[:n_test], test_values=y[:n_test], burnin=1)
    assert np.abs(gauss["S"][0] - ref["S"][0]).max() > 1e-3 and abs(gauss["LPD"] - ref["LPD"]) > 1e-3


def test_verbose_line_and_a_second_relation(B, capsys):
    """the verbose line gains the mean tau; a noise model on the SECOND relation is sampled (its rows move away from the Gaussian
    chain's) while the report covers the first: no result["noise"]"""
    import re
    ids, y, dims, D, feats, n_test, alpha, _, mode = ER.iteration_case(2, 0, 0)

    def run(noise_on):
        a, b, c = B.Entity("a"), B.Entity("b"), B.Entity("c")
        r1 = B.Relation({"a": ids[:, 0], "b": ids[:, 1], "y": y}, "one", [a, b], alpha=alpha, dims=list(dims))
        r2 = B.Relation({"a": ids[:, 0], "c": (ids[:, 1] - 1) % 12 + 1, "y": y[::-1].copy()}, "two", [a, c], alpha=alpha, dims=[dims[0], 12])
        B.assignToTest(r1, np.arange(1, n_test + 1))
        if noise_on == 1:
            B.setEntityNoise(r1, b)
        if noise_on == 2:
            B.setEntityNoise(r2, "c")
        rd = B.RelationData(r1)
        B.addRelation(rd, r2)
        res = B.macau(rd, num_latent=D, burnin=1, psamples=1, verbose=True, seed=5)
        S = rd.entities[0].model.sample.copy()
        tau2 = r2._dev.tau.cpu().numpy().copy() if r2._dev.tau is not None else None
        rd._engine.close()
        return res, S, tau2

    res0, S0, _ = run(0)
    assert " τ̄=" not in capsys.readouterr().out and "noise" not in res0
    res1, S1, _ = run(1)
    lines = [t for t in capsys.readouterr().out.splitlines() if "RMSE=" in t]
    assert len(lines) == 2 and all(re.search(r" τ̄=\d+\.\d{3} \| ", t) for t in lines), lines
    assert res1["noise"]["entity"] == "b" and len(res1["noise"]["precision"]) == dims[1]
    res2, S2, tau2 = run(2)
    assert " τ̄=" not in capsys.readouterr().out and "noise" not in res2
    assert tau2 is not None and np.all(tau2 > 0) and tau2.std() > 0
    assert np.abs(S2 - S0).max() > 1e-3 and np.abs(S1 - S0).max() > 1e-3


# ---- (d) nothing else moved -------------------------------------------------------------------------------------------------
def test_gaussian_chain_is_untouched_by_a_noise_engine_in_the_process(B):
    ids, y, sd, n_test, alpha = ER.planted(seed=5, N1=120, N2=90, n_train=3500, n_test=500)

    def gaussian():
        rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y + 0.25 * ids[:, 0] % 3}, "g", [B.Entity("u"), B.Entity("v")], dims=[120, 90])
        B.assignToTest(rel, np.arange(4000 - n_test + 1, 4001))
        rd = B.RelationData(rel)
        res = B.macau(rd, num_latent=16, burnin=2, psamples=2, verbose=False, seed=17, lpd=True)
        assert "noise" not in res and rel._dev.tau is None and rel._dev.omega is None
        out = [en.model.sample.copy() for en in rd.entities] + [res["predictions"]["pred"].to_numpy().copy(), res["predictions"]["lpd"].to_numpy().copy()]
        rd._engine.close()
        return out

    alone = gaussian()
    rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "p", [B.Entity("u"), B.Entity("v")], dims=[120, 90])
    B.assignToTest(rel, np.arange(4000 - n_test + 1, 4001))
    B.setEntityNoise(rel, "v")
    rdn = B.RelationData(rel)
    res = B.macau(rdn, num_latent=16, burnin=1, psamples=1, verbose=False, seed=17, lpd=True)
    assert len(res["noise"]["precision"]) == 90 and np.all(res["noise"]["precision"] > 0)
    beside = gaussian()                                     # the noise engine is alive: its relation carries tau
    assert rdn._engine.gibbs is not None or not rdn._engine.native
    for a, b in zip(alone, beside):
        assert np.array_equal(a, b)
    rdn._engine.close()


# ---- (e) errors through the C ABI ---------------------------------------------------------------------------------------------
def test_entity_noise_c_abi_errors(B, ctx):
    import torch
    from bdf_amd._lib import GibbsRelation, check, lib
    ids, y, sd, n_test, _ = ER.planted(seed=9, N1=60, N2=50, n_train=1500, n_test=0)
    rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "e", [B.Entity("u"), B.Entity("v")], dims=[60, 50])
    eng = B.GibbsEngine(B.RelationData(rel), 8, seed=3)
    assert eng.native
    n = len(y)
    train = B.DevicePairs(eng.ctx, ids, y)
    op = B.FeatOperator(eng.ctx, np.ones((n, 2)))
    lin, beta, alpha = eng.ctx.tensor(np.full(n, rel.model.mean_value)), eng.ctx.zeros(2), eng.ctx.tensor([1.0])
    om, tau = eng.ctx.tensor(np.ones(n)), eng.ctx.tensor(np.ones(50))
    flags = eng.ctx.tensor(np.zeros(n, dtype=np.int8), dtype=torch.int8)
    bounds = eng.ctx.tensor(np.stack([y, y], axis=1))
    sums = eng.ctx.zeros(2, 8 + 64)

    def record(**kw):
        arr = (GibbsRelation * 1)()
        g = arr[0]
        g.rel, g.mean_value, g.alpha_dev, g.rel_tag, g.nnz = eng.rel[0].handle, rel.model.mean_value, alpha.data_ptr(), 1, n
        g.entity_of_mode[0], g.entity_of_mode[1] = 0, 1
        g.train, g.first_obs, g.obs_block, g.obs_precision = train.handle, 0, n, om.data_ptr()
        g.noise_mode, g.noise_shape, g.noise_rate, g.noise_tau = 2, 2.0, 2.0, tau.data_ptr()
        for k, v in kw.items():
            setattr(g, k, v)
        return arr

    def register(arr):
        check(lib().bdf_gibbs_set_relations(eng.gibbs, 1, C.cast(arr, C.c_void_p)))

    for bad in (dict(probit=1, linear=lin.data_ptr()), dict(censor=flags.data_ptr(), linear=lin.data_ptr()),
                dict(interval=bounds.data_ptr(), linear=lin.data_ptr()), dict(feat=op.handle, beta=beta.data_ptr(), linear=lin.data_ptr()),
                dict(robust_nu=4.0), dict(pg_model=1, linear=lin.data_ptr()), dict(bg_weight=0.1, bg_sums=sums.data_ptr())):
        with pytest.raises(B.ArgumentError, match="noise_mode"):
            register(record(**bad))
    for bad in (dict(noise_mode=3), dict(noise_mode=-1), dict(noise_shape=0.0), dict(noise_shape=float("nan")), dict(noise_rate=-1.0),
                dict(noise_rate=float("inf")), dict(noise_tau=None), dict(obs_precision=None), dict(train=None)):
        with pytest.raises(B.ArgumentError, match="noise"):
            register(record(**bad))
    facs = _facs(eng.factors_of(rel))
    small = B.DevicePairs(eng.ctx, ids[:-1], y[:-1])
    three = B.DevicePairs(eng.ctx, np.concatenate([ids, ids[:, :1]], axis=1), y)

    def draw(rel_h=eng.rel[0].handle, mode=1, train_h=train.handle, D=8, fp=facs, a=1.0, a_dev=None, shape=2.0, rate=2.0, t=tau, out=om):
        check(lib().bdf_entity_noise_draw(eng.ctx.handle, rel_h, mode, train_h, D, fp, 0.0, a, _p(a_dev), shape, rate, 1, _p(t), _p(out), None))

    for bad in (dict(rel_h=None), dict(train_h=None), dict(fp=None), dict(t=None), dict(out=None), dict(mode=-1), dict(mode=2), dict(D=0), dict(D=65),
                dict(a=0.0), dict(a=-1.0), dict(a=float("nan")), dict(a=float("inf")), dict(shape=0.0), dict(shape=-2.0), dict(shape=float("nan")),
                dict(shape=float("inf")), dict(rate=0.0), dict(rate=float("nan")), dict(rate=float("inf")), dict(train_h=small.handle),
                dict(train_h=three.handle)):
        with pytest.raises(B.ArgumentError, match="bdf_entity_noise_draw"):
            draw(**bad)
    draw(a=0.0, a_dev=alpha)                                 # alpha_dev wins over the scalar
    register(record(alpha_sample=1, alpha_lambda0=1.0, alpha_nu0=2.0))      # and the well-formed record is accepted: one iteration runs
    eng.sweep(1)
    eng.sync()
    assert np.all(np.isfinite(rel.entities[0].model.sample))
    t, w = tau.cpu().numpy(), om.cpu().numpy()
    assert np.all(np.isfinite(t)) and np.all(t > 0) and t.std() > 0 and float(alpha.item()) != 1.0
    assert np.array_equal(w, t[ids[:, 1] - 1])
    small.close(); three.close()
    op.close()
    train.close()
    eng.close()


# ---- (f) planted column noise ---------------------------------------------------------------------------------------------------
# r = RMSE(noise) / RMSE(Gaussian) against the clean held-out values and c = corr(log posterior-mean tau, log planted precision) of
# the restated chain on the CPU (ER.run_chain, planted seeds 0, 1, 2, chain seed 1)
R_CPU = (0.5702, 0.5338, 0.4524)
C_CPU = (0.9453, 0.9482, 0.9496)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_planted_column_noise(B, seed):
    """150 x 100, rank 3, 4,500 training cells whose column has noise sd log-uniform in [0.1, 3], 1,500 held-out cells scored against
    their clean values; D = 4, 30 + 50 iterations, alpha = 1 / mean(sd^2) fixed, prior Gamma(2, 2), the same chain seed for both
    models.  The restated chain gave r = 0.570, 0.534, 0.452 (all below 0.8) and c = 0.945, 0.948, 0.950.  The device must keep
    half the margin: r <= (1 + max r_cpu) / 2 = 0.7851 and c >= 1 - 2 (1 - min c_cpu) = 0.8906."""
    ids, y, sd, n_test, alpha = ER.planted(seed)
    n = len(y)

    def run(noise):
        rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "planted", [B.Entity("u"), B.Entity("v")], alpha=alpha, dims=[150, 100])
        B.assignToTest(rel, np.arange(n - n_test + 1, n + 1))
        if noise:
            B.setEntityNoise(rel, "v", 2.0, 2.0)
        rd = B.RelationData(rel)
        res = B.macau(rd, num_latent=4, burnin=30, psamples=50, verbose=False, seed=1)
        pred = res["predictions"]["pred"].to_numpy()
        rd._engine.close()
        return pred, res.get("noise")

    pred_n, noise = run(True)
    pred_g, none = run(False)
    assert none is None and noise["entity"] == "v" and len(noise["precision"]) == 100
    r, c = ER.quality(pred_n, pred_g, y[-n_test:], noise["precision"], sd)
    print(f"planted column noise, seed {seed}: r = {r:.4f} (restated chain {R_CPU[seed]:.4f}), c = {c:.4f} (restated chain {C_CPU[seed]:.4f})")
    assert max(R_CPU) < 0.8
    assert r <= (1.0 + max(R_CPU)) / 2.0, (r, R_CPU)
    assert c >= 1.0 - 2.0 * (1.0 - min(C_CPU)), (c, C_CPU)
