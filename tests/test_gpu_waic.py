"""WAIC on the training cells on the GPU: bdf_pairs_waic_update / bdf_pairs_waic against the numpy restatement
(tests/waic_restatement.py), whole macau() chains of a setWaic relation of every noise model against the restated chain on both
iteration paths, the chain untouched by the switch, the refusals of the C ABI, and the score's verdict on planted data."""
import ctypes as C
import math
import os
import re
import textwrap

import numpy as np
import pytest

from both_paths import child
import censored_restatement as CR
import interval_restatement as IR
import lpd_restatement as LR
import ordinal_restatement as OR
import probit_restatement as PR
import waic_restatement as WR
from test_gpu_lpd import _bounds, _facs, _p

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9                         # per pair, times max(1, |restated value|): the values carry lpd's rounding; V grows like l^2


def _tol(ref):
    return TOL * np.maximum(1.0, np.abs(ref))


def _final_tolerances(lppd_ref, V_ref):
    """what the per-pair tolerance allows the four end-of-run sums: the sum of the pairs' tolerances for sum lppd and sum V; for
    the squares about the mean, every elpd_t may be off by e_t = tol(lppd_t) + tol(V_t) and their mean by the mean of e_t, so term
    t by 2 |elpd_t - mean| d_t + d_t^2 with d_t = e_t + mean e"""
    e = _tol(lppd_ref) + _tol(V_ref)
    d = e + e.mean()
    el = lppd_ref - V_ref
    return _tol(lppd_ref).sum(), _tol(V_ref).sum(), float((2.0 * np.abs(el - el.mean()) * d + d * d).sum())


# ---- (a) the update ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sort", [False, True])
@pytest.mark.parametrize("n_modes", [2, 3])
@pytest.mark.parametrize("D", [1, 7, 10, 32, 64])
def test_waic_update_matches_the_restatement(B, ctx, D, n_modes, sort):
    """Every kind of record x alpha in {0.04, 5, 900} x alpha as a scalar and through alpha_dev (with a decoy scalar), each through
    the phases 0, 1, 2, 2 on the factor sets A, A, B, A, where B is scaled to max |udot| = 40 -- the cases, the shapes and the
    bounds of test_gpu_lpd.py's update test, for its reasons; the restated maps take the predictive mean m that the device forms
    (bdf_predict), as there.  After every launch the four statistics, and after every phase >= 1 the state as bdf_pairs_waic shows
    it -- every pair's (lppd, V) in the caller's order -- and its four end-of-run sums, against the restated stream.

    Tolerance: 1e-9 max(1, |restated value|) per pair and the sum of the pairs' tolerances for a sum (for the squares about the mean:
    what the pairs' tolerances allow them, _final_tolerances); the count of V > 0.4 is equal as an integer.  Phase 0 leaves the
    state bit for bit.  The worst case of every parameter set is printed (-s); DESIGN.md section 17 records it."""
    from bdf_amd._lib import check, lib
    rng = np.random.default_rng(7000 + 100 * D + 10 * n_modes + sort)
    dims = [37, 23, 11][:n_modes]
    n = 1003                                               # not a multiple of 8 or of 256: the last group and the last block are partly idle
    ids = np.stack([rng.integers(1, d + 1, n) for d in dims], axis=1)
    ids[1::7] = ids[0]                                     # the same cell many times over
    y = rng.standard_normal(n)
    pairs = B.DevicePairs(ctx, ids, y)
    if sort:
        pairs.sort(n_modes - 1)
    mean = 0.3
    sets = []
    for reach in (None, 40.0):
        S = [rng.standard_normal((d, D)) for d in dims]
        if reach is not None:                              # rescale the first factor so that max |udot| is `reach`
            S[0] *= reach / np.abs(IR.udot(ids, S)).max()
        St = [ctx.tensor(s) for s in S]
        m_np = IR.udot(ids, S) + mean
        m = pairs.predict(D, St, mean).cpu().numpy()
        scale = np.abs(np.prod([s[ids[:, k] - 1] for k, s in enumerate(S)], axis=0)).sum(axis=1) + abs(mean)
        assert np.all(np.abs(m - m_np) <= 4e-16 * (D + 2) * scale)      # the gather: each of the D + 1 additions rounds once
        sets.append((St, m))
    (St_a, m_a), (St_b, m_b) = sets
    assert np.abs(m_b).max() > 39.0
    stats, fstats, out = ctx.zeros(4), ctx.zeros(4), ctx.tensor(np.full((n, 2), np.nan))
    with pytest.raises(B.ArgumentError, match="bdf_pairs_waic"):          # no posterior draw yet
        check(lib().bdf_pairs_waic(ctx.handle, pairs.handle, _p(out), _p(fstats)))

    def read():
        check(lib().bdf_pairs_waic(ctx.handle, pairs.handle, _p(out), _p(fstats)))
        ctx.sync()
        return out.cpu().numpy().copy(), fstats.cpu().numpy().copy()

    worst_l = worst_v = worst_s = 0.0
    have_state, high = False, 0
    for kind in ("gauss", "probit", "all", "mixed"):
        pairs.set_link(1 if kind == "probit" else 0)
        for alpha in (0.04, 5.0, 900.0):
            ra = math.sqrt(alpha)
            bd = _bounds(rng, y, kind, ra) if kind in ("all", "mixed") else None
            bdev = ctx.tensor(bd) if bd is not None else None
            for through_dev in (False, True):
                # through alpha_dev the scalar argument is a decoy: the device value wins
                a_arg, a_dev = (alpha, None) if not through_dev else (123.0, ctx.tensor([alpha]))
                st = WR.Stream()
                for phase, (St, m) in zip((0, 1, 2, 2), ((St_a, m_a), (St_a, m_a), (St_b, m_b), (St_a, m_a))):
                    before = read() if (phase == 0 and have_state) else None          # (state from the previous combination)
                    check(lib().bdf_pairs_waic_update(ctx.handle, pairs.handle, _p(bdev), D, _facs(St), mean, a_arg, _p(a_dev), phase, _p(stats)))
                    ctx.sync()
                    s = stats.cpu().numpy()
                    l_ref = LR.cell_loglik(y, m, alpha, bd, probit=kind == "probit")
                    lppd_ref, V_ref = st.update(l_ref, phase)
                    assert np.all(np.isfinite(l_ref)) and np.all(np.isfinite(s))
                    t_l, t_v, t_ss = _final_tolerances(lppd_ref, V_ref)
                    es = max(abs(s[0] - math.fsum(l_ref)) / _tol(l_ref).sum(), abs(s[1] - math.fsum(lppd_ref)) / t_l, abs(s[2] - math.fsum(V_ref)) / t_v)
                    worst_s = max(worst_s, es)
                    assert es <= 1.0, (kind, alpha, through_dev, phase, s, math.fsum(l_ref), math.fsum(lppd_ref), math.fsum(V_ref))
                    assert s[3] == float(np.count_nonzero(V_ref > 0.4)), (kind, alpha, through_dev, phase, s[3])
                    if phase == 0:
                        assert s[0] == s[1] and s[2] == 0.0 and s[3] == 0.0      # burn-in: lppd is this draw's l, no variance yet
                        if before is not None:
                            after = read()
                            assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])      # the state is untouched
                        continue
                    have_state = True
                    got, f = read()                                               # in the caller's order, sorted or not
                    assert np.all(np.isfinite(got)) and np.all(np.isfinite(f))
                    el = (np.abs(got[:, 0] - lppd_ref) / _tol(lppd_ref)).max() * TOL
                    ev = (np.abs(got[:, 1] - V_ref) / _tol(V_ref)).max() * TOL
                    worst_l, worst_v = max(worst_l, el), max(worst_v, ev)
                    assert el <= TOL and ev <= TOL, (kind, alpha, through_dev, phase, el, ev)
                    if phase == 1:
                        assert not got[:, 1].any()                               # one draw: V is exactly 0
                    ref = WR.summary(lppd_ref, V_ref)
                    ef = max(abs(f[0] - ref["lppd"]) / t_l, abs(f[1] - ref["p_waic"]) / t_v, abs(f[2] - ref["ss"]) / t_ss)
                    worst_s = max(worst_s, ef)
                    assert ef <= 1.0 and f[3] == ref["n_high"], (kind, alpha, through_dev, phase, f, ref)
                    high += ref["n_high"]
    print(f"waic update D={D} modes={n_modes} sort={sort}: worst relative error of lppd {worst_l:.3e}, of V {worst_v:.3e}; worst error of "
          f"a sum over its tolerance {worst_s:.3e}, over 96 updates")
    assert high > 0
    pairs.close()


def test_waic_methods_return_the_callers_order_and_rerun_bit_for_bit(B, ctx):
    """DevicePairs.waic_update / waic on sorted and unsorted pairs of the same cells: the same per-pair values at the same indices;
    the statistics of a rerun are the same bits; the lpd state beside it is left alone"""
    rng = np.random.default_rng(12)
    n, D = 2500, 12
    ids = np.stack([rng.integers(1, 38, n), rng.integers(1, 24, n)], axis=1)
    y = rng.standard_normal(n)
    S = [ctx.tensor(rng.standard_normal((37, D)) * 0.4), ctx.tensor(rng.standard_normal((23, D)) * 0.4)]
    S2 = [ctx.tensor(rng.standard_normal((37, D)) * 0.4), S[1]]
    bd_h = IR.bin_bounds(y, IR.BIN_EDGES)
    bd = ctx.tensor(bd_h)
    got = []
    for sort in (False, True, True):
        pairs = B.DevicePairs(ctx, ids, y)
        if sort:
            pairs.sort(1)
        pairs.lpd_update(D, S2, 0.1, 2.0, 1, bd)
        lpd0 = pairs.lpd()
        s1 = pairs.waic_update(D, S, 0.1, 2.0, 1, bd).cpu().numpy().copy()
        s2 = pairs.waic_update(D, S2, 0.1, ctx.tensor([2.0]), 2, bd).cpu().numpy().copy()
        f, pw = pairs.waic(pointwise=True)
        f2, none = pairs.waic()
        assert none is None and np.array_equal(f, f2) and np.array_equal(pairs.lpd(), lpd0)
        got.append((pw, s1, s2, f))
        pairs.close()
    assert np.array_equal(got[0][0], got[1][0]) and got[0][0].shape == (n, 2)
    for a, b in zip(got[1], got[2]):
        assert np.array_equal(a, b)
    m1, m2 = (IR.udot(ids, [s.cpu().numpy() for s in F]) + 0.1 for F in (S, S2))
    st = WR.Stream()
    st.update(LR.cell_loglik(y, m1, 2.0, bd_h), 1)
    lppd, V = st.update(LR.cell_loglik(y, m2, 2.0, bd_h), 2)
    assert np.all(np.abs(got[0][0][:, 0] - lppd) <= _tol(lppd)) and np.all(np.abs(got[0][0][:, 1] - V) <= _tol(V))
    ref = WR.summary(lppd, V)
    t_l, t_v, t_ss = _final_tolerances(lppd, V)
    f = got[0][3]
    assert abs(f[0] - ref["lppd"]) <= t_l and abs(f[1] - ref["p_waic"]) <= t_v and abs(f[2] - ref["ss"]) <= t_ss and f[3] == ref["n_high"]


# ---- (b) whole chains --------------------------------------------------------------------------------------------------------
BINS = (-0.8, 0.0, 0.8)
KINDS = ("gauss", "probit", "censored", "binned", "ordinal")
BURNIN, PSAMPLES, SEED = 2, 3, 91


def _chain_case(kind):
    """the whole-chain cases, the small relations of the noise models' own whole-iteration tests: a Gaussian relation that samples
    its precision, a censored and an ordinal one with sampled edges (two modes; their leading cells held out), a probit (two
    modes) and a binned relation (three modes) without test cells.  Returns a dict: ids, y, dims, D, n_test (0: no test cells),
    alpha, alpha_sample and the kind's own: censor / K"""
    if kind == "probit":
        ids, y, dims, D, _, _ = PR.iteration_case(2, False)
        return dict(ids=ids, y=y, dims=dims, D=D, n_test=0, alpha=1.0, alpha_sample=False)
    if kind == "censored":
        ids, y, c, dims, D, _, n_test, alpha, _ = CR.iteration_case(2, False, False)
        return dict(ids=ids, y=y, dims=dims, D=D, n_test=n_test, alpha=alpha, alpha_sample=False, censor=c)
    if kind == "ordinal":
        ids, lev, dims, D, _, n_test, alpha, _ = OR.iteration_case(2, False, False)
        return dict(ids=ids, y=lev, dims=dims, D=D, n_test=n_test, alpha=alpha, alpha_sample=False, K=5)
    ids, y, _, dims, D, _, n_test, alpha, _ = IR.iteration_case(3 if kind == "binned" else 2, False, kind == "gauss")
    return dict(ids=ids, y=y, dims=dims, D=D, n_test=n_test if kind == "gauss" else 0, alpha=alpha, alpha_sample=kind == "gauss")


CHILD = textwrap.dedent('''
    import contextlib, io, sys
    import numpy as np
    sys.path.insert(0, %r); sys.path.insert(0, %r)
    import bdf_amd as B
    from test_gpu_waic import BINS, BURNIN, KINDS, PSAMPLES, SEED, _chain_case
    out, d = sys.argv[1], {}
    for kind in KINDS:
        c = _chain_case(kind)
        ids, y, dims = c["ids"], c["y"], c["dims"]
        names = ["a", "b", "c"][:len(dims)]
        table = {nm: ids[:, k] for k, nm in enumerate(names)}
        table["y"] = y
        rel = B.Relation(table, kind, [B.Entity(nm) for nm in names], alpha=c["alpha"], dims=list(dims))
        rel.model.alpha_sample = c["alpha_sample"]
        if c["n_test"]:
            B.assignToTest(rel, np.arange(1, c["n_test"] + 1))
        if kind == "probit":
            B.setProbit(rel)
        if kind == "censored":
            B.setCensored(rel, c["censor"][c["n_test"]:])
        if kind == "binned":
            B.setBinned(rel, BINS)
        if kind == "ordinal":
            B.setOrdinal(rel)
        B.setWaic(rel, pointwise=True)
        rd = B.RelationData(rel)
        text = io.StringIO()
        with contextlib.redirect_stdout(text):
            res = B.macau(rd, num_latent=c["D"], burnin=BURNIN, psamples=PSAMPLES, verbose=True, seed=SEED)
        key = kind + "_"
        w = res["WAIC"]
        assert sorted(w) == ["elpd", "lppd", "n", "n_high", "p_waic", "pointwise", "se", "waic"]
        d[key + "native"] = np.array(int(rd._engine.native))
        d[key + "summary"] = np.array([w["waic"], w["elpd"], w["lppd"], w["p_waic"], w["se"], w["n_high"], w["n"]], dtype=np.float64)
        d[key + "columns"] = np.array(list(w["pointwise"].columns))
        d[key + "ids"] = w["pointwise"][names].to_numpy()
        d[key + "lppd"], d[key + "p_waic"] = w["pointwise"]["lppd"].to_numpy(), w["pointwise"]["p_waic"].to_numpy()
        d[key + "alpha"], d[key + "lines"] = np.array(rel.model.alpha), np.array([t for t in text.getvalue().splitlines() if "RMSE=" in t])
        if kind == "ordinal":
            d[key + "edges"] = res["ordinal"]["edges_trace"]
        for k, en in enumerate(rd.entities):
            d[key + "S%%d" %% k] = en.model.sample.T
        rd._engine.close()
    np.savez(out, **d)
''') % (ROOT, os.path.join(ROOT, "tests"))


@pytest.fixture(scope="module")
def chains():
    """2 + 3 iterations of macau() on the five setWaic relations, on the native and on the step-by-step path: one child process per path"""
    return child(CHILD, no_native=False), child(CHILD, no_native=True)


@pytest.mark.parametrize("kind", KINDS)
def test_waic_whole_chains_match_the_restatement_on_both_paths(chains, kind):
    """Both paths equal bit for bit; against the restated chain at section 13's tolerances (rtol = atol = 1e-6 for the factors and
    every per-cell value; a sum of n per-cell values: atol = n 1e-6), the verbose line's ELPD to its four printed decimals."""
    c = _chain_case(kind)
    ids, y, dims, n_test = c["ids"], c["y"], c["dims"], c["n_test"]
    key = kind + "_"
    nat, step = ({k[len(key):]: v for k, v in ch.items() if k.startswith(key)} for ch in chains)
    assert nat["native"] == 1 and step["native"] == 0
    assert sorted(nat) == sorted(step)
    for k in nat:
        if k not in ("native", "lines"):
            assert np.array_equal(nat[k], step[k]), k       # the two paths enqueue the same launches: the same bits
    tr = slice(n_test, None)
    interval = IR.bin_bounds(y, BINS) if kind == "binned" else None
    ref = WR.score_chain("interval" if kind == "binned" else kind, ids[tr], y[tr], dims, c["D"], SEED, BURNIN, PSAMPLES, alpha=c["alpha"],
                         alpha_sample=c["alpha_sample"], censor=c["censor"][tr] if kind == "censored" else None, interval=interval,
                         K=c.get("K"), test_ids=ids[:n_test] if n_test else None)
    tol = dict(rtol=1e-6, atol=1e-6)
    for k in range(len(dims)):
        np.testing.assert_allclose(nat["S%d" % k], ref["S"][k], err_msg="sample of entity %d" % k, **tol)
    if kind != "probit":
        np.testing.assert_allclose(nat["alpha"], ref["alpha"], rtol=1e-6)
        assert (nat["alpha"] != c["alpha"]) == c["alpha_sample"]
    if kind == "ordinal":
        np.testing.assert_allclose(nat["edges"], ref["edges_trace"][BURNIN:], **tol)
        assert np.any(ref["edges_trace"][-1] != np.arange(1, 5) + 0.5)            # the edges have moved: the bounds followed them
    n = len(y) - n_test
    w = ref["waic"]
    print(f"{kind}: elpd device {nat['summary'][1]:.6f} restatement {w['elpd']:.6f}; worst per-cell difference of lppd "
          f"{np.abs(nat['lppd'] - ref['lppd_t']).max():.2e}, of p_waic {np.abs(nat['p_waic'] - ref['V_t']).max():.2e}")
    assert list(nat["columns"]) == ["a", "b", "c"][:len(dims)] + ["lppd", "p_waic"] and np.array_equal(nat["ids"], ids[tr])
    assert np.all(np.isfinite(nat["lppd"])) and np.all(np.isfinite(nat["p_waic"])) and len(nat["lppd"]) == n
    np.testing.assert_allclose(nat["lppd"], ref["lppd_t"], **tol)
    np.testing.assert_allclose(nat["p_waic"], ref["V_t"], **tol)
    np.testing.assert_allclose(nat["summary"][:5], [w["waic"], w["elpd"], w["lppd"], w["p_waic"], w["se"]], rtol=1e-6, atol=2e-6 * n)
    assert nat["summary"][5] == w["n_high"] and nat["summary"][6] == n == w["n"]
    # the summary is the pointwise table's: sums, and the standard error from the squares about the mean
    mine = WR.summary(nat["lppd"], nat["p_waic"])
    np.testing.assert_allclose(nat["summary"][:5], [mine["waic"], mine["elpd"], mine["lppd"], mine["p_waic"], mine["se"]], rtol=1e-12, atol=1e-9)
    assert np.all(nat["p_waic"] >= 0.0)
    if kind in ("probit", "binned", "ordinal"):             # every record of these is a probability
        assert np.all(nat["lppd"] <= 0.0)
    # the verbose line: ELPD after RMSE (and LPD, which these runs do not ask for), before the ordinal relation's cut
    assert len(nat["lines"]) == BURNIN + PSAMPLES
    for line, want in zip(nat["lines"], ref["elpd_trace"]):
        mt = re.search(r" RMSE=\s*(?:\d+\.\d{4}|nan) ELPD=(-?\d+\.\d{4})( cut=\[[^\]]*\])? \| ", str(line))
        assert mt and abs(float(mt.group(1)) - want) <= 1e-4 and bool(mt.group(2)) == (kind == "ordinal"), (line, want)


def test_gaussian_chain_is_untouched_by_setwaic(B, capsys):
    """the same Gaussian chain (alpha sampled: the score shares the sampler's training pairs) with and without setWaic: the factors,
    the predictions, RMSE, LPD and every printed character but ELPD bit for bit; without it no result key and nothing printed"""
    ids, y, _, dims, D, _, n_test, alpha, _ = IR.iteration_case(2, False, True)

    def run(waic):
        rel = B.Relation({"a": ids[:, 0], "b": ids[:, 1], "y": y}, "g", [B.Entity("a"), B.Entity("b")], alpha=alpha, dims=list(dims))
        rel.model.alpha_sample = True
        B.assignToTest(rel, np.arange(1, n_test + 1))
        if waic:
            B.setWaic(rel)
        rd = B.RelationData(rel)
        capsys.readouterr()
        res = B.macau(rd, num_latent=D, burnin=1, psamples=2, verbose=True, seed=17, lpd=True)
        lines = [re.sub(r"\[[0-9.]+s\]", "", t) for t in capsys.readouterr().out.splitlines()]
        S = [en.model.sample.copy() for en in rd.entities]
        rd._engine.close()
        return res, S, lines, rel.model.alpha

    plain, S0, lines0, a0 = run(False)
    scored, S1, lines1, a1 = run(True)
    assert plain["RMSE"] == scored["RMSE"] and plain["ROC"] == scored["ROC"] and plain["LPD"] == scored["LPD"] and a0 == a1
    for col in ("pred", "lpd"):
        assert np.array_equal(plain["predictions"][col].to_numpy(), scored["predictions"][col].to_numpy())
    for a, b in zip(S0, S1):
        assert np.array_equal(a, b)
    assert "WAIC" not in plain and not any("ELPD" in t for t in lines0)
    assert sorted(set(scored) - set(plain)) == ["WAIC"]
    w = scored["WAIC"]
    assert sorted(w) == ["elpd", "lppd", "n", "n_high", "p_waic", "se", "waic"] and w["n"] == len(y) - n_test
    assert all(math.isfinite(w[k]) for k in w) and w["waic"] == -2.0 * w["elpd"] and w["p_waic"] > 0.0 and w["se"] > 0.0
    assert [re.sub(r" ELPD=-?\d+\.\d{4}", "", t) for t in lines1] == lines0 and sum("ELPD=" in t for t in lines1) == 3
    assert all(re.search(r" LPD=-?\d+\.\d{4} ELPD=-?\d+\.\d{4} \| ", t) for t in lines1 if "ELPD=" in t)


# ---- (c) refusals -------------------------------------------------------------------------------------------------------------
def test_waic_c_abi_errors(B, ctx):
    from bdf_amd._lib import check, lib
    rng = np.random.default_rng(5)
    n, D = 100, 8
    ids = np.stack([rng.integers(1, 11, n), rng.integers(1, 8, n)], axis=1)
    y = (rng.random(n) < 0.5).astype(np.float64)
    pairs = B.DevicePairs(ctx, ids, y)
    St = [ctx.tensor(rng.standard_normal((10, D))), ctx.tensor(rng.standard_normal((7, D)))]
    bdev = ctx.tensor(np.stack([y - 0.5, y + 0.5], axis=1))
    stats, out, a_dev = ctx.zeros(4), ctx.zeros((n, 2)), ctx.tensor([2.0])
    facs = _facs(St)
    holed = (C.c_void_p * 2)(St[0].data_ptr(), None)

    def update(c=ctx.handle, p=pairs.handle, bounds=None, D=D, fp=facs, a=1.0, a_dev=None, phase=1, st=stats):
        check(lib().bdf_pairs_waic_update(c, p, bounds, D, fp, 0.0, a, _p(a_dev), phase, _p(st)))

    for bad in (dict(c=None), dict(p=None), dict(fp=None), dict(st=None), dict(fp=holed), dict(D=0), dict(D=65), dict(phase=-1), dict(phase=3),
                dict(a=0.0), dict(a=-1.0), dict(a=float("nan")), dict(a=float("inf")), dict(bounds=C.c_void_p(bdev.data_ptr() + 8)),
                dict(phase=2)):                                  # (the last: phase 2 before any phase 1)
        with pytest.raises(B.ArgumentError, match="bdf_pairs_waic_update"):
            update(**bad)
    for bad in ((None, pairs.handle, _p(out), _p(stats)), (ctx.handle, None, _p(out), _p(stats)), (ctx.handle, pairs.handle, _p(out), None),
                (ctx.handle, pairs.handle, _p(out), _p(stats))):
        with pytest.raises(B.ArgumentError, match="bdf_pairs_waic"):
            check(lib().bdf_pairs_waic(*bad))                    # (the last: no posterior draw yet)
    update(phase=0)                                              # burn-in keeps nothing: still no draw
    with pytest.raises(B.ArgumentError, match="bdf_pairs_waic"):
        check(lib().bdf_pairs_waic(ctx.handle, pairs.handle, _p(out), _p(stats)))
    pairs.lpd_update(D, St, 0.0, 1.0, 1)                         # the lpd state's draws are not this state's
    with pytest.raises(B.ArgumentError, match="bdf_pairs_waic"):
        check(lib().bdf_pairs_waic(ctx.handle, pairs.handle, _p(out), _p(stats)))
    pairs.set_link(1)
    with pytest.raises(B.ArgumentError, match="probit"):
        update(bounds=_p(bdev))
    update()                                                     # the probit link without bounds is the 0/1 map
    pairs.set_link(0)
    update(bounds=_p(bdev), a=0.0, a_dev=a_dev, phase=2)         # alpha_dev wins over the scalar; phase 2 after a phase 1
    with pytest.raises(B.ArgumentError, match="bdf_pairs_waic"):
        check(lib().bdf_pairs_waic(ctx.handle, pairs.handle, C.c_void_p(out.data_ptr() + 8), _p(stats)))      # misaligned table
    check(lib().bdf_pairs_waic(ctx.handle, pairs.handle, None, _p(stats)))                                     # no table asked for
    ctx.sync()
    s0 = stats.cpu().numpy().copy()
    check(lib().bdf_pairs_waic(ctx.handle, pairs.handle, _p(out), _p(stats)))
    ctx.sync()
    assert np.array_equal(stats.cpu().numpy(), s0) and np.all(np.isfinite(out.cpu().numpy())) and np.all(np.isfinite(s0))
    pairs.close()
    empty = B.DevicePairs(ctx, np.zeros((0, 2), dtype=np.int64), np.zeros(0))        # no pairs: the statistics are zero
    stats.fill_(7.0)
    check(lib().bdf_pairs_waic_update(ctx.handle, empty.handle, None, D, facs, 0.0, 1.0, None, 1, _p(stats)))
    ctx.sync()
    assert np.array_equal(stats.cpu().numpy(), np.zeros(4))
    stats.fill_(7.0)
    check(lib().bdf_pairs_waic(ctx.handle, empty.handle, None, _p(stats)))
    ctx.sync()
    assert np.array_equal(stats.cpu().numpy(), np.zeros(4))
    empty.close()


def test_macau_refuses_waic_with_more_than_one_rank_on_a_real_engine(B):
    ids, y, _, dims, D, _, n_test, alpha, _ = IR.iteration_case(2, False, False)
    rel = B.Relation({"a": ids[:, 0], "b": ids[:, 1], "y": y}, "g", [B.Entity("a"), B.Entity("b")], alpha=alpha, dims=list(dims))
    B.setWaic(rel)
    rd = B.RelationData(rel)
    eng = B.GibbsEngine(rd, D, seed=3)
    eng.world = 2                      # what an engine built with shard=(rank, 2) says of itself (its set-up needs a second process)
    with pytest.raises(B.ArgumentError, match="more than one rank"):
        B.macau(rd, num_latent=D, burnin=1, psamples=2, verbose=False, engine=eng, reset_model=False)
    eng.world = 1
    with pytest.raises(B.ArgumentError, match="psamples"):
        B.macau(rd, num_latent=D, burnin=1, psamples=1, verbose=False, engine=eng, reset_model=False)
    res = B.macau(rd, num_latent=D, burnin=1, psamples=2, verbose=False, engine=eng, reset_model=False)      # without test cells
    assert math.isfinite(res["WAIC"]["waic"]) and res["WAIC"]["n"] == len(y) and "pointwise" not in res["WAIC"]
    B.setWaic(rel, on=False)
    res = B.macau(rd, num_latent=D, burnin=1, psamples=1, verbose=False, engine=eng, reset_model=False)
    assert "WAIC" not in res
    eng.close()


# ---- (d) quality ----------------------------------------------------------------------------------------------------------------
def test_waic_and_the_held_out_lpd_choose_the_planted_rank(B):
    """The planted rank-3 Gaussian data of waic_restatement.planted_gauss (60 x 40, a random half of the cells the training table,
    the other half held out), alpha = 4 fixed, 30 + 30 iterations, seed 1, fitted at num_latent = 3 and at num_latent = 1.  The
    elpd per training cell (WAIC, from the training half alone) of the first fit must exceed the second's by at least half the
    smallest of the three gaps that the CPU restatement of both fits gives on the seeds 2, 3, 4 (QUALITY_ELPD_GAPS, recorded in
    DESIGN.md section 17), and the held-out LPD of the other half must order the two fits the same way."""
    ids, y, n_test = WR.planted_gauss()
    N1, N2, _ = WR.QUALITY_SHAPE

    def device(D):
        rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "planted", [B.Entity("u"), B.Entity("v")], alpha=WR.QUALITY_ALPHA, dims=[N1, N2])
        B.assignToTest(rel, np.arange(len(y) - n_test + 1, len(y) + 1))
        B.setWaic(rel)
        rd = B.RelationData(rel)
        res = B.macau(rd, num_latent=D, burnin=WR.QUALITY_ITERS[0], psamples=WR.QUALITY_ITERS[1], verbose=False, seed=1, lpd=True)
        rd._engine.close()
        w = res["WAIC"]
        assert w["n"] == len(y) - n_test and math.isfinite(w["se"]) and w["n_high"] < w["n"] // 2
        return w["elpd"] / w["n"], float(res["LPD"])

    (e3, l3), (e1, l1) = device(3), device(1)
    margin = 0.5 * min(WR.QUALITY_ELPD_GAPS)
    print(f"rank by WAIC: elpd per cell {e3:.4f} at D = 3, {e1:.4f} at D = 1, gap {e3 - e1:.4f} (asserted: at least {margin:.4f}); "
          f"held-out LPD {l3:.4f} and {l1:.4f}, gap {l3 - l1:.4f}")
    assert margin > 0.0 and e3 - e1 >= margin, (e3, e1, margin)
    assert l3 > l1, (l3, l1)
