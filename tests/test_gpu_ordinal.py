"""The ordinal probit noise model on the GPU: bdf_ordinal_step against the numpy restatement
(tests/ordinal_restatement.py), whole macau(lpd=True) iterations on ordinal relations against the restated chain on both iteration
paths, fixed edges against setBinned, the Gaussian chain untouched by an ordinal engine in the same process, the edges and the
held-out log predictive density on planted data with unevenly spaced levels, and the errors of the C ABI."""
import ctypes as C
import os
import textwrap

import numpy as np
import pytest

from both_paths import child
import ordinal_restatement as OR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.inf


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


# ---- (1) the step -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sort", [False, True])
@pytest.mark.parametrize("n_modes", [2, 3])
@pytest.mark.parametrize("D", [1, 7, 10, 32, 64])
def test_ordinal_step_matches_the_restatement(B, ctx, D, n_modes, sort):
    """K in {4, 5, 16}, 1,003 cells (no multiple of 8 or 256), one level empty (several at K = 16), alpha from the host and from
    the device; four steps in a row from the edges k + 1/2 with step size 0.3, the first two adapting.  The proposal and its
    Jacobian term to 1e-12; S to 8e-9 absolute -- 2 evaluations x 4e-12 (DESIGN.md section 15's bound on the log mass) x n; then
    the same decision (the restated margins |log u - S| are 3 and more: test_ordinal_host.py), and with it the edges, the step
    size, the counters and the rows' bounds."""
    import torch
    from bdf_amd._lib import check, lib
    worst_S = 0.0
    decisions = []
    for K in (4, 5, 16):
        ids, S, mean, codes, dims = OR.step_case(D, n_modes, K)
        n = len(codes)
        ref = OR.step_sequence(D, n_modes, K)
        pairs = B.DevicePairs(ctx, ids, codes.astype(np.float64))
        if sort:
            pairs.sort(n_modes - 1)
        St = [ctx.tensor(s) for s in S]
        cd = ctx.tensor(codes, dtype=torch.int8)
        for through_dev in (False, True):
            # through alpha_dev the scalar argument is a decoy: the device value wins
            a_arg = ctx.tensor([OR.STEP_ALPHA]) if through_dev else OR.STEP_ALPHA
            o = B.DeviceOrdinal(ctx, K, OR.STEP_START, 3)                # (a trace of three rows for four steps: the fourth is not kept)
            if through_dev:
                o.set_adapt(2)                                           # adapt = -1: the object's own count decides
            start = OR.bounds_of(codes, OR.start_edges(K))
            bd = ctx.tensor(start)
            e_dev = OR.start_edges(K)[1:K]
            for k, (sweep, want) in enumerate(zip(OR.STEP_SWEEPS, ref)):
                ctx.set_sweep(sweep)
                if through_dev:
                    fp = (C.c_void_p * len(St))(*[t.data_ptr() for t in St])
                    check(lib().bdf_ordinal_step(ctx.handle, o.handle, pairs.handle, _p(cd), D, fp, mean, 123.0, _p(a_arg), 1, -1, _p(bd)))
                else:
                    o.step(ctx, pairs, cd, D, St, mean, a_arg, 1, 1 if k < 2 else 0, bd)
                prop, got = o.proposal(), o.read(min(k + 1, 3))
                assert np.abs(prop["edges"] - want["prop"][1:K]).max() <= 1e-12, (K, k)
                assert abs(prop["jacobian"] - want["jac"]) <= 1e-12
                assert abs(prop["log_u"] - want["log_u"]) <= 1e-14 * max(1.0, abs(want["log_u"]))
                assert np.isfinite(got["S"])
                worst_S = max(worst_S, abs(got["S"] - want["S"]))
                assert abs(got["S"] - want["S"]) <= 8e-9, (K, k, through_dev, got["S"], want["S"])
                assert prop["accepted"] == want["accepted"]
                decisions.append(prop["accepted"])
                # accepted: the proposal is published as it is; refused: the edges are what they were, bit for bit
                e_dev = prop["edges"] if prop["accepted"] else e_dev
                assert np.array_equal(got["edges"], e_dev) and np.abs(got["edges"] - want["e"][1:K]).max() <= 1e-12
                assert got["edges"][0] == 1.5 and got["edges"][-1] == K - 0.5
                assert abs(got["sigma"] - want["sigma"]) <= 1e-13 * want["sigma"]
                assert (got["proposals"], got["accepts"]) == (want["proposals"], want["accepts"])
                full = np.concatenate([[-INF], got["edges"], [INF]])
                assert np.array_equal(bd.cpu().numpy(), OR.bounds_of(codes, full))               # the caller's order, sorted or not
                if k < 3:
                    assert np.array_equal(got["trace"][k], got["edges"])
            assert ref[1]["sigma"] != OR.STEP_START and ref[3]["sigma"] == ref[1]["sigma"]       # two steps adapted, two did not
            tb = ctx.tensor(np.full((7, 2), np.nan))
            o.bounds(ctx, cd[:7], tb)                                    # the other entry point: any codes, from the current edges
            assert np.array_equal(tb.cpu().numpy(), OR.bounds_of(codes[:7], full))
            o.close()
        pairs.close()
    print(f"ordinal step D={D} modes={n_modes} sort={sort}: max |S_dev - S_ref| = {worst_S:.3e} over 24 steps, {sum(decisions)} accepted")


def test_ordinal_step_far_tails_stay_finite(B, ctx):
    """alpha = 900 and levels that have nothing to do with the means: cells up to 100 standard deviations from their bin, far
    beyond the 37 at which Phi underflows.  S is finite.  It also agrees with the restatement to 1e-9 of the sum of the terms' sizes:
    a term of size alpha d^2 / 2 (5,000 at d = 3.3) moves by alpha d = 3,000 times the last bit of m, 1e-15, between the device's dot
    product and numpy's -- 1e-15 of its size -- and the deep-tail form of the log mass is good to as much."""
    import torch
    rng = np.random.default_rng(11)
    K, D, n = 5, 10, 1003
    ids, S, mean, _, dims = OR.step_case(D, 2, K)
    codes = rng.integers(1, K + 1, n).astype(np.int8)
    m = OR.udot(ids, S) + mean
    sd = np.abs(m - codes) * 30.0
    assert np.count_nonzero(sd > 37.0 + 15.0) > 100
    pairs = B.DevicePairs(ctx, ids, codes.astype(np.float64))
    St, cd, bd = [ctx.tensor(s) for s in S], ctx.tensor(codes, dtype=torch.int8), ctx.tensor(OR.bounds_of(codes, OR.start_edges(K)))
    o = B.DeviceOrdinal(ctx, K, 0.05, 1)
    st = OR.State(K, 0.05)
    ctx.set_sweep(9)
    o.step(ctx, pairs, cd, D, St, mean, 900.0, 2, 0, bd)
    want = st.step(m, codes, 900.0, 1234, 9, 2, False)
    got = o.read()
    size = np.abs(OR.LR.lpd_mass(m, *OR.bounds_of(codes, want["prop"]).T, 900.0)).sum()
    print(f"far tails: S_dev = {got['S']:.6f}, S_ref = {want['S']:.6f}, sum of |log mass| = {size:.3e}")
    assert np.isfinite(got["S"]) and np.isfinite(want["S"])
    assert abs(got["S"] - want["S"]) <= 1e-9 * size
    assert o.proposal()["accepted"] == want["accepted"]
    o.close()
    pairs.close()


# ---- (2) whole iterations -----------------------------------------------------------------------------------------------------
CASES = OR.ITERATION_CASES

CHILD = textwrap.dedent('''
    import sys
    import numpy as np
    sys.path.insert(0, %r); sys.path.insert(0, %r)
    import bdf_amd as B
    import ordinal_restatement as OR
    out, d = sys.argv[1], {}
    for n_modes in (2, 3):
        for with_feat in (0, 1):
            for alpha_sample in (0, 1):
                ids, lev, dims, D, feats, n_test, alpha, _ = OR.iteration_case(n_modes, with_feat, alpha_sample)
                names = ["a", "b", "c"][:n_modes]
                ents = [B.Entity(nm, F=feats[k]) for k, nm in enumerate(names)]
                table = {nm: ids[:, k] for k, nm in enumerate(names)}
                table["y"] = lev
                rel = B.Relation(table, "ord", ents, alpha=alpha, dims=list(dims))
                rel.model.alpha_sample = bool(alpha_sample)
                B.assignToTest(rel, np.arange(1, n_test + 1))
                B.setOrdinal(rel)
                B.setTestOrdinal(rel)
                rd = B.RelationData(rel)
                res = B.macau(rd, num_latent=D, burnin=2, psamples=2, verbose=False, seed=OR.ITERATION_SEED, lpd=True)
                key = "%%d%%d%%d_" %% (n_modes, with_feat, alpha_sample)
                d[key + "native"], d[key + "pred"] = np.array(int(rd._engine.native)), res["predictions"]["pred"].to_numpy()
                d[key + "lpd"], d[key + "LPD"] = res["predictions"]["lpd"].to_numpy(), np.array(res["LPD"])
                d[key + "mean"], d[key + "alpha"] = np.array(rel.model.mean_value), np.array(rel.model.alpha)
                d[key + "trace"], d[key + "edges"], d[key + "last"] = res["ordinal"]["edges_trace"], res["ordinal"]["edges"], rel.model.ordinal_edges
                d[key + "step"], d[key + "accept"] = np.array(res["ordinal"]["step"]), np.array(res["ordinal"]["accept"])
                d[key + "full"] = rd._engine.rel[0].ordinal.read(4)["trace"]
                for k, en in enumerate(rd.entities):
                    d[key + "S%%d" %% k], d[key + "mu%%d" %% k], d[key + "Lam%%d" %% k] = en.model.sample.T, en.model.mu, en.model.Lambda
                    if feats[k] is not None:
                        d[key + "beta%%d" %% k], d[key + "lb%%d" %% k] = en.model.beta, np.array(en.lambda_beta)
                rd._engine.close()
    np.savez(out, **d)
''') % (ROOT, os.path.join(ROOT, "tests"))


@pytest.fixture(scope="module")
def chains():
    """2 + 2 iterations of every case of CASES on the native and on the step-by-step path: one child process per path"""
    return child(CHILD, no_native=False), child(CHILD, no_native=True)


@pytest.fixture(scope="module")
def restated():
    """the restated chain of every case (test_ordinal_host.py checks that across them proposals are accepted and refused, none on
    a knife's edge)"""
    return OR.restated_iterations()


@pytest.mark.parametrize("n_modes,with_feat,alpha_sample", CASES)
def test_ordinal_whole_iterations_match_the_restatement_on_both_paths(chains, restated, n_modes, with_feat, alpha_sample):
    ids, lev, dims, D, feats, n_test, alpha, _ = OR.iteration_case(n_modes, with_feat, alpha_sample)
    key = "%d%d%d_" % (n_modes, with_feat, alpha_sample)
    nat, step = ({k[len(key):]: v for k, v in ch.items() if k.startswith(key)} for ch in chains)
    assert nat["native"] == 1 and step["native"] == 0
    assert sorted(nat) == sorted(step) and len(nat) >= 12 + 3 * n_modes
    for k in nat:
        if k != "native":
            assert np.array_equal(nat[k], step[k]), k       # the two paths enqueue the same launches: the same bits
    ref = restated[(n_modes, with_feat, alpha_sample)]
    tol = dict(rtol=1e-6, atol=1e-6)
    assert abs(nat["mean"] - ref["mean"]) <= 1e-12
    np.testing.assert_allclose(nat["alpha"], ref["alpha"], rtol=1e-6)
    assert (nat["alpha"] != alpha) == bool(alpha_sample)
    for k in range(n_modes):
        np.testing.assert_allclose(nat["S%d" % k], ref["S"][k], err_msg="sample of entity %d" % k, **tol)
        np.testing.assert_allclose(nat["mu%d" % k], ref["mu"][k], **tol)
        np.testing.assert_allclose(nat["Lam%d" % k], ref["Lam"][k], **tol)
        if feats[k] is not None:
            eb = np.abs(nat["beta%d" % k] - ref["beta"][k])
            print(f"ordinal chain {key}: beta of entity {k} within {eb.max():.2e} (relative to 1e-6 + 1e-6 |beta|: "
                  f"{(eb / (1e-6 + 1e-6 * np.abs(ref['beta'][k]))).max():.2e}), lambda_beta within {abs(nat['lb%d' % k] - ref['lb'][k]) / ref['lb'][k]:.2e} relative")
            np.testing.assert_allclose(nat["beta%d" % k], ref["beta"][k], err_msg="beta of entity %d" % k, **tol)
            assert abs(nat["lb%d" % k] - ref["lb"][k]) <= 1e-6 * ref["lb"][k]
    np.testing.assert_allclose(nat["pred"], ref["pred"], **tol)
    np.testing.assert_allclose(nat["lpd"], ref["lpd"], **tol)
    assert abs(nat["LPD"] - ref["LPD"]) <= 1e-6
    # the edges: every iteration's, the posterior mean, the last draw, the step size (adapted in the burn-in, then frozen)
    np.testing.assert_allclose(nat["full"], ref["edges_trace"], **tol)
    assert np.array_equal(nat["trace"], nat["full"][2:]) and np.array_equal(nat["last"], nat["full"][3])
    np.testing.assert_allclose(nat["edges"], ref["edges_trace"][2:].mean(axis=0), **tol)
    np.testing.assert_allclose(nat["step"], ref["sigma"], rtol=1e-6)
    assert nat["step"] != 0.1 and nat["accept"] == ref["accepted"][2:].mean()
    assert np.all(nat["full"][:, 0] == 1.5) and np.all(nat["full"][:, -1] == 4.5) and np.all(np.diff(nat["full"], axis=1) > 0)


# ---- (3) fixed edges are setBinned --------------------------------------------------------------------------------------------
def test_fixed_edges_are_the_binned_chain_bit_for_bit(B):
    ids, lev, dims, D, _, n_test, alpha, _ = OR.iteration_case(2, False, True)

    def run(ordinal):
        rel = B.Relation({"a": ids[:, 0], "b": ids[:, 1], "y": lev}, "r", [B.Entity("a"), B.Entity("b")], alpha=alpha, dims=list(dims))
        rel.model.alpha_sample = True
        B.assignToTest(rel, np.arange(1, n_test + 1))
        if ordinal:
            B.setOrdinal(rel, sample_edges=False)
            B.setTestOrdinal(rel)
        else:
            B.setBinned(rel, [1.5, 2.5, 3.5, 4.5])
            B.setTestBinned(rel, [1.5, 2.5, 3.5, 4.5])
        rd = B.RelationData(rel)
        res = B.macau(rd, num_latent=D, burnin=2, psamples=2, verbose=False, seed=5, lpd=True)
        out = [en.model.sample.copy() for en in rd.entities] + [res["predictions"]["pred"].to_numpy(), res["predictions"]["lpd"].to_numpy(),
                                                               np.array([res["LPD"], res["RMSE"], rel.model.alpha])]
        assert rd._engine.rel[0].ordinal is None
        rd._engine.close()
        return out, res

    (fixed, res), (binned, _) = run(True), run(False)
    for a, b in zip(fixed, binned):
        assert np.array_equal(a, b)
    assert np.array_equal(res["ordinal"]["edges"], [1.5, 2.5, 3.5, 4.5]) and res["ordinal"]["accept"] == 0.0
    assert np.array_equal(res["ordinal"]["edges_trace"], np.tile([1.5, 2.5, 3.5, 4.5], (2, 1)))


# ---- (4) nothing else moved ---------------------------------------------------------------------------------------------------
def test_gaussian_chain_is_untouched_by_an_ordinal_engine_in_the_process(B):
    ids, lev, n_test = OR.planted_ordinal(seed=5, N1=120, N2=90, n_cells=4000, n_test=500)

    def gaussian():
        rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": lev + 0.25 * (ids[:, 0] % 3)}, "g", [B.Entity("u"), B.Entity("v")], dims=[120, 90])
        B.assignToTest(rel, np.arange(4000 - n_test + 1, 4001))
        rd = B.RelationData(rel)
        res = B.macau(rd, num_latent=16, burnin=2, psamples=2, verbose=False, seed=17)
        out = [en.model.sample.copy() for en in rd.entities] + [res["predictions"]["pred"].to_numpy().copy()]
        rd._engine.close()
        return out

    alone = gaussian()
    rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": lev}, "o", [B.Entity("u"), B.Entity("v")], dims=[120, 90])
    B.assignToTest(rel, np.arange(4000 - n_test + 1, 4001))
    B.setOrdinal(rel)
    B.setTestOrdinal(rel)
    rdo = B.RelationData(rel)
    res = B.macau(rdo, num_latent=16, burnin=1, psamples=1, verbose=False, seed=17, lpd=True)
    assert res["ordinal"]["edges_trace"].shape == (1, 5)
    beside = gaussian()                                     # the ordinal engine is alive: its object, its codes, its rewritten bounds
    assert rdo._engine.rel[0].ordinal is not None
    for a, b in zip(alone, beside):
        assert np.array_equal(a, b)
    # the edges' trace and burn-in cover one run: a chain whose edges have moved is not continued
    with pytest.raises(B.ArgumentError, match="new engine"):
        B.macau(rdo, num_latent=16, burnin=0, psamples=1, verbose=False, seed=17, engine=rdo._engine, reset_model=False)
    rdo._engine.close()


# ---- (5) quality --------------------------------------------------------------------------------------------------------------
def test_ordinal_quality_on_planted_data(B):
    """Planted data (rank 4, 300 x 200, 9,000 training and 3,000 held-out cells, noise precision 6.25) in six levels cut at 1.5,
    2.06, 3.66, 4.22, 5.5 -- the two middle levels four times as wide as their neighbours.  macau(lpd=True) with D = 8,
    alpha = 6.25, 60 + 60 iterations.  With setOrdinal every interior posterior-mean edge must lie nearer its planted value than
    its start k + 1/2, and the held-out LPD must exceed that of sample_edges=False (edges fixed at k + 1/2) by at least half the
    smallest gain the CPU restatement shows over the seeds 2, 3, 4.  The restatement gives gains of 0.1174, 0.1127 and 0.1219 nats
    per cell (LPD -0.7481 / -0.8655, -0.7406 / -0.8533, -0.7414 / -0.8633; edges 2.07 - 2.08, 3.72 - 3.76, 4.31 - 4.32), recorded as
    ordinal_restatement.PLANTED_GAINS and recomputed by test_ordinal_host.py, so the bound is 0.0564.  A model that never moves
    its edges gains 0."""
    ids, lev, n_test = OR.planted_ordinal()
    D, burnin, psamples, alpha = 8, 60, 60, 6.25
    n = len(lev)

    def device(sample_edges):
        rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": lev}, "planted", [B.Entity("u"), B.Entity("v")], alpha=alpha, dims=[300, 200])
        B.assignToTest(rel, np.arange(n - n_test + 1, n + 1))
        B.setOrdinal(rel, sample_edges=sample_edges)
        B.setTestOrdinal(rel)
        rd = B.RelationData(rel)
        res = B.macau(rd, num_latent=D, burnin=burnin, psamples=psamples, verbose=False, seed=1, lpd=True)
        rd._engine.close()
        return res

    sampled, fixed = device(True), device(False)
    gains = OR.PLANTED_GAINS
    edges = sampled["ordinal"]["edges"]
    print(f"ordinal quality: device LPD {sampled['LPD']:.4f} with sampled edges, {fixed['LPD']:.4f} with fixed ones, gain "
          f"{sampled['LPD'] - fixed['LPD']:.4f}; edges {np.round(edges, 3)}, acceptance {sampled['ordinal']['accept']:.2f}, step "
          f"{sampled['ordinal']['step']:.3f}; the restatement's recorded gains {gains[0]:.4f} {gains[1]:.4f} {gains[2]:.4f}")
    planted = np.array(OR.PLANTED_EDGES)
    start = np.arange(1, 6) + 0.5
    assert edges[0] == 1.5 and edges[-1] == 5.5
    assert np.all(np.abs(edges[1:-1] - planted[1:-1]) < np.abs(edges[1:-1] - start[1:-1])), edges
    assert sampled["LPD"] - fixed["LPD"] >= 0.5 * min(gains), (sampled["LPD"], fixed["LPD"], gains)


# ---- (6) errors through the C ABI ---------------------------------------------------------------------------------------------
def test_ordinal_c_abi_errors(B, ctx):
    import torch
    from bdf_amd._lib import check, lib
    ids, S, mean, codes, dims = OR.step_case(10, 2, 5)
    pairs = B.DevicePairs(ctx, ids, codes.astype(np.float64))
    St = [ctx.tensor(s) for s in S]
    fp = (C.c_void_p * 2)(*[t.data_ptr() for t in St])
    cd, bd = ctx.tensor(codes, dtype=torch.int8), ctx.tensor(OR.bounds_of(codes, OR.start_edges(5)))
    h = C.c_void_p()
    for K, step, cap, out in ((3, 0.1, 0, C.byref(h)), (17, 0.1, 0, C.byref(h)), (5, 0.0, 0, C.byref(h)), (5, 11.0, 0, C.byref(h)),
                              (5, float("nan"), 0, C.byref(h)), (5, 0.1, -1, C.byref(h)), (5, 0.1, 0, None)):
        with pytest.raises(B.ArgumentError, match="bdf_ordinal_create"):
            check(lib().bdf_ordinal_create(ctx.handle, K, step, cap, out))
    with pytest.raises(B.ArgumentError, match="bdf_ordinal_create"):
        check(lib().bdf_ordinal_create(None, 5, 0.1, 0, C.byref(h)))
    o = B.DeviceOrdinal(ctx, 5, 0.1, 2)

    def step(ord_h=o.handle, train=pairs.handle, c=_p(cd), D=10, f=fp, a=1.0, a_dev=None, adapt=0, b=_p(bd)):
        check(lib().bdf_ordinal_step(ctx.handle, ord_h, train, c, D, f, mean, a, _p(a_dev), 1, adapt, b))

    for bad in (dict(ord_h=None), dict(train=None), dict(c=None), dict(f=None), dict(b=None), dict(D=0), dict(D=65), dict(a=0.0), dict(a=-1.0),
                dict(a=float("nan")), dict(a=float("inf")), dict(adapt=2), dict(adapt=-2), dict(b=C.c_void_p(bd.data_ptr() + 8))):
        with pytest.raises(B.ArgumentError, match="bdf_ordinal_step"):
            step(**bad)
    with pytest.raises(B.ArgumentError, match="bdf_ordinal_bounds"):
        check(lib().bdf_ordinal_bounds(ctx.handle, o.handle, _p(cd), 5, C.c_void_p(bd.data_ptr() + 8)))
    with pytest.raises(B.ArgumentError, match="bdf_ordinal_bounds"):
        check(lib().bdf_ordinal_bounds(ctx.handle, None, _p(cd), 5, _p(bd)))
    with pytest.raises(B.ArgumentError, match="bdf_ordinal_bounds"):
        check(lib().bdf_ordinal_bounds(ctx.handle, o.handle, None, 5, _p(bd)))
    with pytest.raises(B.ArgumentError, match="bdf_ordinal_read"):
        o.read(3)                                            # the object keeps two rows
    with pytest.raises(B.ArgumentError, match="bdf_ordinal_read"):
        check(lib().bdf_ordinal_read(o.handle, None, None, None, None, None, None, 1))
    with pytest.raises(B.ArgumentError, match="bdf_ordinal_set_adapt"):
        o.set_adapt(-1)
    got = o.read(2)                                          # nothing above took a step
    assert got["proposals"] == 0 and np.array_equal(got["edges"], [1.5, 2.5, 3.5, 4.5]) and np.all(np.isnan(got["trace"]))
    step(a=0.0, a_dev=ctx.tensor([2.0]))                     # alpha_dev wins over the scalar
    assert o.read(1)["proposals"] == 1
    o.close()
    pairs.close()
