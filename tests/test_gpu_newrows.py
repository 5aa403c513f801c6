"""Cells of new rows on the GPU (setNewRows / setNewTest): bdf_newrows_quad and bdf_newrows_update through the C
ABI against the numpy restatement (tests/newrows_restatement.py), whole macau() runs on planted Macau data against the restatement
driven by the per-iteration device state on both iteration paths, the run untouched by the setters' absence, and the quality of the
cold-start predictions against the CPU chains of the restatement's own sampler."""
import ctypes as C
import math
import os
import re
import textwrap

import numpy as np
import pytest

from both_paths import child
import newrows_restatement as NR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 64                          # BDF_NEWROWS_TILE: rows of V a workgroup of the quad kernel takes
GROUP = 256                        # cells a workgroup of the update takes (32 groups of 8 lanes)
FINAL = 256                        # partial sums the scalars' final reduction takes in one pass (one per thread)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _spd(rng, D):
    A = rng.standard_normal((D, D))
    L = A @ A.T / D + np.eye(D)
    return 0.5 * (L + L.T)


# ---- (a) bdf_newrows_quad ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 3, 4, 5, 16, 17, 32, 33, 63, 64])
def test_quad_matches_the_restatement(B, ctx, D):
    """q = v' Lambda^-1 v against np.linalg.solve for M in {1, 15, 16, 17, a workgroup's tile - 1, the tile, the tile + 1, three
    workgroups + 1}, Lambda = A A' / D + I (cond <= ~1e3): relative 1e-10 (the bound D eps cond is ~6e-12), q >= 0 everywhere, a
    second run the same bits, and nothing written behind the M-th entry"""
    from bdf_amd._lib import check, lib
    rng = np.random.default_rng(100 + D)
    worst = 0.0
    for M in (1, 15, 16, 17, TILE - 1, TILE, TILE + 1, 3 * TILE + 1):
        Lam, V = _spd(rng, D), rng.standard_normal((M, D))
        assert np.linalg.cond(Lam) < 2e3
        Lt, Vt = ctx.tensor(Lam), ctx.tensor(V)
        runs = []
        for _ in range(2):
            q = ctx.tensor(np.full(M + 8, -7.0))
            check(lib().bdf_newrows_quad(ctx.handle, D, M, _p(Lt), _p(Vt), _p(q)))
            ctx.sync()
            runs.append(q.cpu().numpy())
        got, ref = runs[0], NR.quad(Lam, V)
        assert np.array_equal(runs[0], runs[1])
        assert np.array_equal(got[M:], np.full(8, -7.0))
        assert np.all(got[:M] >= 0.0)
        e = (np.abs(got[:M] - ref) / ref).max()
        worst = max(worst, e)
        assert e <= 1e-10, (D, M, e)
    print(f"quad D={D}: worst relative error {worst:.2e} (asserted: 1e-10)")


def test_quad_raises_notpd_and_does_not_fault(B):
    """a Lambda with a negative eigenvalue: the context's NOTPD flag at the next sync (once), and a clean call afterwards"""
    from bdf_amd._lib import check, lib
    ctx = B.Context(seed=5)
    rng = np.random.default_rng(3)
    D, M = 12, 70
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    ev = np.linspace(0.5, 3.0, D)
    ev[4] = -0.7
    bad = (Q * ev) @ Q.T
    bad = 0.5 * (bad + bad.T)
    V = ctx.tensor(rng.standard_normal((M, D)))
    q = ctx.zeros(M)
    check(lib().bdf_newrows_quad(ctx.handle, D, M, _p(ctx.tensor(bad)), _p(V), _p(q)))
    with pytest.raises(B.NotPositiveDefinite):
        ctx.sync()
    ctx.sync()
    good = _spd(rng, D)
    check(lib().bdf_newrows_quad(ctx.handle, D, M, _p(ctx.tensor(good)), _p(V), _p(q)))
    ctx.sync()
    assert np.allclose(q.cpu().numpy(), NR.quad(good, V.cpu().numpy()), rtol=1e-10)
    for bad_args in ((None, D, M, _p(V), _p(V), _p(q)), (ctx.handle, 0, M, _p(V), _p(V), _p(q)), (ctx.handle, 65, M, _p(V), _p(V), _p(q)),
                     (ctx.handle, D, -1, _p(V), _p(V), _p(q)), (ctx.handle, D, M, None, _p(V), _p(q)), (ctx.handle, D, M, _p(V), None, _p(q))):
        with pytest.raises(B.ArgumentError, match="bdf_newrows_quad"):
            check(lib().bdf_newrows_quad(*bad_args))
    ctx.close()


# ---- (b) bdf_newrows_update -------------------------------------------------------------------------------------------------------
def _state(B, pairs):
    """the running state in the CALLER's order: (5, n) -- mean, M2, sum q, M, A -- and the draws it holds"""
    from bdf_amd._lib import check, lib
    st, draws = C.c_void_p(), C.c_double()
    check(lib().bdf_newrows_state(pairs.handle, C.byref(st), C.byref(draws)))
    raw = np.zeros((5, pairs.n))
    if st.value and pairs.n:
        check(lib().bdf_d2h(pairs.ctx.handle, raw.ctypes.data_as(C.c_void_p), st, raw.size * 8))
    if pairs._order is not None:
        out = np.empty_like(raw)
        out[:, pairs._order] = raw
        raw = out
    return raw, draws.value


UPDATE_CASES = [(1, 16), (GROUP - 1, 16), (GROUP, 16), (GROUP + 1, 7), (GROUP + 1, 32), (GROUP + 1, 64), (GROUP * (FINAL + 1) + 3, 16)]


@pytest.mark.parametrize("probit", [False, True])
@pytest.mark.parametrize("n,D", UPDATE_CASES)
def test_update_matches_the_restatement(B, ctx, n, D, probit):
    """The phase sequence 0, 0, 1, 2, 2, 2, 2 with fresh factors (and a fresh Lambda, so a fresh q) at every step, on n cells of 13 new
    rows x 29 columns of which about a fifth have a NaN value, for four settings: alpha by value / through alpha_dev (with a decoy
    scalar), clamping off / on, pairs unsorted / sorted.  n: 1; one fewer, as many as and one more than a workgroup takes (one more
    also at D = 7, 32, 64: the three shapes of the gather); and 256 x 257 + 3 cells, whose 258 partial sums are more than the final
    reduction's 256 threads take in one pass.

    The restated maps take the predictive mean m that the device's own gather forms (bdf_predict on the same cells: the same dot
    product in the same order), after it is checked against numpy to the rounding of its D + 1 additions -- as test_gpu_waic.py does.
    Then: the state's mean, M2 and sum q to 1e-12 relative to max(|value|, the size of what is summed: max |p| for the mean, its
    square for M2); lpd to 1e-9 absolute, the scalars to 1e-9 relative to max(1, |value|), the counts exactly -- the tolerances of
    test_gpu_waic.py for the same maps.  Phase 0 leaves the state bit for bit.  Sorted and unsorted pairs give the same
    bdf_newrows_result in the caller's order, bit for bit."""
    from bdf_amd._lib import check, lib
    rng = np.random.default_rng(9000 + 10 * D + n % 1000 + probit)
    n_new, M, mean = 13, 29, (0.0 if probit else 0.3)
    ids = np.stack([rng.integers(1, n_new + 1, n), rng.integers(1, M + 1, n)], axis=1)
    y = (rng.random(n) < 0.5).astype(np.float64) if probit else rng.standard_normal(n)
    y[rng.random(n) < 0.2] = np.nan
    if n > 1:
        y[0], y[1 % n] = (1.0 if probit else 0.25), np.nan
    plain = B.DevicePairs(ctx, ids, np.zeros(n))             # the device's own gather, identity link, the caller's order
    steps = []
    for phase in (0, 0, 1, 2, 2, 2, 2):
        uh, V, Lam = rng.standard_normal((n_new, D)) * 0.6, rng.standard_normal((M, D)) * 0.6, _spd(rng, D)
        q = NR.quad(Lam, V)
        ut, vt = ctx.tensor(uh), ctx.tensor(V)
        m = plain.predict(D, [ut, vt], mean).cpu().numpy()
        scale = np.abs(uh[ids[:, 0] - 1] * V[ids[:, 1] - 1]).sum(axis=1) + abs(mean)
        assert np.all(np.abs(m - NR.cells(ids, uh, V, q, mean)[0]) <= 4e-16 * (D + 2) * scale)
        steps.append((phase, ut, vt, ctx.tensor(q), m, q[ids[:, 1] - 1]))
    results = {}
    worst = dict(state=0.0, lpd=0.0, stats=0.0)
    for through_dev, clamp, sort in ((False, (), False), (True, (-0.4, 0.8), True), (False, (0.1, 0.9), True), (True, (), False)):
        alpha = 2.5
        pairs = B.DevicePairs(ctx, ids, y)
        if sort:
            pairs.sort(1)
        if probit:
            pairs.set_link(1)
        a_arg, a_dev = (alpha, None) if not through_dev else (123.0, ctx.tensor([alpha]))
        lo, hi = clamp if len(clamp) else (1.0, -1.0)
        cut = 0.5 if probit else 0.1
        stats, out = ctx.zeros(8), ctx.tensor(np.full((n, 3), -5.0))
        st = NR.Stream()
        for phase, ut, vt, qt, m, qc in steps:
            before = _state(B, pairs) if st.draws else None
            check(lib().bdf_newrows_update(ctx.handle, pairs.handle, D, _p(ut), _p(vt), _p(qt), mean, a_arg, _p(a_dev), phase, lo, hi, cut, 1, _p(stats)))
            ctx.sync()
            s = stats.cpu().numpy()
            p, l = NR.predict(probit, m, qc), NR.loglik(probit, y, m, qc, alpha)
            avg, lpd = st.update(p, qc, l, phase)
            ref = NR.scalars(y, avg, p, lpd, l, clamp, cut, True)
            assert np.all(np.isfinite(s)) and s[7] == 0.0
            assert s[2] == ref[2] and s[3] == ref[3] and s[4] == ref[4] == float(np.sum(~np.isnan(y)))
            for k in (0, 1, 5, 6):
                e = abs(s[k] - ref[k]) / max(1.0, abs(ref[k]))
                worst["stats"] = max(worst["stats"], e)
                assert e <= 1e-9, (through_dev, clamp, sort, phase, k, s[k], ref[k])
            state, draws = _state(B, pairs)
            if phase == 0:
                assert s[0] == s[1] and s[2] == s[3] and s[5] == s[6] and draws == st.draws
                if before is not None:
                    assert np.array_equal(state, before[0])
                continue
            assert draws == st.draws
            P = max(1.0, np.abs(p).max(), np.abs(st.mean).max())
            for got, want, size in ((state[0], st.mean, P), (state[1], st.M2, P * P), (state[2], st.sq, 0.0)):
                e = (np.abs(got - want) / np.maximum(np.abs(want), size + 1e-300)).max()
                worst["state"] = max(worst["state"], e)
                assert e <= 1e-12, (through_dev, clamp, sort, phase, e)
            check(lib().bdf_newrows_result(ctx.handle, pairs.handle, _p(out)))
            ctx.sync()
            o = out.cpu().numpy()
            has = ~np.isnan(y)
            assert np.array_equal(o[:, 0], state[0]) and np.array_equal(np.isnan(o[:, 2]), ~has)
            e = np.abs(o[has, 2] - lpd[has]).max() if has.any() else 0.0
            worst["lpd"] = max(worst["lpd"], e)
            assert e <= 1e-9, (through_dev, clamp, sort, phase, e)
            sd = st.stdev(probit)
            assert np.array_equal(np.isnan(o[:, 1]), np.isnan(sd))
            if st.draws >= 2:
                assert np.all(np.abs(o[:, 1] - sd) <= 1e-9 * np.maximum(1.0, sd))
        results[(through_dev, clamp, sort)] = out.cpu().numpy().copy()
        pairs.close()
    # the same alpha by value and through alpha_dev, sorted and unsorted (no clamp touches the state): the same result, the caller's order
    assert np.array_equal(results[(False, (), False)], results[(True, (), False)], equal_nan=True)
    assert np.array_equal(results[(False, (), False)], results[(True, (-0.4, 0.8), True)], equal_nan=True)
    print(f"newrows update n={n} D={D} probit={probit}: worst relative error of the state {worst['state']:.2e}, absolute of lpd {worst['lpd']:.2e}, "
          f"relative of a scalar {worst['stats']:.2e}")
    plain.close()


def test_update_of_cells_without_a_value_and_refusals(B, ctx):
    """a cell list that is all NaN: every scalar 0, the count 0, no NaN in them, predictions all the same; score_lpd = 0: no lpd;
    and what the C ABI refuses"""
    from bdf_amd._lib import check, lib
    rng = np.random.default_rng(77)
    n, D, n_new, M = GROUP + 1, 8, 5, 9
    ids = np.stack([rng.integers(1, n_new + 1, n), rng.integers(1, M + 1, n)], axis=1)
    ut, vt = ctx.tensor(rng.standard_normal((n_new, D))), ctx.tensor(rng.standard_normal((M, D)))
    qt = ctx.tensor(rng.random(M) + 0.1)
    pairs = B.DevicePairs(ctx, ids, np.full(n, np.nan))
    stats, out = ctx.tensor(np.full(8, 7.0)), ctx.zeros((n, 3))
    for phase in (0, 1, 2):
        check(lib().bdf_newrows_update(ctx.handle, pairs.handle, D, _p(ut), _p(vt), _p(qt), 0.2, 2.0, None, phase, 1.0, -1.0, 0.0, 1, _p(stats)))
        ctx.sync()
        assert np.array_equal(stats.cpu().numpy(), np.zeros(8))
    check(lib().bdf_newrows_result(ctx.handle, pairs.handle, _p(out)))
    ctx.sync()
    o = out.cpu().numpy()
    m = 0.2 + np.sum(ut.cpu().numpy()[ids[:, 0] - 1] * vt.cpu().numpy()[ids[:, 1] - 1], axis=1)
    assert np.allclose(o[:, 0], m, rtol=1e-12, atol=1e-13) and np.isnan(o[:, 2]).all()
    assert np.allclose(o[:, 1], np.sqrt(qt.cpu().numpy()[ids[:, 1] - 1]), rtol=1e-12)      # two equal draws: M2 = 0, stdev^2 = mean q
    pairs.close()
    y = rng.standard_normal(n)
    pairs = B.DevicePairs(ctx, ids, y)

    def update(c=ctx.handle, p=pairs.handle, D=D, u=_p(ut), v=_p(vt), q=_p(qt), a=2.0, a_dev=None, phase=1, score=0, st=_p(stats)):
        check(lib().bdf_newrows_update(c, p, D, u, v, q, 0.0, a, a_dev, phase, 1.0, -1.0, 0.0, score, st))

    for bad in (dict(c=None), dict(p=None), dict(st=None), dict(u=None), dict(v=None), dict(q=None), dict(D=0), dict(D=65), dict(phase=-1), dict(phase=3),
                dict(a=0.0), dict(a=float("nan")), dict(phase=2)):
        with pytest.raises(B.ArgumentError, match="bdf_newrows_update"):
            update(**bad)
    with pytest.raises(B.ArgumentError, match="bdf_newrows_result"):
        check(lib().bdf_newrows_result(ctx.handle, pairs.handle, _p(out)))          # no posterior draw yet
    update(phase=1, score=0)
    with pytest.raises(B.ArgumentError, match="score_lpd"):
        update(phase=2, score=1)
    update(phase=2, score=0)
    ctx.sync()
    s = stats.cpu().numpy()
    assert s[4] == n and s[5] == 0.0 and s[6] == 0.0 and s[0] > 0.0
    check(lib().bdf_newrows_result(ctx.handle, pairs.handle, _p(out)))
    ctx.sync()
    assert np.isnan(out.cpu().numpy()[:, 2]).all()
    three = B.DevicePairs(ctx, np.ones((4, 3), dtype=np.int64), np.zeros(4))
    with pytest.raises(B.ArgumentError, match="two-mode"):
        update(p=three.handle)
    three.close()
    pairs.set_pg_link(1)
    with pytest.raises(B.ArgumentError, match="no closed form"):
        update()
    pairs.close()
    empty = B.DevicePairs(ctx, np.zeros((0, 2), dtype=np.int64), np.zeros(0))
    stats.fill_(7.0)
    update(p=empty.handle)
    ctx.sync()
    assert np.array_equal(stats.cpu().numpy(), np.zeros(8))
    empty.close()


# ---- (c) macau() end to end -------------------------------------------------------------------------------------------------------
SHAPE = dict(n_train=60, n_new=20, M=30, numF=6, D=4, density=0.4, noise=0.3)
BURNIN, PSAMPLES, SEED = 5, 6, 31
CASES = {                          # kind of F_new (and of F), alpha sampled, lpd, probit, new rows = ten training rows
    "dense_fixed": ("dense", False, False, False, False),
    "csr_sampled": ("csr", True, True, False, False),
    "bin_fixed": ("bin", False, True, False, False),
    "dense_probit": ("dense", False, True, True, False),
    "train_rows": ("dense", False, False, False, True),
    "second_mode": ("dense", False, True, False, False),          # the entity with features in the relation's second column
}


def _case(name):
    kind, sampled, lpd, probit, train_rows = CASES[name]
    Ft, Fn, (ids, y), (nids, ny) = NR.planted(seed=500 + sorted(CASES).index(name), binary=kind == "bin", **SHAPE)
    if probit:
        y, ny = (y > 0).astype(np.float64), (ny > 0).astype(np.float64)
    ny = ny.copy()
    ny[3::11] = np.nan                                     # a few cells whose value is unknown
    if train_rows:
        Fn = Ft[5:15].copy()
        keep = nids[:, 0] <= 10
        nids, ny = nids[keep], ny[keep]
    return dict(kind=kind, sampled=sampled, lpd=lpd, probit=probit, Ft=Ft, Fn=Fn, ids=ids, y=y, nids=nids, ny=ny, second=name == "second_mode")


def _as_kind(B, F, kind):
    import scipy.sparse as sp
    if kind == "csr":
        return B.sparse_csr(sp.csr_matrix(F))
    if kind == "bin":
        r, c = np.nonzero(F)
        return B.SparseBinMatrix(F.shape[0], F.shape[1], r + 1, c + 1)
    return F


def _build(B, c, with_new=True):
    u, v = B.Entity("u", F=_as_kind(B, c["Ft"], c["kind"])), B.Entity("v")
    ids, nids = c["ids"], c["nids"]
    if c["second"]:
        table, ents, dims = {"v": ids[:, 1], "u": ids[:, 0], "y": c["y"]}, [v, u], [SHAPE["M"], SHAPE["n_train"]]
        new = {"v": nids[:, 1], "u": nids[:, 0], "y": c["ny"]}
    else:
        table, ents, dims = {"u": ids[:, 0], "v": ids[:, 1], "y": c["y"]}, [u, v], [SHAPE["n_train"], SHAPE["M"]]
        new = {"u": nids[:, 0], "v": nids[:, 1], "y": c["ny"]}
    rel = B.Relation(table, "planted", ents, alpha=1.0 / 0.09, dims=dims)
    rel.model.alpha_sample = c["sampled"]
    B.assignToTest(rel, np.arange(1, 41))
    if c["probit"]:
        B.setProbit(rel)
    if with_new:
        B.setNewRows(u, _as_kind(B, c["Fn"], c["kind"]))
        B.setNewTest(rel, u, new)
    return rel, u, v


CHILD = textwrap.dedent('''
    import contextlib, io, sys
    import numpy as np
    sys.path.insert(0, %r); sys.path.insert(0, %r)
    import bdf_amd as B
    from test_gpu_newrows import BURNIN, CASES, PSAMPLES, SEED, SHAPE, _build, _case
    out, d = sys.argv[1], {}
    for name in sorted(CASES):
        c = _case(name)
        rel, u, v = _build(B, c)
        rd = B.RelationData(rel)
        draws = []

        def grab(data):
            a = float(rel._dev.alpha_dev.cpu().item()) if rel.model.alpha_sample else rel.model.alpha
            draws.append((u.model.mu.copy(), u.model.Lambda.copy(), u.model.beta.copy(), v.model.sample.T.copy(), a))
            return None

        text = io.StringIO()
        with contextlib.redirect_stdout(text):
            res = B.macau(rd, num_latent=SHAPE["D"], burnin=BURNIN, psamples=PSAMPLES, verbose=True, seed=SEED, lpd=c["lpd"], f=grab)
        key = name + "_"
        nr = res["new_rows"]
        want = ["RMSE", "ROC", "accuracy", "entity", "factors", "n_rows", "n_scored", "predictions"] + (["LPD"] if c["lpd"] else [])
        assert sorted(nr) == sorted(want), sorted(nr)
        assert nr["entity"] == "u" and nr["n_rows"] == len(c["Fn"])
        d[key + "native"] = np.array(int(rd._engine.native))
        d[key + "columns"] = np.array(list(nr["predictions"].columns))
        d[key + "table"] = nr["predictions"].to_numpy(dtype=np.float64)
        d[key + "scalars"] = np.array([nr["RMSE"], nr["ROC"], nr["accuracy"], nr["n_scored"], nr.get("LPD", np.nan)], dtype=np.float64)
        d[key + "factors"] = nr["factors"]
        d[key + "mean"] = np.array(rel.model.mean_value)
        d[key + "lines"] = np.array([t for t in text.getvalue().splitlines() if "RMSE=" in t])
        for k, nm in enumerate(("mu", "Lambda", "beta", "V", "alpha")):
            d[key + nm] = np.array([dr[k] for dr in draws])
        d[key + "test"] = np.array([res["RMSE"], res["ROC"]])
        rd._engine.close()
    np.savez(out, **d)
''') % (ROOT, os.path.join(ROOT, "tests"))


@pytest.fixture(scope="module")
def runs():
    """5 + 6 iterations of macau() on every case, on the native and on the step-by-step path: one child process per path"""
    return child(CHILD, no_native=False), child(CHILD, no_native=True)


@pytest.mark.parametrize("name", sorted(CASES))
def test_macau_new_rows_match_the_restatement_on_both_paths(runs, name):
    """Both paths equal bit for bit (the draws read back through f=, the table, the scalars, the factors).  result["new_rows"]
    against the restatement driven by the per-iteration device state (mu, Lambda, beta, V, alpha) to 1e-9; a wrong stream order --
    launches that read the NEXT iteration's beta, mu or Lambda, or the previous one's -- shows here as a difference of the order of
    the draws' spread.  The verbose line's new: figures to their printed decimals."""
    c = _case(name)
    key = name + "_"
    nat, step = ({k[len(key):]: v for k, v in ch.items() if k.startswith(key)} for ch in runs)
    assert nat["native"] == 1 and step["native"] == 0 and sorted(nat) == sorted(step)
    for k in nat:
        if k not in ("native", "lines"):
            assert np.array_equal(nat[k], step[k], equal_nan=nat[k].dtype.kind == "f"), k
    assert [re.sub(r"\[[0-9.]+s\]", "", str(t)) for t in nat["lines"]] == [re.sub(r"\[[0-9.]+s\]", "", str(t)) for t in step["lines"]]
    nids, ny, probit, lpd = c["nids"], c["ny"], c["probit"], c["lpd"]
    names = ["v", "u"] if c["second"] else ["u", "v"]
    assert list(nat["columns"]) == names + ["y", "pred", "stdev"] + (["lpd"] if lpd else [])
    tab = nat["table"]
    cu, cv = names.index("u"), names.index("v")
    assert np.array_equal(tab[:, cu], nids[:, 0]) and np.array_equal(tab[:, cv], nids[:, 1]) and np.array_equal(tab[:, 2], ny, equal_nan=True)
    assert len(nat["mu"]) == PSAMPLES
    mean, st = float(nat["mean"]), NR.Stream()
    fac = np.zeros_like(nat["factors"])
    for s in range(PSAMPLES):
        mu, Lam, beta, V, alpha = (nat[k][s] for k in ("mu", "Lambda", "beta", "V", "alpha"))
        uh = NR.uhat(mu, beta, c["Fn"])
        fac += uh
        m, q = NR.cells(nids, uh, V, NR.quad(Lam, V), mean)
        p, l = NR.predict(probit, m, q), NR.loglik(probit, ny, m, q, 1.0 if probit else float(alpha))
        avg, lp = st.update(p, q, l, 1 if s == 0 else 2)
    has = ~np.isnan(ny)
    tol = dict(rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(tab[:, 3], st.mean, **tol)
    np.testing.assert_allclose(tab[:, 4], st.stdev(probit), **tol)
    np.testing.assert_allclose(nat["factors"], fac / PSAMPLES, **tol)
    cut = 0.5 if probit else 0.0                           # (setProbit moves the relation's class_cut to 0.5)
    sc = NR.scalars(ny, avg, p, lp, l, (), cut, lpd)
    rmse, roc, acc, n_scored, LPD = nat["scalars"]
    assert n_scored == has.sum() == sc[4]
    np.testing.assert_allclose(rmse, math.sqrt(sc[0] / sc[4]), **tol)
    assert acc == sc[2] / sc[4]
    from bdf_amd.driver import AUC_ROC
    np.testing.assert_allclose(roc, AUC_ROC(ny[has] < cut, -st.mean[has]), equal_nan=True, **tol)
    if lpd:
        assert np.array_equal(np.isnan(tab[:, 5]), ~has)
        np.testing.assert_allclose(tab[has, 5], lp[has], **tol)
        np.testing.assert_allclose(LPD, sc[5] / sc[4], **tol)
    if name == "train_rows":
        # the new rows ARE training rows 6 .. 15: their factors are the posterior mean of those rows' mu + beta' f (to 1e-12: the same
        # operator product on the same features)
        want = np.mean([NR.uhat(nat["mu"][s], nat["beta"][s], c["Ft"][5:15]) for s in range(PSAMPLES)], axis=0)
        assert np.all(np.abs(nat["factors"] - want) <= 1e-12 * np.maximum(1.0, np.abs(want)))
    assert len(nat["lines"]) == BURNIN + PSAMPLES
    for line in nat["lines"]:
        mt = re.search(r" new:RMSE=\s*(\d+\.\d{4}|nan) ROC=\s*(\d+\.\d{4}|nan)( LPD=-?\d+\.\d{4})? \| ", str(line))
        assert mt and bool(mt.group(3)) == lpd, line
    last = re.search(r" new:RMSE=\s*(\d+\.\d{4})", str(nat["lines"][-1]))
    assert abs(float(last.group(1)) - rmse) <= 1e-4


def test_a_run_without_the_setters_is_untouched(B, capsys):
    """the same chain with and without setNewRows / setNewTest: every result key but "new_rows", every value and every printed
    character but the new: figures bit for bit; without them no key and nothing printed"""
    c = _case("csr_sampled")

    def run(with_new):
        rel, u, v = _build(B, c, with_new)
        rd = B.RelationData(rel)
        capsys.readouterr()
        res = B.macau(rd, num_latent=SHAPE["D"], burnin=2, psamples=3, verbose=True, seed=SEED, lpd=True)
        lines = [re.sub(r"\[[0-9.]+s\]", "", t) for t in capsys.readouterr().out.splitlines()]
        S = [en.model.sample.copy() for en in rd.entities] + [u.model.beta.copy()]
        rd._engine.close()
        return res, S, lines

    plain, S0, lines0 = run(False)
    new, S1, lines1 = run(True)
    assert "new_rows" not in plain and not any("new:" in t for t in lines0)
    assert sorted(set(new) - set(plain)) == ["new_rows"] and sorted(set(plain) - set(new)) == []
    for k in plain:
        if k in ("predictions", "train_counts"):
            assert plain[k].equals(new[k]), k
        elif k != "f_output":
            assert plain[k] == new[k] or (plain[k] != plain[k] and new[k] != new[k]), k
    for a, b in zip(S0, S1):
        assert np.array_equal(a, b)
    assert [re.sub(r" new:RMSE=\s*\S+ ROC=\s*\S+ LPD=\S+", "", t) for t in lines1] == lines0
    assert sum("new:RMSE=" in t for t in lines1) == 5


# ---- (d) quality ------------------------------------------------------------------------------------------------------------------
def test_cold_start_quality_matches_the_cpu_chains(B):
    """The planted shape enlarged to 300 + 100 rows, M = 60 (newrows_restatement.QUALITY_SHAPE), alpha = 1 / 0.09 fixed, 50 + 100
    iterations.  ratio = (cold RMSE) / (RMSE of predicting mean_value) must be at most the largest of the five CPU chains' ratios x
    1.25, and the share of held-out values inside pred +- 1.645 sqrt(stdev^2 + 1 / alpha) within the CPU chains' range widened by
    0.05 on each side: the chains use different random streams and agree in law only.  The CPU figures:
    ratios 0.16551 ... 0.16569, coverage 0.9076 ... 0.9110."""
    sh = dict(NR.QUALITY_SHAPE)
    Ft, Fn, (ids, y), (nids, ny) = NR.planted(**sh)
    u, v = B.Entity("u", F=Ft), B.Entity("v")
    rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": y}, "planted", [u, v], alpha=NR.QUALITY_ALPHA, dims=[sh["n_train"], sh["M"]])
    B.setNewRows(u, Fn)
    B.setNewTest(rel, u, {"u": nids[:, 0], "v": nids[:, 1], "y": ny})
    rd = B.RelationData(rel)
    res = B.macau(rd, num_latent=sh["D"], burnin=NR.QUALITY_ITERS[0], psamples=NR.QUALITY_ITERS[1], verbose=False, seed=7)
    mean = rel.model.mean_value
    rd._engine.close()
    t = res["new_rows"]["predictions"]
    g = NR.quality(t["pred"].to_numpy(), t["stdev"].to_numpy(), ny, mean, NR.QUALITY_ALPHA)
    print(f"cold start: ratio {g['ratio']:.5f} (CPU chains {min(NR.QUALITY_CPU_RATIOS):.5f} ... {max(NR.QUALITY_CPU_RATIOS):.5f}), coverage "
          f"{g['coverage']:.4f} (CPU chains {min(NR.QUALITY_CPU_COVERAGE):.4f} ... {max(NR.QUALITY_CPU_COVERAGE):.4f}), RMSE {g['rmse']:.4f}")
    assert abs(res["new_rows"]["RMSE"] - g["rmse"]) <= 1e-9
    assert g["ratio"] <= 1.25 * max(NR.QUALITY_CPU_RATIOS), g["ratio"]
    assert min(NR.QUALITY_CPU_COVERAGE) - 0.05 <= g["coverage"] <= max(NR.QUALITY_CPU_COVERAGE) + 0.05, g["coverage"]
