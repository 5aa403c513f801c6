"""Convergence diagnostics of held-out predictions (setDiagnostics; csrc/k_diag.hip) on the device.

Push: a pushed row, mapped to the caller's order, is bdf_predict's output on the same pairs and factors bit for bit; the row's first
scalar is the float64 sum of (value - p)^2 within 1e-13 of the sum of the terms; the second is alpha.  n in {1, 7, 8, 9, 257} (a
group is 8 pairs, a workgroup 256), two and three modes, D in {5, 8, 32, 36} (the scalar-lane, one-piece and two-piece gathers),
unsorted and sorted pairs, with a baseline, with the probit link.

Compute: known series through bdf_diag_write -- iid, AR(0.9), AR(-0.5), constant, two halves at different levels, a trend, iid at
an offset of 1e3 -- for cells in {1, 63, 64, 65, 129} (a workgroup's tile is 64 series), 0 and 2 scalars, draws in {4, 5, 8, 9,
64, 65, 200, 320, 321} (320 is the last count whose tile the kernel keeps in LDS, 321 the first it reads from the plane), against
tests/diag_restatement.py at 1e-9 relative.  The stop of Geyer's sequence and its monotone minimum are discrete: before it
compares, the test asserts on the host that no deciding P_k of any series lies within 1e-9 of zero or of its predecessor.  The
summary is compared exactly -- the counts with those of the restated columns (no restated figure lies within 1e-9 of a cut), the
maximum and the minimum with those of the columns the device returned, which they are in any order of reduction -- and at 1e-9
with the restated maximum and minimum.

Whole run: 30 x 20 cells, D = 4, burnin 5, psamples 8 and 9, plain Gaussian and with a sampled alpha and biases, on both iteration
paths (tests/both_paths.py)."""
import ctypes as C
import functools
import gc
import math
import os
import textwrap

import numpy as np
import pytest

import diag_restatement as DR
from both_paths import child

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9
DIMS = [37, 23, 11]
MEAN, ALPHA = 0.3, 5.0
LDS_DRAWS = 320                    # BDF_DIAG_LDS_DRAWS of csrc/k_diag.hip
KINDS = ("iid", "ar+", "ar-", "constant", "levels", "trend", "offset")


def _diag(*args):
    from bdf_amd.engine import DeviceDiag
    return DeviceDiag(*args)


# ---- push ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(n_modes, D, n):
    rng = np.random.default_rng(4000 + 1000 * n_modes + 10 * D + n)
    dims = DIMS[:n_modes]
    ids = np.stack([rng.integers(1, d + 1, n) for d in dims], axis=1).reshape(n, n_modes)
    S = [rng.standard_normal((d, D)) / D ** (0.5 / n_modes) for d in dims]
    c = {"ids": ids, "S": S, "y": rng.standard_normal(n), "y01": (rng.random(n) < 0.5).astype(np.float64), "base": rng.standard_normal(n)}
    for v in [*c.values(), *S]:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@pytest.mark.parametrize("variant", ["plain", "baseline", "probit"])
@pytest.mark.parametrize("sort", [False, True])
@pytest.mark.parametrize("D", [5, 8, 32, 36])
@pytest.mark.parametrize("n_modes", [2, 3])
def test_a_pushed_row_is_the_prediction_bit_for_bit(B, ctx, n_modes, D, sort, variant):
    from bdf_amd._lib import check, lib
    for n in (1, 7, 8, 9, 257):
        c = _case(n_modes, D, n)
        pairs = B.DevicePairs(ctx, c["ids"], c["y01" if variant == "probit" else "y"])
        if sort:
            pairs.sort(n_modes - 1)
        base = None
        if variant == "baseline":
            base = ctx.tensor(c["base"])
            check(lib().bdf_pairs_set_baseline(pairs.handle, C.c_void_p(base.data_ptr())))
        if variant == "probit":
            pairs.set_link(1)
        facs = [ctx.tensor(s) for s in c["S"]]
        diag = _diag(ctx, n, 2, 2)
        diag.push(pairs, D, facs, MEAN, ALPHA)
        diag.push(pairs, D, facs, MEAN, ctx.tensor(np.array([ALPHA * 2])))           # (alpha on the device wins)
        want = pairs.predict(D, facs, MEAN)
        ctx.sync()
        want, plane = want.cpu().numpy(), diag.plane()
        assert plane.shape == (2, n + 2)
        order = pairs._order if pairs._order is not None else np.arange(n)
        got = np.empty(n)
        got[order] = plane[0, :n]
        assert got.tobytes() == want.tobytes(), (n, np.max(np.abs(got - want)))
        assert plane[1, :n].tobytes() == plane[0, :n].tobytes()
        terms = (c["y01" if variant == "probit" else "y"] - want) ** 2
        assert abs(plane[0, n] - math.fsum(terms)) <= 1e-13 * math.fsum(np.abs(terms)), (n, plane[0, n], math.fsum(terms))
        assert plane[1, n] == plane[0, n] and plane[0, n + 1] == ALPHA and plane[1, n + 1] == ALPHA * 2
        with pytest.raises(B.ArgumentError, match="the plane is full"):
            diag.push(pairs, D, facs, MEAN, ALPHA)
        diag.close()
        pairs.close()


def test_push_refuses_pairs_of_another_size(B, ctx):
    c = _case(2, 8, 9)
    pairs = B.DevicePairs(ctx, c["ids"], c["y"])
    diag = _diag(ctx, 8, 1, 4)
    with pytest.raises(B.ArgumentError, match="the pairs hold 9 cells, the plane's rows 8"):
        diag.push(pairs, 8, [ctx.tensor(s) for s in c["S"]], MEAN)
    with pytest.raises(B.ArgumentError, match="a split chain needs at least 4"):
        diag.compute(1.1, 100.0)
    diag.close()
    pairs.close()


# ---- compute ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _series(draws, total):
    """(draws, total) doubles, column c of kind KINDS[c % 7]; left unchanged"""
    rng = np.random.default_rng(100 * draws + total)
    x = np.empty((draws, total))
    for c in range(total):
        kind = KINDS[c % len(KINDS)]
        if kind == "iid":
            x[:, c] = rng.standard_normal(draws)
        elif kind == "ar+":
            x[:, c] = DR.ar1(rng, draws, 0.9)[:, 0]
        elif kind == "ar-":
            x[:, c] = DR.ar1(rng, draws, -0.5)[:, 0]
        elif kind == "constant":
            x[:, c] = 2.5
        elif kind == "levels":
            x[:, c] = rng.standard_normal(draws) + np.where(np.arange(draws) < draws // 2, 0.0, 5.0)
        elif kind == "trend":
            x[:, c] = rng.standard_normal(draws) + np.linspace(0.0, 3.0, draws)
        else:
            x[:, c] = 1e3 + rng.standard_normal(draws)
    x.setflags(write=False)
    return x


def _rel(got, want):
    both = np.isnan(got) & np.isnan(want)
    with np.errstate(invalid="ignore"):
        return np.where(both, 0.0, np.abs(got - want) / np.abs(want))


@pytest.mark.parametrize("n_scalars", [0, 2])
@pytest.mark.parametrize("cells", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("draws", [4, 5, 8, 9, 64, 65, 200, LDS_DRAWS, LDS_DRAWS + 1])
def test_compute_against_the_restatement(B, ctx, draws, cells, n_scalars):
    total = cells + n_scalars
    x = _series(draws, total)
    rhat_cut, ess_cut = 1.1, draws / 2.0
    assert DR.decisions_clear(x, TOL)                       # no series is on the edge of a discrete decision: none is left out
    rhat, ess, mcse = DR.diagnostics(x)
    assert not (np.abs(rhat[:cells] / rhat_cut - 1.0) < TOL).any() and not (np.abs(ess[:cells] / ess_cut - 1.0) < TOL).any()
    perm = np.random.default_rng(draws + cells).permutation(cells)                 # storage position -> the caller's index
    diag = _diag(ctx, cells, n_scalars, draws + 1)
    rows = ctx.tensor(x)
    for i in range(draws):
        diag.write(i, rows[i])
    stats, out = diag.compute(rhat_cut, ess_cut, pointwise=True, order=perm)
    ctx.sync()
    stats, out = stats.cpu().numpy(), out.cpu().numpy()
    plane = diag.plane()
    diag.close()
    assert plane.tobytes() == x.tobytes()
    cols = np.empty((cells, 3))
    cols[perm] = np.stack([rhat, ess, mcse], axis=1)[:cells]
    assert np.array_equal(np.isnan(out), np.isnan(cols))
    worst = float(_rel(out, cols).max())
    print(f"draws={draws} cells={cells} scalars={n_scalars}: worst relative deviation of (rhat, ess, mcse) {worst:.2e}")
    assert worst <= TOL
    for k in range(n_scalars):
        got, want = stats[6 + 3 * k:9 + 3 * k], np.array([rhat[cells + k], ess[cells + k], mcse[cells + k]])
        assert np.array_equal(np.isnan(got), np.isnan(want)) and _rel(got, want).max() <= TOL
    # the summary: the cells alone; a cell without figures is counted as constant and is in no other figure
    want, own = DR.summary(rhat[:cells], ess[:cells], rhat_cut, ess_cut), DR.summary(out[:, 0], out[:, 1], rhat_cut, ess_cut)
    got = dict(zip(("max_rhat", "min_ess", "n_rhat_high", "n_ess_low", "n_constant", "n_draws"), stats[:6]))
    assert got["n_draws"] == draws
    for k in ("n_rhat_high", "n_ess_low", "n_constant"):
        assert got[k] == want[k] == own[k], k
    assert want["n_constant"] == sum(1 for c in range(cells) if KINDS[c % 7] == "constant")
    for k in ("max_rhat", "min_ess"):
        if np.isnan(want[k]):
            assert np.isnan(got[k]) and np.isnan(own[k])
        else:
            assert got[k] == own[k] and abs(got[k] - want[k]) <= TOL * abs(want[k]), k


def test_compute_without_columns_gives_the_same_summary(B, ctx):
    x = _series(65, 131)
    res = []
    for pointwise in (False, True):
        diag = _diag(ctx, 129, 2, 65)
        rows = ctx.tensor(x)
        for i in range(65):
            diag.write(i, rows[i])
        stats, out = diag.compute(1.1, 32.5, pointwise=pointwise)
        ctx.sync()
        assert (out is None) == (not pointwise)
        res.append(stats.cpu().numpy())
        diag.close()
    assert res[0].tobytes() == res[1].tobytes()


# ---- lifetime -----------------------------------------------------------------------------------------------------------------------
def test_a_closed_handle_gives_back_what_it_took(B):
    from bdf_amd._lib import check, lib

    def live():
        blocks, nbytes = C.c_int64(-1), C.c_int64(-1)
        check(lib().bdf_dev_live(C.byref(blocks), C.byref(nbytes)))
        return blocks.value, nbytes.value

    gc.collect()
    base = live()
    own = B.Context(seed=5)
    c = _case(2, 8, 257)
    pairs = B.DevicePairs(own, c["ids"], c["y"])
    held = live()
    diag = _diag(own, 257, 2, 6)
    assert live() == (held[0] + 2, held[1] + 6 * 259 * 8 + 4 * 8)         # the plane and the push's four statistics
    facs = [own.tensor(s) for s in c["S"]]
    for _ in range(6):
        diag.push(pairs, 8, facs, MEAN, ALPHA)
    stats, _ = diag.compute(1.1, 3.0, pointwise=True)
    own.sync()
    assert stats.cpu().numpy()[5] == 6
    scratch = live()
    diag.close()
    assert live() == (scratch[0] - 2, scratch[1] - 6 * 259 * 8 - 4 * 8)
    pairs.close()
    own.close()
    gc.collect()
    assert live() == base


# ---- the whole run ------------------------------------------------------------------------------------------------------------------
PSAMPLES = (8, 9)
CHILD = textwrap.dedent('''
    import sys
    import numpy as np
    sys.path.insert(0, %r); sys.path.insert(0, %r)
    import bdf_amd as B
    from bdf_amd import engine as E
    out, d = sys.argv[1], {}
    rng = np.random.default_rng(0)
    U, V = rng.standard_normal((30, 2)), rng.standard_normal((20, 2))
    i, j = np.nonzero(rng.random((30, 20)) < 0.6)
    y = np.sum(U[i] * V[j], axis=1) + 0.3 * rng.standard_normal(len(i))
    planes = []
    close = E.DeviceDiag.close

    def keep(self):                                          # the pushed draws, read out before the run's summary closes its handle
        if self.handle:
            planes.append(self.plane())
        close(self)
    E.DeviceDiag.close = keep

    for model in ("plain", "alpha_bias"):
        for psamples in %r:
            rel = B.Relation({"u": i + 1, "v": j + 1, "y": y}, "plays", [B.Entity("u"), B.Entity("v")], alpha=2.0, dims=[30, 20])
            B.assignToTest(rel, np.arange(1, 61))
            if model == "alpha_bias":
                rel.model.alpha_sample = True
                B.setBias(rel, rel.entities[0])
            B.setDiagnostics(rel, pointwise=True, rhat_cut=1.05, ess_cut=6.0)
            rd = B.RelationData(rel)
            res = B.macau(rd, num_latent=4, burnin=5, psamples=psamples, verbose=False, seed=11)
            key = "%%s_%%d_" %% (model, psamples)
            g = res["diagnostics"]
            d[key + "native"] = np.array(int(rd._engine.native))
            d[key + "keys"] = np.array(list(g))
            d[key + "scalar_names"] = np.array(list(g["scalars"]))
            for k, v in g.items():
                if k != "scalars":
                    d[key + "diag_" + k] = np.array(v)
            for name, s in g["scalars"].items():
                d[key + "scalar_" + name] = np.array([s["rhat"], s["ess"], s["mcse"]])
            d[key + "columns"] = np.array(list(res["predictions"].columns))
            for k in ("pred", "rhat", "ess", "mcse"):
                d[key + "col_" + k] = res["predictions"][k].to_numpy()
            d[key + "order"] = rd._engine.test_pairs()._order
            d[key + "values"] = rel.test_vec.values
            d[key + "plane"] = planes.pop()
            assert not planes
            rd._engine.close()
    np.savez(out, **d)
''') % (ROOT, os.path.join(ROOT, "tests"), PSAMPLES)


@pytest.fixture(scope="module")
def runs():
    return child(CHILD, no_native=False), child(CHILD, no_native=True)


def _of(path, key):
    return {k[len(key):]: v for k, v in path.items() if k.startswith(key)}


@pytest.mark.parametrize("psamples", PSAMPLES)
@pytest.mark.parametrize("model", ["plain", "alpha_bias"])
def test_macau_on_both_paths(runs, model, psamples):
    nat, step = (_of(p, "%s_%d_" % (model, psamples)) for p in runs)
    assert nat["native"] == 1 and step["native"] == 0
    assert nat["keys"].tolist() == ["n_draws", "max_rhat", "min_ess", "n_rhat_high", "n_ess_low", "n_constant", "rhat_cut", "ess_cut", "scalars"]
    assert nat["scalar_names"].tolist() == (["sse", "alpha"] if model == "alpha_bias" else ["sse"])      # alpha is traced only when sampled
    assert nat["columns"].tolist()[-5:] == ["pred", "stdev", "rhat", "ess", "mcse"]
    for k in nat:
        if k.startswith(("diag_", "scalar_", "col_")) or k in ("keys", "scalar_names", "columns"):
            assert nat[k].tobytes() == step[k].tobytes(), k                   # the two paths: equal bits
    assert nat["diag_n_draws"] == psamples and nat["diag_rhat_cut"] == 1.05 and nat["diag_ess_cut"] == 6.0


@pytest.mark.parametrize("psamples", PSAMPLES)
@pytest.mark.parametrize("model", ["plain", "alpha_bias"])
def test_macau_result_is_the_restatement_of_the_plane(runs, model, psamples):
    for path in runs:
        r = _of(path, "%s_%d_" % (model, psamples))
        plane, order, n = r["plane"], r["order"], 60
        assert plane.shape == (psamples, n + (2 if model == "alpha_bias" else 1))
        assert DR.decisions_clear(plane, TOL)
        rhat, ess, mcse = DR.diagnostics(plane)
        for k, v in (("rhat", rhat), ("ess", ess), ("mcse", mcse)):
            want = np.empty(n)
            want[order] = v[:n]
            assert _rel(r["col_" + k], want).max() <= TOL, k
        names = ["sse", "alpha"][:plane.shape[1] - n]
        for q, name in enumerate(names):
            assert _rel(r["scalar_" + name], np.array([rhat[n + q], ess[n + q], mcse[n + q]])).max() <= TOL, name
        want = DR.summary(rhat[:n], ess[:n], 1.05, 6.0)
        assert abs(r["diag_max_rhat"] - want["max_rhat"]) <= TOL * want["max_rhat"] and abs(r["diag_min_ess"] - want["min_ess"]) <= TOL * want["min_ess"]
        assert r["diag_max_rhat"] == r["col_rhat"].max() and r["diag_min_ess"] == r["col_ess"].min()
        assert not (np.abs(rhat[:n] / 1.05 - 1.0) < TOL).any() and not (np.abs(ess[:n] / 6.0 - 1.0) < TOL).any()
        assert (r["diag_n_rhat_high"], r["diag_n_ess_low"], r["diag_n_constant"]) == (want["n_rhat_high"], want["n_ess_low"], 0)
        # the plane's mean over the draws is the unclamped posterior mean prediction: 1e-12 of the cell's largest draw (a mean that
        # cancels cannot be held relative to itself)
        mean = np.empty(n)
        mean[order] = plane[:, :n].mean(axis=0)
        scale = np.empty(n)
        scale[order] = np.abs(plane[:, :n]).max(axis=0)
        assert (np.abs(mean - r["col_pred"]) <= 1e-12 * scale).all()
        # the first scalar is the draw's sum of squared test errors
        sse = ((r["values"][order][None, :] - plane[:, :n]) ** 2).sum(axis=1)
        assert np.abs(plane[:, n] - sse).max() <= 1e-13 * sse.max()
        if model == "alpha_bias":
            assert (plane[:, n + 1] > 0).all() and len(set(plane[:, n + 1])) == psamples


def _plain(B):
    rng = np.random.default_rng(0)
    i, j = np.nonzero(rng.random((30, 20)) < 0.6)
    rel = B.Relation({"u": i + 1, "v": j + 1, "y": rng.standard_normal(len(i))}, "plays", [B.Entity("u"), B.Entity("v")], alpha=2.0, dims=[30, 20])
    B.assignToTest(rel, np.arange(1, 61))
    return rel


def test_macau_without_pointwise_and_a_second_run_on_the_same_engine(B, capsys):
    rel = _plain(B)
    rd = B.RelationData(rel)
    plain = B.macau(rd, num_latent=4, burnin=5, psamples=8, verbose=False, seed=11)
    rd._engine.close()
    assert "diagnostics" not in plain
    B.setDiagnostics(rel)
    rd = B.RelationData(rel)
    res = B.macau(rd, num_latent=4, burnin=5, psamples=8, verbose=False, seed=11)
    assert list(res["predictions"].columns) == list(plain["predictions"].columns)             # pointwise = false: no columns
    assert res["predictions"]["pred"].to_numpy().tobytes() == plain["predictions"]["pred"].to_numpy().tobytes()     # the chain is untouched
    assert res["diagnostics"]["n_draws"] == 8 and list(res["diagnostics"]["scalars"]) == ["sse"]
    assert capsys.readouterr().out == ""
    # the same engine again, the chain going on: a fresh plane of this call's draws
    again = B.macau(rd, num_latent=4, burnin=0, psamples=5, verbose=True, seed=11, engine=rd._engine, reset_model=False)
    assert again["diagnostics"]["n_draws"] == 5 and again["diagnostics"]["max_rhat"] != res["diagnostics"]["max_rhat"]
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Diagnostics:")]
    assert len(lines) == 1 and "max R̂=" in lines[0] and "min ESS=" in lines[0] and "of 60 cells above 1.1" in lines[0]
    rd._engine.close()
