"""The edges of what the six pair kernels share (csrc/pair_gather.h: the argument head, the lane prologue, the group test, the two
launch geometries, the reduced launch), through the six entry points that run on it: bdf_probit_draw, bdf_censored_draw,
bdf_interval_draw, bdf_ordinal_step, bdf_pairs_lpd_update and bdf_pairs_waic_update.

n in {0, 1, 7, 8, 9, 257}: an empty launch, a lone lane, one short of a group of eight lanes, exactly one group, one over, and
one pair alone in a second workgroup (a workgroup is 32 groups: 256 pairs).  (n_modes, D) in {(2, 7), (2, 32), (3, 64), (4, 64)}:
the scalar path, two modes in one 32-byte piece per lane, two row pieces, and the widest gather, which runs at two waves.
Unsorted pairs and pairs stored sorted by the last mode.  Against the restatement modules at the bound the entry points' own
tests use, 1e-9.  For n = 0 the call returns BDF_OK, the statistics are four zeros and the outputs are untouched."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import censored_restatement as CR
import interval_restatement as IR
import lpd_restatement as LR
import ordinal_restatement as OR
import probit_restatement as PR
import waic_restatement as WR

pytestmark = pytest.mark.gpu

NS = (0, 1, 7, 8, 9, 257)
SHAPES = [(2, 7), (2, 32), (3, 64), (4, 64)]
DIMS = [37, 23, 11, 7]
SEED = 1234                        # the ctx fixture's
MEAN, ALPHA, K = 0.3, 5.0, 5
TOL = 1e-9

shapes = pytest.mark.parametrize("n_modes,D", SHAPES)
sorts = pytest.mark.parametrize("sort", [False, True])


def _bounds(rng, y):
    """(n, 2) bounds around y, standardised widths 1e-3 ... 10 (log-uniform, as test_gpu_lpd.py draws them), y anywhere inside:
    about 30 % two-sided, 15 % right-open, 10 % left-open, 5 % (-inf, +inf), the rest exact"""
    n = len(y)
    width, where, pick = 10.0 ** rng.uniform(-3.0, 1.0, n) / math.sqrt(ALPHA), rng.random(n), rng.random(n)
    lo, hi = y - where * width, y + (1.0 - where) * width
    hi[(pick >= 0.3) & (pick < 0.45)] = np.inf
    lo[(pick >= 0.45) & (pick < 0.55)] = -np.inf
    none = (pick >= 0.55) & (pick < 0.6)
    lo[none], hi[none] = -np.inf, np.inf
    lo[pick >= 0.6], hi[pick >= 0.6] = y[pick >= 0.6], y[pick >= 0.6]
    return np.ascontiguousarray(np.stack([lo, hi], axis=1))


@functools.lru_cache(maxsize=None)
def _case(n_modes, D, n):
    """one relation per (shape, n), shared by the six tests and left unchanged: cells (some of them the same cell), factors scaled
    to udot of order 1, Gaussian and 0/1 values, censoring flags, bounds (two-sided, half-open, (-inf, inf) and exact) and levels"""
    rng = np.random.default_rng(9000 + 1000 * n_modes + 10 * D + n)
    dims = DIMS[:n_modes]
    ids = np.stack([rng.integers(1, d + 1, n) for d in dims], axis=1).reshape(n, n_modes)
    ids[1::7] = ids[:1]
    S = [rng.standard_normal((d, D)) / D ** (0.5 / n_modes) for d in dims]
    y = rng.standard_normal(n)
    pick = rng.random(n)
    c = {"ids": ids, "S": S, "y": y, "y01": (rng.random(n) < 0.5).astype(np.float64), "u": PR.udot(ids, S), "m": PR.udot(ids, S) + MEAN,
         "censor": np.where(pick < 0.3, 1, np.where(pick < 0.4, -1, 0)).astype(np.int8), "bounds": _bounds(rng, y),
         "codes": rng.integers(1, K + 1, n).astype(np.int8)}
    for v in [*c.values(), *S]:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _facs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _dev(ctx, a, dtype=None):
    """a device copy; of an empty array eight rows of zeros, so that the argument is no NULL pointer"""
    import torch
    a = np.asarray(a)
    if a.shape[0] == 0:
        a = np.zeros((8,) + a.shape[1:], dtype=a.dtype)
    return ctx.tensor(a, dtype=dtype or torch.float64)


def _nan(ctx, *shape):
    return ctx.tensor(np.full((max(shape[0], 8),) + shape[1:], np.nan))


def _setup(B, ctx, n_modes, D, n, sort, values):
    c = _case(n_modes, D, n)
    pairs = B.DevicePairs(ctx, c["ids"], c[values])
    if sort:
        pairs.sort(n_modes - 1)
    return c, pairs, [ctx.tensor(s) for s in c["S"]]


def _untouched(t, n):
    return bool(np.all(np.isnan(t.cpu().numpy()[n:])))


@sorts
@shapes
def test_probit_draw_edges(B, ctx, n_modes, D, sort):
    from bdf_amd._lib import check, lib
    for n in NS:
        c, pairs, St = _setup(B, ctx, n_modes, D, n, sort, "y01")
        lin, z = _nan(ctx, n), _nan(ctx, n)
        ctx.set_sweep(11)
        check(lib().bdf_probit_draw(ctx.handle, pairs.handle, D, _facs(St), MEAN, 2, _p(lin), _p(z)))
        ctx.sync()
        assert _untouched(lin, n) and _untouched(z, n)
        zh, lh = z.cpu().numpy()[:n], lin.cpu().numpy()[:n]
        z_ref = PR.draw_z(c["m"], c["y01"], PR.uniforms(SEED, 11, 2, n))
        err = np.abs(zh - z_ref).max(initial=0.0)
        print(f"probit modes={n_modes} D={D} sort={sort} n={n}: {err:.3e}")
        assert np.all(np.isfinite(zh)) and err <= TOL, (n, err)
        assert np.array_equal(lh, c["y01"] - zh)
        pairs.close()


@sorts
@shapes
def test_censored_draw_edges(B, ctx, n_modes, D, sort):
    import torch
    from bdf_amd._lib import check, lib
    a_arg, a_dev = (123.0, ctx.tensor([ALPHA])) if sort else (ALPHA, None)      # through alpha_dev the scalar is a decoy
    for n in NS:
        c, pairs, St = _setup(B, ctx, n_modes, D, n, sort, "y")
        cd = _dev(ctx, c["censor"], torch.int8)
        lin, z = _nan(ctx, n), _nan(ctx, n)
        ctx.set_sweep(12)
        check(lib().bdf_censored_draw(ctx.handle, pairs.handle, _p(cd), D, _facs(St), MEAN, a_arg, _p(a_dev), 3, _p(lin), _p(z)))
        ctx.sync()
        assert _untouched(lin, n) and _untouched(z, n)
        zh, lh = z.cpu().numpy()[:n], lin.cpu().numpy()[:n]
        z_ref = CR.draw_z(c["m"], c["y"], c["censor"], ALPHA, CR.uniforms(SEED, 12, 3, n))
        err = np.abs(zh - z_ref).max(initial=0.0)
        print(f"censored modes={n_modes} D={D} sort={sort} n={n}: {err:.3e}")
        assert np.all(np.isfinite(zh)) and err <= TOL, (n, err)
        assert np.array_equal(lh, MEAN + (c["y"] - zh)) and np.array_equal(zh[c["censor"] == 0], c["y"][c["censor"] == 0])
        pairs.close()


@sorts
@shapes
def test_interval_draw_edges(B, ctx, n_modes, D, sort):
    from bdf_amd._lib import check, lib
    a_arg, a_dev = (123.0, ctx.tensor([ALPHA])) if sort else (ALPHA, None)
    for n in NS:
        c, pairs, St = _setup(B, ctx, n_modes, D, n, sort, "y")
        lo, hi = c["bounds"][:, 0], c["bounds"][:, 1]
        bdev = _dev(ctx, c["bounds"])
        lin, z = _nan(ctx, n), _nan(ctx, n)
        ctx.set_sweep(13)
        check(lib().bdf_interval_draw(ctx.handle, pairs.handle, _p(bdev), D, _facs(St), MEAN, a_arg, _p(a_dev), 1, _p(lin), _p(z)))
        ctx.sync()
        assert _untouched(lin, n) and _untouched(z, n)
        zh, lh = z.cpu().numpy()[:n], lin.cpu().numpy()[:n]
        z_ref = IR.draw_z(c["m"], lo, hi, ALPHA, IR.uniforms(SEED, 13, 1, n), y=c["y"])
        err = np.abs(zh - z_ref).max(initial=0.0)
        print(f"interval modes={n_modes} D={D} sort={sort} n={n}: {err:.3e}")
        assert np.all(np.isfinite(zh)) and np.all(zh >= lo) and np.all(zh <= hi) and err <= TOL, (n, err)
        assert np.array_equal(lh, MEAN + (c["y"] - zh)) and np.array_equal(zh[lo == hi], c["y"][lo == hi])
        pairs.close()


@sorts
@shapes
def test_ordinal_step_edges(B, ctx, n_modes, D, sort):
    """two steps from the edges k + 1/2: the proposal and S against the restated step (S is the fixed-order sum of the pairs' mass
    terms plus the Jacobian term: for n = 0 the Jacobian term alone), the decision wherever the restated margin |log u - S| is
    not within the bound itself, and the rows' bounds from the edges the device then holds"""
    import torch
    for n in NS:
        c, pairs, St = _setup(B, ctx, n_modes, D, n, sort, "y")
        cd = _dev(ctx, c["codes"], torch.int8)
        o = B.DeviceOrdinal(ctx, K, 0.3, 0)
        ref = OR.State(K, 0.3)
        bd = _nan(ctx, n, 2)
        for sweep in (14, 15):
            ctx.set_sweep(sweep)
            o.step(ctx, pairs, cd, D, St, MEAN, ALPHA, 2, 0, bd)
            want = ref.step(c["m"], c["codes"], ALPHA, SEED, sweep, 2, False)
            prop, got = o.proposal(), o.read()
            assert np.abs(prop["edges"] - want["prop"][1:K]).max() <= 1e-12 and want["ok"]
            err = abs(got["S"] - want["S"])
            print(f"ordinal modes={n_modes} D={D} sort={sort} n={n} sweep={sweep}: {err:.3e}")
            assert np.isfinite(got["S"]) and err <= TOL, (n, sweep, got["S"], want["S"])
            if abs(want["log_u"] - want["S"]) > 10 * TOL:
                assert prop["accepted"] == want["accepted"]
            full = np.concatenate([[-np.inf], got["edges"], [np.inf]])
            ref.e = full                                              # (the next step starts from the device's own edges)
            bh = bd.cpu().numpy()
            assert np.all(np.isnan(bh[n:]))
            if prop["accepted"]:
                assert np.array_equal(bh[:n], OR.bounds_of(c["codes"], full))
        o.close()
        pairs.close()


def _kinds(c):
    """(values, link, bounds) of the two kinds of pairs: 0/1 values under the probit link, and Gaussian values with mixed bounds"""
    return (("y01", 1, None), ("y", 0, c["bounds"]))


@sorts
@shapes
def test_lpd_update_edges(B, ctx, n_modes, D, sort):
    """phases 0, 1, 2, the last on halved factors; per pair 1e-9, the two sums 1e-9 n"""
    from bdf_amd._lib import check, lib
    for n in NS:
        for values, link, bd in _kinds(_case(n_modes, D, n)):
            c, pairs, St = _setup(B, ctx, n_modes, D, n, sort, values)
            pairs.set_link(link)
            St2 = [St[0] * 0.5] + St[1:]
            bdev = _dev(ctx, bd) if bd is not None and n else None
            stats, out = ctx.tensor(np.full(4, np.nan)), _nan(ctx, n)
            st = LR.Stream()
            for phase, F, m in ((0, St, c["m"]), (1, St, c["m"]), (2, St2, 0.5 * c["u"] + MEAN)):
                check(lib().bdf_pairs_lpd_update(ctx.handle, pairs.handle, _p(bdev), D, _facs(F), MEAN, ALPHA, None, phase, _p(stats)))
                ctx.sync()
                s = stats.cpu().numpy()
                l_ref = LR.cell_loglik(c[values], m, ALPHA, bd, probit=link == 1)
                lpd_ref = st.update(l_ref, phase)
                es = max(abs(s[0] - math.fsum(l_ref)), abs(s[1] - math.fsum(lpd_ref)))
                assert es <= TOL * n and s[2] == 0.0 and s[3] == 0.0, (n, values, phase, s)
                if phase == 0:
                    continue
                check(lib().bdf_pairs_lpd(ctx.handle, pairs.handle, _p(out)))
                ctx.sync()
                assert _untouched(out, n)
                el = np.abs(out.cpu().numpy()[:n] - lpd_ref).max(initial=0.0)
                print(f"lpd modes={n_modes} D={D} sort={sort} n={n} {values} phase={phase}: {el:.3e}, sums {es:.3e}")
                assert el <= TOL, (n, values, phase, el)
            pairs.close()


@sorts
@shapes
def test_waic_update_edges(B, ctx, n_modes, D, sort):
    """phases 0, 1, 2, the last on halved factors; per pair 1e-9 max(1, |restated value|) and for a sum the sum of the pairs'
    tolerances, as test_gpu_waic.py holds them; the count of V > 0.4 as an integer; then the end-of-run read-out"""
    from bdf_amd._lib import check, lib

    def tol(ref):
        return TOL * np.maximum(1.0, np.abs(ref))

    for n in NS:
        for values, link, bd in _kinds(_case(n_modes, D, n)):
            c, pairs, St = _setup(B, ctx, n_modes, D, n, sort, values)
            pairs.set_link(link)
            St2 = [St[0] * 0.5] + St[1:]
            bdev = _dev(ctx, bd) if bd is not None and n else None
            stats, fstats, out = ctx.tensor(np.full(4, np.nan)), ctx.tensor(np.full(4, np.nan)), _nan(ctx, n, 2)
            st = WR.Stream()
            for phase, F, m in ((0, St, c["m"]), (1, St, c["m"]), (2, St2, 0.5 * c["u"] + MEAN)):
                check(lib().bdf_pairs_waic_update(ctx.handle, pairs.handle, _p(bdev), D, _facs(F), MEAN, ALPHA, None, phase, _p(stats)))
                ctx.sync()
                s = stats.cpu().numpy()
                l_ref = LR.cell_loglik(c[values], m, ALPHA, bd, probit=link == 1)
                lppd_ref, V_ref = st.update(l_ref, phase)
                assert abs(s[0] - math.fsum(l_ref)) <= tol(l_ref).sum() and abs(s[1] - math.fsum(lppd_ref)) <= tol(lppd_ref).sum(), (n, values, phase, s)
                assert abs(s[2] - math.fsum(V_ref)) <= tol(V_ref).sum() and s[3] == float(np.count_nonzero(V_ref > WR.HIGH)), (n, values, phase, s)
                if phase == 0:
                    continue
                check(lib().bdf_pairs_waic(ctx.handle, pairs.handle, _p(out), _p(fstats)))
                ctx.sync()
                got, f = out.cpu().numpy(), fstats.cpu().numpy()
                assert np.all(np.isnan(got[n:]))
                el = (np.abs(got[:n, 0] - lppd_ref) / tol(lppd_ref)).max(initial=0.0)
                ev = (np.abs(got[:n, 1] - V_ref) / tol(V_ref)).max(initial=0.0)
                print(f"waic modes={n_modes} D={D} sort={sort} n={n} {values} phase={phase}: lppd {el * TOL:.3e}, V {ev * TOL:.3e}")
                assert el <= 1.0 and ev <= 1.0, (n, values, phase, el, ev)
                assert abs(f[0] - math.fsum(lppd_ref)) <= tol(lppd_ref).sum() and abs(f[1] - math.fsum(V_ref)) <= tol(V_ref).sum()
                assert f[3] == float(np.count_nonzero(V_ref > WR.HIGH)) and np.isfinite(f[2]) and (n > 0 or f[2] == 0.0)
            pairs.close()
