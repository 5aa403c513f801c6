"""The edges of what the pair kernels share (csrc/pair_gather.h: the argument head, the lane prologue, the group test, the two
launch geometries, the reduced launch, the choice of an instantiation by the shape), through the entry points that run on it:
bdf_probit_draw, bdf_censored_draw, bdf_interval_draw, bdf_ordinal_step, bdf_pairs_lpd_update, bdf_pairs_waic_update,
bdf_robust_draw, bdf_pairs_weighted_sse, bdf_pg_draw, and bdf_predict / bdf_predict_update under the probit, the logistic and
the count link.

n in {0, 1, 7, 8, 9, 257}: an empty launch, a lone lane, one short of a group of eight lanes, exactly one group, one over, and
one pair alone in a second workgroup (a workgroup is 32 groups: 256 pairs, so nblocks = ceil(ceil(n / 8) / 32) = 0, 1, 1, 1, 1, 2).
(n_modes, D): one per instantiation <NM, VEC, NC> of BDF_BY_SHAPE -- D = 7 the scalar path <NM, 1, 1>, D = 32 one 32-byte piece
of a row per lane <NM, 4, 1>, D = 64 two pieces <NM, 4, 2> -- for two, three and four modes; <4, 4, 2> is the widest gather, the
only one launched at two waves per SIMD.  Unsorted pairs and pairs stored sorted by the last mode.  Against the restatement
modules at the bound the entry points' own tests use, 1e-9 (the links: numpy's link of the identity kernel's psi at 1e-12).  For
n = 0 the call returns BDF_OK and the outputs are untouched; the statistics of the six first entry points are then four zeros,
*wsse_out and the weighted sum exactly 0.0."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import censored_restatement as CR
import interval_restatement as IR
import lpd_restatement as LR
import ordinal_restatement as OR
import pg_restatement as PG
import probit_restatement as PR
import robust_restatement as RR
import waic_restatement as WR

pytestmark = pytest.mark.gpu

NS = (0, 1, 7, 8, 9, 257)
SHAPES = [(n_modes, D) for n_modes in (2, 3, 4) for D in (7, 32, 64)]      # one per instantiation of BDF_BY_SHAPE
COUNT_R = 5
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
    """one relation per (shape, n), shared by the tests and left unchanged: cells (some of them the same cell), factors scaled
    to udot of order 1, Gaussian and 0/1 values, censoring flags, bounds (two-sided, half-open, (-inf, inf) and exact), levels,
    weights log-uniform on 1e-3 .. 1e3 and counts (mean ~3) with b = y + COUNT_R on each side of 170 wherever n allows"""
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
    c["w"] = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), n))
    c["counts"] = rng.poisson(rng.gamma(3.0, 1.0, n)).astype(np.float64)
    c["counts"][:2] = [171.0 - COUNT_R, 169.0 - COUNT_R][:n]                # b = 171: the moment-matched normal; b = 169: the sum of 169 variates
    c["counts"][2:4] = [170.0 - COUNT_R, 0.0][:max(n - 2, 0)]
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


# ---- the robust draw, the weighted sum and the Polya-Gamma draw ---------------------------------------------------------------
@sorts
@shapes
def test_robust_draw_edges(B, ctx, n_modes, D, sort):
    """nu in {1, 4}, alpha as a scalar and through alpha_dev (the scalar then a decoy): omega against the restatement at 1e-9
    relative, no cell excluded, and sum omega e^2 against math.fsum at 1e-9 relative (test_gpu_robust.py's bounds); the output is
    eight longer than n and stays NaN beyond n; without wsse_out the same omega bits; n = 0: BDF_OK, *wsse_out == 0.0 exactly
    (k_robust_final with no partial sums), omega untouched"""
    from bdf_amd._lib import check, lib
    sweep = 30
    for n in NS:
        c, pairs, St = _setup(B, ctx, n_modes, D, n, sort, "y")
        e = (c["y"] - MEAN) - c["u"]
        for nu in (1.0, 4.0):
            for a_arg, a_dev in ((ALPHA, None), (123.0, ctx.tensor([ALPHA]))):
                sweep += 1
                om, om2, s = _nan(ctx, n + 8), _nan(ctx, n + 8), ctx.tensor([np.nan])
                ctx.set_sweep(sweep)
                check(lib().bdf_robust_draw(ctx.handle, pairs.handle, D, _facs(St), MEAN, a_arg, _p(a_dev), nu, 2, _p(om), _p(s)))
                check(lib().bdf_robust_draw(ctx.handle, pairs.handle, D, _facs(St), MEAN, a_arg, _p(a_dev), nu, 2, _p(om2), None))
                ctx.sync()
                assert _untouched(om, n) and _untouched(om2, n)
                oh, oh2, sh = om.cpu().numpy()[:n], om2.cpu().numpy()[:n], float(s.item())
                ref, _ = RR.omegas(SEED, sweep, 2, e, ALPHA, nu)
                ref_s = math.fsum(ref * e * e)
                err = np.abs(oh / ref - 1.0).max(initial=0.0)
                err_s = abs(sh - ref_s) / ref_s if n else abs(sh)
                print(f"robust modes={n_modes} D={D} sort={sort} n={n} nu={nu} dev={a_dev is not None}: omega {err:.3e}, sum {err_s:.3e}")
                assert np.all(np.isfinite(oh)) and np.all(oh > 0) and err <= TOL, (n, nu, err)
                assert abs(sh - ref_s) <= TOL * ref_s and (n > 0 or sh == 0.0), (n, nu, sh, ref_s)
                assert np.array_equal(oh, oh2)
        pairs.close()


@sorts
@shapes
def test_weighted_sse_edges(B, ctx, n_modes, D, sort):
    """weights log-uniform on 1e-3 .. 1e3 in the caller's order: sum w e^2 against math.fsum at 1e-9 relative; n = 0: exactly 0.0"""
    from bdf_amd._lib import check, lib
    for n in NS:
        c, pairs, St = _setup(B, ctx, n_modes, D, n, sort, "y")
        e = (c["y"] - MEAN) - c["u"]
        s, wt = ctx.tensor([np.nan]), _dev(ctx, c["w"])
        check(lib().bdf_pairs_weighted_sse(ctx.handle, pairs.handle, D, _facs(St), MEAN, _p(wt), _p(s)))
        ctx.sync()
        sh, ref = float(s.item()), math.fsum(c["w"] * e * e)
        print(f"weighted sse modes={n_modes} D={D} sort={sort} n={n}: {abs(sh - ref) / ref if n else abs(sh):.3e}")
        assert abs(sh - ref) <= TOL * ref and (n > 0 or sh == 0.0), (n, sh, ref)
        pairs.close()


PG_MODELS = ((1, 0), (2, COUNT_R))
PG_FIRST_SWEEP, PG_SWEEPS = 41, 40


@functools.lru_cache(maxsize=None)
def _pg_reference(n_modes, D, n, model, r):
    """(sweep, omega) of the restated draw at the first sweep number from PG_FIRST_SWEEP, of PG_SWEEPS, at which its smallest
    decision margin exceeds 1e-6 (a flipped accept / reject decision gives another omega outright); the streams are keyed by
    the caller's index, so sorted and unsorted pairs share it"""
    c = _case(n_modes, D, n)
    y = c["y01"] if model == 1 else c["counts"]
    for sweep in range(PG_FIRST_SWEEP, PG_FIRST_SWEEP + PG_SWEEPS):
        ref, mg = PG.draw_pg(c["m"], PG.b_of(model, y, r), SEED, sweep, 1 + model)
        if mg.min(initial=np.inf) > 1e-6:
            ref.setflags(write=False)
            return sweep, ref
    raise AssertionError("no sweep with every decision margin above 1e-6")


@sorts
@shapes
def test_pg_draw_edges(B, ctx, n_modes, D, sort):
    """the logit model and counts with r = 5 (b = y + r on each side of 170 wherever n allows): omega at 1e-9 relative and
    linear_out at 1e-9 relative / 1e-6 (test_gpu_pg.py's bounds), no cell excluded; the outputs are eight longer than n and stay
    NaN beyond n; n = 0: BDF_OK, the outputs untouched"""
    from bdf_amd._lib import check, lib
    for n in NS:
        for model, r in PG_MODELS:
            values = "y01" if model == 1 else "counts"
            c, pairs, St = _setup(B, ctx, n_modes, D, n, sort, values)
            y = c[values]
            if model == 2 and n >= 2:
                assert PG.b_of(model, y, r).max() > PG.SUM_MAX > PG.b_of(model, y, r)[1] > 100
            sweep, ref = _pg_reference(n_modes, D, n, model, r)
            om, lin = _nan(ctx, n + 8), _nan(ctx, n + 8)
            ctx.set_sweep(sweep)
            check(lib().bdf_pg_draw(ctx.handle, pairs.handle, D, _facs(St), MEAN, model, float(r), 1 + model, _p(om), _p(lin)))
            ctx.sync()
            assert _untouched(om, n) and _untouched(lin, n)
            oh, lh = om.cpu().numpy()[:n], lin.cpu().numpy()[:n]
            ref_l = PG.linear_of(MEAN, y, PG.kappa_of(model, y, r), ref)
            err = np.abs(oh / ref - 1.0).max(initial=0.0)
            err_l = (np.abs(lh - ref_l) / (TOL * np.abs(ref_l) + 1e-6)).max(initial=0.0)
            print(f"pg modes={n_modes} D={D} sort={sort} n={n} model={model} sweep={sweep}: omega {err:.3e}, linear at {err_l:.3e} of its tolerance")
            assert np.all(np.isfinite(oh)) and np.all(oh > 0) and np.all(np.isfinite(lh))
            assert err <= TOL and err_l <= 1.0, (n, model, sweep, err, err_l)
            pairs.close()


# ---- the links of the prediction kernels --------------------------------------------------------------------------------------
def _link(link, psi):
    return PR.phi(psi) if link == 1 else PG.link(link - 1, psi, float(COUNT_R))


@sorts
@shapes
def test_link_predict_edges(B, ctx, n_modes, D, sort):
    """links 1 (probit), 2 (logistic) and 3 (counts, r = 5): bdf_predict against numpy's link of the identity kernel's psi at 1e-12
    relative (how test_links_of_the_prediction_kernels of test_gpu_pg.py reads that bound); three updates, phases 0, 1, 2, the
    last on halved factors: the running average and sum of squares at 1e-12 relative, the statistics' two sums of squares
    against math.fsum at 1e-10 relative.  bdf_predict's output is eight longer than n and stays NaN beyond n.  n = 0: BDF_OK and
    the output untouched (include/bdf.h does not say what stats_out then holds: not asserted)"""
    from bdf_amd._lib import check, lib

    def predict(pairs, F):
        out = _nan(ctx, pairs.n + 8)
        check(lib().bdf_predict(ctx.handle, pairs.handle, D, _facs(F), MEAN, _p(out)))
        ctx.sync()
        assert _untouched(out, pairs.n)
        return out.cpu().numpy()[:pairs.n]

    for n in NS:
        c, plain, St = _setup(B, ctx, n_modes, D, n, sort, "y")
        St2 = [St[0] * 0.5] + St[1:]
        base, base2 = predict(plain, St), predict(plain, St2)
        np.testing.assert_allclose(base, c["m"], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(base2, 0.5 * c["u"] + MEAN, rtol=1e-12, atol=1e-12)
        plain.close()
        for link in (1, 2, 3):
            values = "counts" if link == 3 else "y01"
            c, pairs, St = _setup(B, ctx, n_modes, D, n, sort, values)
            if link == 1:
                pairs.set_link(1)
            else:
                pairs.set_pg_link(link - 1, float(COUNT_R))
            ref, ref2 = _link(link, base), _link(link, base2)
            got = predict(pairs, St)
            assert np.all(np.isfinite(got))
            np.testing.assert_allclose(got, ref, rtol=1e-12, atol=0)
            worst = np.abs(got / ref - 1.0).max(initial=0.0)
            for phase, F, p, avg in ((0, St, ref, ref), (1, St, ref, ref), (2, St2, ref2, (ref + ref2) / 2.0)):
                stats = ctx.tensor(np.full(4, np.nan))
                check(lib().bdf_predict_update(ctx.handle, pairs.handle, D, _facs(F), MEAN, phase, 1.0, -1.0, 0.5, _p(stats)))
                ctx.sync()
                if n == 0:
                    continue
                st = stats.cpu().numpy()
                for q, x in ((0, avg), (1, p)):
                    want = math.fsum((c[values] - x) ** 2)
                    worst = max(worst, abs(st[q] / want - 1.0))
                    assert abs(st[q] - want) <= 1e-10 * want, (n, link, phase, q, st[q], want)
            avg, sq = pairs.state()
            assert len(avg) == n and len(sq) == n
            np.testing.assert_allclose(avg, (ref + ref2) / 2.0, rtol=1e-12, atol=0)
            np.testing.assert_allclose(sq, ref * ref + ref2 * ref2, rtol=1e-12, atol=0)
            worst = max(worst, np.abs(avg / ((ref + ref2) / 2.0) - 1.0).max(initial=0.0), np.abs(sq / (ref * ref + ref2 * ref2) - 1.0).max(initial=0.0))
            print(f"links modes={n_modes} D={D} sort={sort} n={n} link={link}: {worst:.3e}")
            pairs.close()
