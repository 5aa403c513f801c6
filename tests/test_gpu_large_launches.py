"""Launches past one pass of what the small shapes never leave: more than 256 workgroups' partial sums under the fixed-order
final sums (`for (b = tid; b < nblocks; b += 256)` in k_predict_final, k_robust_final and k_ordinal_accept), and the second trip of
the grid-stride kernels, whose grid is capped at 8192 workgroups.  Two modes, D = 8, dims (37, 23) unless said otherwise.

(a) N_FINAL = 256 * 256 + 1 = 65,537 pairs: a workgroup takes 256 pairs, so nblocks = ceil(ceil(n / 8) / 32) = 257 -- lane 0 of the
    final sum adds partial 0 and partial 256.
(b) N_RUNS = 512 * 256 + 1 = 131,073 pairs sorted by mode 1, D = 32: k_update_runs and k_predict_runs take 512 pairs per workgroup,
    nblocks = ceil(n / 512) = 257 (and the general kernel on the unsorted pairs 513).
(c) N_STRIDE = 8192 * 256 + 9 = 2,097,161 pairs: ceil(n / 8) = 262,146 groups of eight pairs for 8192 * 32 = 262,144 groups of eight
    lanes -- groups 0 and 1 of workgroup 0 take a second trip, one with eight pairs and one with a lone lane, while every other
    group leaves the loop after its first.

The sums are held against math.fsum of the restatements' per-pair terms, the per-pair outputs at the entry points' usual
bounds.  In (b) the order of every addition is specified, so equality is the test (tests/test_gpu_predict_fit.py)."""
import ctypes as C
import functools
import math
import time

import numpy as np
import pytest

import censored_restatement as CR
import lpd_restatement as LR
import ordinal_restatement as OR
import pg_restatement as PG
import probit_restatement as PR
import robust_restatement as RR
import waic_restatement as WR
from test_gpu_pair_edges import _bounds, _dev, _facs, _nan, _p, _untouched
from test_gpu_predict_fit import CLAMP, CUT, MEAN as FIT_MEAN, _check, _dots, _Model, _stats

pytestmark = pytest.mark.gpu

N_FINAL = 256 * 256 + 1
N_RUNS = 512 * 256 + 1
N_STRIDE = 8192 * 256 + 9
D, DIMS = 8, (37, 23)
SEED = 1234                        # the ctx fixture's
MEAN, ALPHA, K, COUNT_R = 0.3, 5.0, 5, 5
TOL = 1e-9


@functools.lru_cache(maxsize=None)
def _case(n):
    """one relation per n, shared by the tests and left unchanged.  The rows of mode 0 carry one sign each and the rows of mode 1
    are positive: the D products of a pair share their sign, so udot is good to a few ulp in any order of summation, and the
    seed is one for which no cell's psi = udot + MEAN, 0.5 udot + MEAN or 0.75 udot + MEAN (the halved factors of the second
    update and the running average) is below a hundredth of |udot| + MEAN -- asserted below: a relative bound of 1e-12 on psi is
    then a bound on the kernel, not on the cancellation.  |udot| is of order 1."""
    rng = np.random.default_rng(77)
    sign = np.where(rng.random(DIMS[0]) < 0.5, -1.0, 1.0)
    S = [sign[:, None] * rng.uniform(0.1, 0.5, (DIMS[0], D)), rng.uniform(0.3, 0.9, (DIMS[1], D))]
    ids = np.stack([rng.integers(1, d + 1, n) for d in DIMS], axis=1)
    u = PR.udot(ids, S)
    for f in (1.0, 0.5, 0.75):
        assert np.all(np.abs(f * u + MEAN) >= 0.01 * (np.abs(f * u) + MEAN))
    y = u + MEAN + rng.standard_normal(n)
    pick = rng.random(n)
    c = {"ids": ids, "S": S, "u": u, "m": u + MEAN, "y": y, "y01": (rng.random(n) < 0.5).astype(np.float64),
         "counts": rng.poisson(rng.gamma(3.0, 1.0, n)).astype(np.float64),
         "censor": np.where(pick < 0.3, 1, np.where(pick < 0.4, -1, 0)).astype(np.int8),
         "w": np.exp(rng.uniform(np.log(1e-3), np.log(1e3), n))}
    if n <= N_FINAL:
        c["bounds"], c["codes"] = _bounds(rng, y), rng.integers(1, K + 1, n).astype(np.int8)
        c["codes"][-1] = 3             # (a middle level: both of its edges move, so the last pair's mass term is not 0)
    for v in [*c.values(), *S]:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def _setup(B, ctx, n, values):
    c = _case(n)
    return c, B.DevicePairs(ctx, c["ids"], c[values]), [ctx.tensor(s) for s in c["S"]]


def _fsum(a):
    return math.fsum(np.asarray(a, dtype=np.float64).tolist())


# ---- (a) 257 partial sums ---------------------------------------------------------------------------------------------------------
def test_robust_sums_over_257_workgroups(B, ctx):
    """bdf_robust_draw: omega at 1e-9 relative, sum omega e^2 against math.fsum at 1e-9 relative (k_robust_final over 257 partial
    sums); bdf_pairs_weighted_sse on weights log-uniform on 1e-3 .. 1e3 the same"""
    from bdf_amd._lib import check, lib
    n = N_FINAL
    c, pairs, St = _setup(B, ctx, n, "y")
    e = (c["y"] - MEAN) - c["u"]
    om, s, s2, wt = _nan(ctx, n + 8), ctx.tensor([np.nan]), ctx.tensor([np.nan]), ctx.tensor(c["w"])
    ctx.set_sweep(31)
    check(lib().bdf_robust_draw(ctx.handle, pairs.handle, D, _facs(St), MEAN, ALPHA, None, 4.0, 2, _p(om), _p(s)))
    check(lib().bdf_pairs_weighted_sse(ctx.handle, pairs.handle, D, _facs(St), MEAN, _p(wt), _p(s2)))
    ctx.sync()
    assert _untouched(om, n)
    oh, sh, sh2 = om.cpu().numpy()[:n], float(s.item()), float(s2.item())
    ref, _ = RR.omegas(SEED, 31, 2, e, ALPHA, 4.0)
    ref_s, ref_s2 = _fsum(ref * e * e), _fsum(c["w"] * e * e)
    err = np.abs(oh / ref - 1.0).max()
    print(f"257 workgroups, robust: omega {err:.3e}, sum omega e^2 {abs(sh / ref_s - 1.0):.3e}, sum w e^2 {abs(sh2 / ref_s2 - 1.0):.3e}")
    assert err <= TOL
    assert abs(sh - ref_s) <= TOL * ref_s, (sh, ref_s)
    assert abs(sh2 - ref_s2) <= TOL * ref_s2, (sh2, ref_s2)
    # the sum of the device's own omega: the final sum alone, without the draw's error
    own = _fsum(oh * e * e)
    assert abs(sh - own) <= 1e-12 * own, (sh, own)
    pairs.close()


def _kinds(c):
    """(values, link, bounds) as tests/test_gpu_pair_edges.py: 0/1 values under the probit link, Gaussian values with mixed bounds"""
    return (("y01", 1, None), ("y", 0, c["bounds"]))


def test_lpd_sums_over_257_workgroups(B, ctx):
    """bdf_pairs_lpd_update phases 1 and 2 (the second on halved factors): per pair 1e-9, the two sums 1e-9 n"""
    from bdf_amd._lib import check, lib
    n = N_FINAL
    for values, link, bd in _kinds(_case(n)):
        c, pairs, St = _setup(B, ctx, n, values)
        pairs.set_link(link)
        St2 = [St[0] * 0.5] + St[1:]
        bdev = _dev(ctx, bd) if bd is not None else None
        stats, out = ctx.tensor(np.full(4, np.nan)), _nan(ctx, n + 8)
        st = LR.Stream()
        for phase, F, m in ((1, St, c["m"]), (2, St2, 0.5 * c["u"] + MEAN)):
            check(lib().bdf_pairs_lpd_update(ctx.handle, pairs.handle, _p(bdev), D, _facs(F), MEAN, ALPHA, None, phase, _p(stats)))
            check(lib().bdf_pairs_lpd(ctx.handle, pairs.handle, _p(out)))
            ctx.sync()
            s = stats.cpu().numpy()
            l_ref = LR.cell_loglik(c[values], m, ALPHA, bd, probit=link == 1)
            lpd_ref = st.update(l_ref, phase)
            es = max(abs(s[0] - _fsum(l_ref)), abs(s[1] - _fsum(lpd_ref)))
            el = np.abs(out.cpu().numpy()[:n] - lpd_ref).max()
            print(f"257 workgroups, lpd {values} phase={phase}: per pair {el:.3e}, sums {es:.3e} (of {abs(_fsum(l_ref)):.1f})")
            assert es <= TOL * n and s[2] == 0.0 and s[3] == 0.0, (values, phase, s)
            assert _untouched(out, n) and el <= TOL, (values, phase, el)
        pairs.close()


def test_waic_sums_over_257_workgroups(B, ctx):
    """bdf_pairs_waic_update phases 1 and 2: per pair 1e-9 max(1, |restated value|), a sum at the sum of the pairs' tolerances
    (test_gpu_waic.py), the count of V > 0.4 as an integer"""
    from bdf_amd._lib import check, lib

    def tol(ref):
        return TOL * np.maximum(1.0, np.abs(ref))

    n = N_FINAL
    for values, link, bd in _kinds(_case(n)):
        c, pairs, St = _setup(B, ctx, n, values)
        pairs.set_link(link)
        St2 = [St[0] * 0.5] + St[1:]
        bdev = _dev(ctx, bd) if bd is not None else None
        stats, fstats, out = ctx.tensor(np.full(4, np.nan)), ctx.tensor(np.full(4, np.nan)), _nan(ctx, n + 8, 2)
        st = WR.Stream()
        for phase, F, m in ((1, St, c["m"]), (2, St2, 0.5 * c["u"] + MEAN)):
            check(lib().bdf_pairs_waic_update(ctx.handle, pairs.handle, _p(bdev), D, _facs(F), MEAN, ALPHA, None, phase, _p(stats)))
            check(lib().bdf_pairs_waic(ctx.handle, pairs.handle, _p(out), _p(fstats)))
            ctx.sync()
            s, f, got = stats.cpu().numpy(), fstats.cpu().numpy(), out.cpu().numpy()
            l_ref = LR.cell_loglik(c[values], m, ALPHA, bd, probit=link == 1)
            lppd_ref, V_ref = st.update(l_ref, phase)
            high = float(np.count_nonzero(V_ref > WR.HIGH))
            el = (np.abs(got[:n, 0] - lppd_ref) / tol(lppd_ref)).max()
            ev = (np.abs(got[:n, 1] - V_ref) / tol(V_ref)).max()
            es = [abs(s[0] - _fsum(l_ref)) / tol(l_ref).sum(), abs(s[1] - _fsum(lppd_ref)) / tol(lppd_ref).sum(),
                  abs(s[2] - _fsum(V_ref)) / tol(V_ref).sum(), abs(f[0] - _fsum(lppd_ref)) / tol(lppd_ref).sum(),
                  abs(f[1] - _fsum(V_ref)) / tol(V_ref).sum()]
            print(f"257 workgroups, waic {values} phase={phase}: lppd {el * TOL:.3e}, V {ev * TOL:.3e}, sums at {max(es):.3e} of their tolerance")
            assert np.all(np.isnan(got[n:])) and el <= 1.0 and ev <= 1.0, (values, phase, el, ev)
            assert max(es) <= 1.0 and s[3] == high and f[3] == high and np.isfinite(f[2]), (values, phase, es, s, f)
        pairs.close()


def test_ordinal_accept_sums_over_257_workgroups(B, ctx):
    """bdf_ordinal_step, two steps: S (k_ordinal_accept's own fixed-order sum of 257 partial sums plus the Jacobian term) against
    the restated step at 1e-9 n, the decision wherever the restated margin |log u - S| is not within ten times that.  A cell of
    the lowest or the highest level has a mass term of exactly 0: the pair that is alone in the last workgroup is of level 3"""
    import torch
    n = N_FINAL
    c, pairs, St = _setup(B, ctx, n, "y")
    cd = ctx.tensor(c["codes"], dtype=torch.int8)
    o = B.DeviceOrdinal(ctx, K, 0.3, 0)
    ref = OR.State(K, 0.3)
    bd = _nan(ctx, n + 8, 2)
    for sweep in (14, 15):
        ctx.set_sweep(sweep)
        o.step(ctx, pairs, cd, D, St, MEAN, ALPHA, 2, 0, bd)
        before = ref.e
        want = ref.step(c["m"], c["codes"], ALPHA, SEED, sweep, 2, False)
        prop, got = o.proposal(), o.read()
        assert np.abs(prop["edges"] - want["prop"][1:K]).max() <= 1e-12 and want["ok"]
        # the last pair is alone in workgroup 257: its term must stand out of the bound, or a dropped partial sum would pass
        last = abs(OR.mass_terms(c["m"][-1:], c["codes"][-1:], before, want["prop"], ALPHA)[0])
        assert last > 100 * TOL * n, last
        err = abs(got["S"] - want["S"])
        print(f"257 workgroups, ordinal sweep={sweep}: S {err:.3e} (S = {want['S']:.3f}, margin {abs(want['log_u'] - want['S']):.3e}, "
              f"the last pair's term {last:.3e})")
        assert np.isfinite(got["S"]) and err <= TOL * n, (sweep, got["S"], want["S"])
        if abs(want["log_u"] - want["S"]) > 10 * TOL * n:
            assert prop["accepted"] == want["accepted"]
        full = np.concatenate([[-np.inf], got["edges"], [np.inf]])
        ref.e = full
        bh = bd.cpu().numpy()
        assert np.all(np.isnan(bh[n:]))
        if prop["accepted"]:
            assert np.array_equal(bh[:n], OR.bounds_of(c["codes"], full))
    o.close()
    pairs.close()


# ---- bdf_predict and bdf_predict_update under the four links, for (a) and (c) ----------------------------------------------------
_BASE = {}
LINK_VALUES = {0: "y", 1: "y01", 2: "y01", 3: "counts"}
CUTS = {0: (0.25, 0.2, 0.3), 1: (0.5, 0.45, 0.55), 2: (0.5, 0.45, 0.55), 3: (3.0, 2.5, 3.5)}
LINK_CLAMP = {0: (-1.0, 1.5), 1: (1.0, -1.0), 2: (1.0, -1.0), 3: (1.0, -1.0)}       # (lo > hi: no clamp)


def _link(link, psi):
    return psi if link == 0 else PR.phi(psi) if link == 1 else PG.link(link - 1, psi, float(COUNT_R))


def _predict_raw(ctx, pairs, F, mean):
    from bdf_amd._lib import check, lib
    out = _nan(ctx, pairs.n + 8)
    check(lib().bdf_predict(ctx.handle, pairs.handle, D, _facs(F), mean, _p(out)))
    ctx.sync()
    assert _untouched(out, pairs.n)
    return out.cpu().numpy()[:pairs.n]


def _base(B, ctx, n):
    """the identity kernel's psi on the factors and on the halved factors, held against numpy at 1e-12 relative; once per n"""
    if n not in _BASE:
        c, plain, St = _setup(B, ctx, n, "y")
        b1, b2 = _predict_raw(ctx, plain, St, MEAN), _predict_raw(ctx, plain, [St[0] * 0.5] + St[1:], MEAN)
        plain.close()
        np.testing.assert_allclose(b1, c["m"], rtol=1e-12, atol=0)
        np.testing.assert_allclose(b2, 0.5 * c["u"] + MEAN, rtol=1e-12, atol=0)
        print(f"identity psi n={n}: {max(np.abs(b1 / c['m'] - 1.0).max(), np.abs(b2 / (0.5 * c['u'] + MEAN) - 1.0).max()):.3e}")
        _BASE[n] = (b1, b2)
    return _BASE[n]


def _clamp(x, lo, hi):
    return x if lo > hi else np.minimum(np.maximum(x, lo), hi)


def _check_predict(B, ctx, n, link, edges=False):
    """bdf_predict, then bdf_predict_update phases 1 and 2 (the second on halved factors) on unsorted pairs under `link`: the
    per-pair output, running average and sum of squares against numpy's link of the identity kernel's psi at 1e-12 relative;
    stats[0] and stats[1] against math.fsum at 1e-12 relative; stats[2] and stats[3] as exact integers, with the class cut
    the first of CUTS[link] that no pair's average or prediction comes within 1e-9 of (found on the CPU before the launch; no
    pair excluded).

    1e-12 on the two sums is derived, not measured: a statistic's path is at most two sequential additions in a lane, then
    butterflies and trees of depth about 50 in all (6 + 2 per workgroup, up to 32 + 8 in the final sum), over positive terms each
    good to a few ulp: about 50 x 2.2e-16 ~ 1e-14, and the bound leaves two decades.

    edges: assert the first nine and the last nine pairs separately (in (c) the last nine are the second trip)."""
    from bdf_amd._lib import check, lib
    t0 = time.perf_counter()
    c = _case(n)
    y = c[LINK_VALUES[link]]
    host = time.perf_counter() - t0
    base, base2 = _base(B, ctx, n)
    t0 = time.perf_counter()
    p1, p2 = _link(link, base), _link(link, base2)
    avg2 = (p1 + p2) / 2.0
    near = np.concatenate([p1, p2, avg2])
    cut = next((x for x in CUTS[link] if np.abs(near - x).min() > 1e-9), None)
    assert cut is not None, "every candidate for the class cut is within 1e-9 of some pair"
    lo, hi = LINK_CLAMP[link]
    label = y < cut
    want = []
    for avg, p in ((p1, p1), (avg2, p2)):
        want.append((_fsum((y - _clamp(avg, lo, hi)) ** 2), _fsum((y - _clamp(p, lo, hi)) ** 2),
                     float(np.count_nonzero(label == (avg < cut))), float(np.count_nonzero(label == (p < cut)))))
    host += time.perf_counter() - t0
    t0 = time.perf_counter()
    pairs, St = B.DevicePairs(ctx, c["ids"], y), [ctx.tensor(s) for s in c["S"]]
    if link == 1:
        pairs.set_link(1)
    elif link:
        pairs.set_pg_link(link - 1, float(COUNT_R))
    got = _predict_raw(ctx, pairs, St, MEAN)
    stats = []
    for phase, F in ((1, St), (2, [St[0] * 0.5] + St[1:])):
        st = ctx.tensor(np.full(4, np.nan))
        check(lib().bdf_predict_update(ctx.handle, pairs.handle, D, _facs(F), MEAN, phase, lo, hi, cut, _p(st)))
        ctx.sync()
        stats.append(st.cpu().numpy())
    avg, sq = pairs.state()
    pairs.close()
    dev = time.perf_counter() - t0
    t0 = time.perf_counter()
    worst = 0.0
    for name, g, w in (("out", got, p1), ("avg", avg, avg2), ("sq", sq, p1 * p1 + p2 * p2)):
        assert np.all(np.isfinite(g))
        for where, sl in ((("first nine", slice(0, 9)), ("last nine", slice(n - 9, n))) if edges else ()) + (("all", slice(None)),):
            np.testing.assert_allclose(g[sl], w[sl], rtol=1e-12, atol=0, err_msg=f"{name}, {where} pairs, link {link}")
        worst = max(worst, np.abs(g / w - 1.0).max())
    worst_s = 0.0
    for phase, s, w in zip((1, 2), stats, want):
        for q in (0, 1):
            worst_s = max(worst_s, abs(s[q] / w[q] - 1.0))
            assert abs(s[q] - w[q]) <= 1e-12 * w[q], (link, phase, q, s[q], w[q])
        assert s[2] == w[2] and s[3] == w[3], (link, phase, s, w)
    host += time.perf_counter() - t0
    print(f"predict n={n} link={link} cut={cut}: per pair {worst:.3e}, sums of squares {worst_s:.3e}, counts exact; "
          f"host reference {host:.2f} s, device and copies {dev:.2f} s")


@pytest.mark.parametrize("link", [0, 1, 2, 3])
def test_predict_update_sums_over_257_workgroups(B, ctx, link):
    """k_predict (link 0) and the three link kernels leave 257 workgroups' statistics to k_predict_final"""
    _check_predict(B, ctx, N_FINAL, link)


# ---- (b) 257 workgroups of the sorted kernels ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _runs_case():
    rng = np.random.default_rng(4242)
    dims = [37, 11]
    facs = [rng.standard_normal((d, 32)) * 0.7 for d in dims]
    ids = np.stack([rng.integers(1, d + 1, N_RUNS) for d in dims], axis=1).astype(np.int64)
    return ids, rng.standard_normal(N_RUNS) + 3.0, facs


def test_update_runs_over_257_workgroups(B, ctx):
    """k_update_runs on the pairs sorted by mode 1 (257 workgroups) and k_predict on the unsorted ones (513), phases 1, 2, 2, against
    the model of tests/test_gpu_predict_fit.py, whose _stats adds partial b into slot b % 256 as k_predict_final does: tolerance 0"""
    ids, y, facs = _runs_case()
    _check(B, ctx, ids, y, facs, 32, 1)


def test_predict_runs_over_257_workgroups(B, ctx):
    """k_predict_runs on the same pairs: the raw predictions of the sorted pairs (bdf_predict), and the update of sorted pairs
    that carry a per-pair baseline (bdf_pairs_set_baseline; every entry the mean, so that the model's values are the kernel's),
    phases 1, 2, 2 with k_predict_final over 257 partial sums: tolerance 0"""
    from bdf_amd._lib import check, lib
    ids, y, facs = _runs_case()
    n = N_RUNS
    ft = [ctx.tensor(f.copy()) for f in facs]
    srt = B.DevicePairs(ctx, ids, y).sort(1)
    order = np.argsort(ids[:, 1], kind="stable")
    np.testing.assert_array_equal(srt._order, order)
    lin = ctx.tensor(np.full(n, FIT_MEAN))
    check(lib().bdf_pairs_set_baseline(srt.handle, _p(lin)))
    model = _Model(y)
    f = [x.copy() for x in facs]
    for phase in (1, 2, 2):
        for k in (0, 1):
            ft[k].mul_(0.75)
            f[k] = f[k] * 0.75
        dots = _dots(ids - 1, f, 32)
        raw = srt.predict(32, ft, 123.0).cpu().numpy()               # (with a baseline the mean is a decoy)
        np.testing.assert_array_equal(raw, dots + FIT_MEAN)
        s = srt.update(32, ft, 123.0, phase, list(CLAMP), CUT).cpu().numpy().copy()
        terms = model.update(dots, phase)
        np.testing.assert_array_equal(s, _stats(terms[order], 2), err_msg="statistics of the sorted pairs with a baseline, phase=%d" % phase)
        a, q = srt.state()
        np.testing.assert_array_equal(a, model.avg)
        np.testing.assert_array_equal(q, model.sq)
    print(f"257 workgroups, k_predict_runs: raw predictions, statistics and state equal the model's bits over phases 1, 2, 2; last statistics {s}")
    srt.close()


# ---- (c) the second grid-stride trip ------------------------------------------------------------------------------------------------
def _by_trip(err, n):
    """the last nine pairs (the second trip), the first nine, then all: a failure says which trip"""
    assert err[n - 9:].max() <= TOL, ("second trip", err[n - 9:])
    assert err[:9].max() <= TOL, ("first trip, first nine pairs", err[:9])
    assert err.max() <= TOL, ("first trip", int(np.argmax(err)), err.max())


def test_probit_draw_second_trip(B, ctx):
    """bdf_probit_draw: z against the restatement at 1e-9 over all pairs, linear_out = y - z bit for bit; k_probit_draw's lanes
    past the end `continue` out of the second trip"""
    from bdf_amd._lib import check, lib
    n = N_STRIDE
    t0 = time.perf_counter()
    c = _case(n)
    z_ref = PR.draw_z(c["m"], c["y01"], PR.uniforms(SEED, 11, 2, n))
    host = time.perf_counter() - t0
    t0 = time.perf_counter()
    c, pairs, St = _setup(B, ctx, n, "y01")
    lin, z = _nan(ctx, n + 8), _nan(ctx, n + 8)
    ctx.set_sweep(11)
    check(lib().bdf_probit_draw(ctx.handle, pairs.handle, D, _facs(St), MEAN, 2, _p(lin), _p(z)))
    ctx.sync()
    assert _untouched(lin, n) and _untouched(z, n)
    zh, lh = z.cpu().numpy()[:n], lin.cpu().numpy()[:n]
    pairs.close()
    dev = time.perf_counter() - t0
    err = np.abs(zh - z_ref)
    print(f"second trip, probit: {err.max():.3e} (last nine pairs {err[n - 9:].max():.3e}); host reference {host:.2f} s, device and copies {dev:.2f} s")
    assert np.all(np.isfinite(zh))
    _by_trip(err, n)
    assert np.array_equal(lh, c["y01"] - zh)


def test_censored_draw_second_trip(B, ctx):
    """bdf_censored_draw with alpha through alpha_dev: z at 1e-9 over all pairs, linear_out = mean + (y - z) bit for bit, the
    measured cells' z their values"""
    import torch
    from bdf_amd._lib import check, lib
    n = N_STRIDE
    t0 = time.perf_counter()
    c = _case(n)
    z_ref = CR.draw_z(c["m"], c["y"], c["censor"], ALPHA, CR.uniforms(SEED, 12, 3, n))
    host = time.perf_counter() - t0
    t0 = time.perf_counter()
    c, pairs, St = _setup(B, ctx, n, "y")
    cd = ctx.tensor(c["censor"], dtype=torch.int8)
    lin, z, a_dev = _nan(ctx, n + 8), _nan(ctx, n + 8), ctx.tensor([ALPHA])
    ctx.set_sweep(12)
    check(lib().bdf_censored_draw(ctx.handle, pairs.handle, _p(cd), D, _facs(St), MEAN, 123.0, _p(a_dev), 3, _p(lin), _p(z)))
    ctx.sync()
    assert _untouched(lin, n) and _untouched(z, n)
    zh, lh = z.cpu().numpy()[:n], lin.cpu().numpy()[:n]
    pairs.close()
    dev = time.perf_counter() - t0
    err = np.abs(zh - z_ref)
    print(f"second trip, censored: {err.max():.3e} (last nine pairs {err[n - 9:].max():.3e}); host reference {host:.2f} s, device and copies {dev:.2f} s")
    assert np.all(np.isfinite(zh))
    _by_trip(err, n)
    assert np.array_equal(lh, MEAN + (c["y"] - zh)) and np.array_equal(zh[c["censor"] == 0], c["y"][c["censor"] == 0])


@pytest.mark.parametrize("link", [0, 1, 2, 3])
def test_predict_second_trip(B, ctx, link):
    """k_predict (link 0) and the three predict_link_body kernels: pair_finish accumulates st[] over the two trips of groups 0 and 1
    of workgroup 0, and the width-8 shuffles of the second trip run while the wave's other groups have left the loop"""
    _check_predict(B, ctx, N_STRIDE, link, edges=True)
