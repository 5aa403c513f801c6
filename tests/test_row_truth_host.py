"""tests/row_truth.py on the CPU: the derivation of the exact sample (one Cholesky of the reversed P against the reference's literal
inv / chol in mpmath itself), the working precision, the low-rank restatement against the oracle, and -- for every case
tests/test_gpu_row_conditioning.py runs -- the conditions on the inputs (cond_2(P) per kind, no small pivot) and the float64 yardstick
inside the derived bound 8 D kappa u.  The oracle's literal route is printed beside it: it is the one the second assertion of
row_truth.check would refuse (hundreds of times the yardstick on `alpha`)."""
import numpy as np
import pytest
from mpmath import mp

import row_truth as T

SEED = 1234


def _normals(O, case, sweep=3, tag=11):
    return np.stack([O.normals(SEED, sweep, 1, tag, row, case.D) for row in range(case.N)])


@pytest.mark.parametrize("D,kind", [(8, "alpha"), (32, "prior"), (64, "plain")])
def test_reversed_cholesky_is_the_references_map(O, D, kind):
    """x = J R^-T (J z + R^-1 J b) against chol(inv(P)) z + inv(P) b, both in mpmath at 60 digits, before any rounding: 1e-25
    relative.  (kappa up to 1e8 costs the literal route eight of its sixty digits.)"""
    case = T.make_case(kind, D, 3)
    z = O.normals(SEED, 3, 1, 11, 1, D)
    with mp.workdps(60):
        P, b = T.exact_system(case, 1, True)
        a = T.ref_sample_from(T.chol_mp([r[::-1] for r in P[::-1]]), b, z)
        lit = T.ref_sample_literal(P, b, z)
        rel = max(abs(p - q) for p, q in zip(a, lit)) / max(abs(q) for q in lit)
        assert rel <= mp.mpf(10) ** -25, float(rel)


@pytest.mark.parametrize("kind,D", [("plain", 8), ("prior", 8), ("alpha", 8), ("collinear", 8), ("weights", 8), ("long", 8), ("prior", 64)])
def test_forty_digits_are_enough(O, kind, D):
    """the truth at mp.dps = 40 and at 60 rounds to the same float64s, for the reference's map and the low-rank map"""
    case = T.make_case(kind, D, 3)
    z = _normals(O, case)
    a, b = T.Truth.of(case, 40), T.Truth.of(case, 60)
    for per_row in (False, True):
        assert np.array_equal(a.ref_samples(z, per_row), b.ref_samples(z, per_row))
    if kind not in ("weights", "long"):
        zs = [O.lowrank_normals(SEED, 3, 11, row, D, int(case.counts[row])) for row in range(case.N)]
        assert np.array_equal(a.lowrank_samples(zs, True), b.lowrank_samples(zs, True))


@pytest.mark.parametrize("D", [24, 32, 48, 64])
def test_lowrank_restatement_equals_the_oracle(O, D):
    """the mpmath statement of the low-rank map against orc_sample_row_lowrank on well-conditioned rows (kappa 13 .. 25) of n = D / 2
    observations.  The oracle is float64: what separates the two is its own rounding, four D-term sums or substitutions per element,
    so the bound is D u (5.3e-15 at D = 24, 1.4e-14 at D = 64), the floor row_truth.check gives a D-term substitution.  Measured
    0.7e-15 (D = 24) to 2.3e-15 (D = 64) of the largest element: the 1e-15 the two were expected to agree to is the size of that
    rounding, and no bound it keeps to at D >= 32 (1.1e-15 at D = 64 even with item factors of 0.1, kappa 5).  A restatement that
    took the observations or the normals in another order would be off by about 1."""
    case = T.make_case("plain", D, 4, nobs=(D // 2, D // 2))
    assert np.all(case.counts == D // 2)
    zs = [O.lowrank_normals(SEED, 3, 11, row, D, D // 2) for row in range(case.N)]
    for per_row in (False, True):
        exact = T.Truth.of(case).lowrank_samples(zs, per_row)
        err = T.row_errors(T.lowrank_yardstick(O, case, zs, per_row), exact)
        print(f"low-rank restatement D={D} per_row={per_row}: {err.max():.2e}")
        assert err.max() <= D * T.U


def test_the_index_order_is_the_oracles(O):
    """row_truth orders a row's observations as the oracle's index does (Term.rowids): the low-rank normals delta_a follow that order"""
    case = T.make_case("plain", 24, 26, second=True)
    for t, order, ptr in zip(case.terms, case._order, case._ptr):
        rp, ri = O.index_build(t.ids, [case.N, t.M])[0]
        assert np.array_equal(rp, ptr) and np.array_equal(ri - 1, order)


def _conditions(case, tr):
    lo_hi = T.KAPPA_RANGE.get(case.kind)
    if lo_hi is not None:
        assert np.all(tr.kappa >= lo_hi[0]) and np.all(tr.kappa <= lo_hi[1]), (case.key, tr.kappa.min(), tr.kappa.max())
    # no pivot of the exact reversed factorisation below 1e-9 of max |P|: a correct kernel raises no flag
    assert np.all(tr.min_pivot >= 1e-9 * tr.max_P), (case.key, (tr.min_pivot / tr.max_P).min())


_DISTINCT = sorted({("lr32" if r == "lr32" else None, k, D, nobs, second) for r, k, D, nobs, second in T.route_cases()}, key=repr)


@pytest.mark.parametrize("route,kind,D,nobs,second", _DISTINCT, ids=[f"{k}-{D}-{n}-{s}" for _, k, D, n, s in _DISTINCT])
def test_case_conditions_and_yardstick(O, route, kind, D, nobs, second):
    """every case of the GPU file: cond_2(P) of its kind, no small pivot, and the float64 yardstick within 8 D kappa u of the exact
    sample ((8 D + n) kappa u on rows of n > 64 observations), shared and per-row prior means.  Prints the oracle's literal route."""
    case = T.case_of(route, kind, D, nobs, second)
    tr = T.Truth.of(case)
    _conditions(case, tr)
    z = _normals(O, case)
    for per_row in (False, True):
        exact = tr.ref_samples(z, per_row)
        yard = T.ref_yardstick(case, z, per_row)
        T.check(f"yardstick {case.key} per_row={per_row}", D, tr.kappa, yard, exact, yard, case.counts)
        if kind != "weights":
            orc = T.oracle_samples(O, case, z, per_row)
            print(f"    the oracle's route: worst error / (D kappa u) {T.figures(D, tr.kappa, orc, exact):.3g}, "
                  f"{T.row_errors(orc, exact).max() / max(T.row_errors(yard, exact).max(), D * T.U):.3g} times the yardstick")
    if nobs is not None and kind in ("plain", "prior", "alpha") and D > 16 and nobs[1] <= 32:
        # the low-rank routes: the oracle's low-rank function is the yardstick, kappa = max(cond(Lambda), cond(G))
        zs = [O.lowrank_normals(SEED, 3, 11, row, D, int(case.counts[row])) for row in range(case.N)]
        kap = tr.lowrank_kappa()
        for per_row in (False, True):
            exact = tr.lowrank_samples(zs, per_row)
            yard = T.lowrank_yardstick(O, case, zs, per_row)
            T.check(f"low-rank yardstick {case.key} per_row={per_row}", D, kap, yard, exact, yard, case.counts)


_BLOCKS = T.block_cases()


@pytest.mark.parametrize("kind,D,nv,nu", _BLOCKS, ids=[f"{k}-{D}-{nv}-{nu}" for k, D, nv, nu in _BLOCKS])
def test_block_case_conditions_and_yardstick(O, kind, D, nv, nu):
    case = T.make_case(kind, D, nu, nobs=(nv, nv), block=True)
    assert np.all(case.counts == nv) and len(set(map(tuple, case.terms[0].ids[:, 1].reshape(nu, nv)))) == 1
    tr = T.Truth.of(case)
    _conditions(case, tr)
    z = _normals(O, case)
    yard = T.ref_yardstick(case, z, False)
    T.check(f"yardstick block {case.key}", D, tr.kappa, yard, tr.ref_samples(z, False), yard, nv)


@pytest.mark.parametrize("D", [5, 16, 33, 64])
def test_quad_yardstick(D):
    """|L^-1 v|^2 with the `prior` Lambda: the float64 route within 8 D cond_2(Lambda) u of the mpmath value"""
    rng = np.random.default_rng(4000 + D)
    Lam, V = T.prior_lambda(rng, D), 0.5 * rng.standard_normal((17, D))
    q, qy = T.quad_exact(Lam, V), T.quad_f64(Lam, V)
    assert np.array_equal(q, T.quad_exact(Lam, V, dps=60))
    T.check(f"quad yardstick D={D}", D, np.linalg.cond(Lam), qy[:, None], q[:, None], qy[:, None])
