"""The censored (Tobit) noise model on the host (no GPU): setCensored and what it guards, the restated draw map of
tests/censored_restatement.py against closed forms and scipy's truncated normal, its Philox uniforms against the oracle, and the
resource listings the build leaves for the new kernels and for the units that now share pair_gather.h."""
import os
import re

import numpy as np
import pytest
from scipy.stats import norm, truncnorm

import censored_restatement as CR
from test_probit_host import PREDICT_KERNELS, _resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _relation(B, n=40, test=None, alpha=2.0):
    rng = np.random.default_rng(3)
    ids = np.stack([rng.integers(1, 9, n), rng.integers(1, 7, n)], axis=1)
    rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": rng.standard_normal(n)}, "ratings", [B.Entity("u"), B.Entity("v")], alpha=alpha, dims=[8, 6])
    if test is not None:
        B.assignToTest(rel, test)
    return rel


def _flags(n, seed=5):
    return np.random.default_rng(seed).integers(-1, 2, n)


# ---- setCensored ------------------------------------------------------------------------------------------------------------
def test_default_has_no_flags(B):
    assert _relation(B).model.censor is None and B.RelationModel().censor is None


def test_setcensored_stores_int8_flags_and_resets_the_device_state(B):
    rel = _relation(B, test=np.arange(1, 11))
    rel._dev = object()
    c = _flags(30)
    assert B.setCensored(rel, c) is None
    assert rel.model.censor.dtype == np.int8 and np.array_equal(rel.model.censor, c) and rel._dev is None
    assert rel.model.alpha == 2.0 and rel.model.alpha_sample is False and rel.model.probit is False
    B.setCensored(rel, [0] * 30)                                   # a list works; the flags are replaced
    assert not rel.model.censor.any()
    B.setPrecision(rel, 3.0)                                       # the precision stays a parameter
    rel.model.alpha_sample = True
    assert rel.model.alpha == 3.0 and rel.model.censor is not None


def test_setcensored_refuses_a_wrong_length_and_other_values(B):
    rel = _relation(B, test=np.arange(1, 11))
    for bad in (_flags(40), _flags(29), np.zeros((30, 1), dtype=int), np.full(30, 2), np.full(30, -2), np.zeros(30), np.full(30, 0.5)):
        with pytest.raises(B.ArgumentError):
            B.setCensored(rel, bad)
    assert rel.model.censor is None


def test_order_relative_to_the_test_split(B):
    rel = _relation(B)
    B.setCensored(rel, _flags(40))
    with pytest.raises(B.ArgumentError, match="assignToTest before setCensored"):
        B.assignToTest(rel, np.arange(1, 11))
    assert rel.data.nnz() == 40 and len(rel.test_vec) == 0         # nothing was split off
    B.setTest(rel, {"u": [1, 2, 3], "v": [1, 1, 2], "y": [0.1, 1.0, -1.0]})     # setTest leaves the training rows alone
    assert len(rel.test_vec) == 3 and len(rel.model.censor) == 40
    rel2 = _relation(B)
    B.setTest(rel2, {"u": [1, 2, 3], "v": [1, 1, 2], "y": [0.1, 1.0, -1.0]})
    B.setCensored(rel2, _flags(40))
    assert len(rel2.model.censor) == 40
    rel3 = _relation(B, test=np.arange(1, 11))                     # the documented order
    B.setCensored(rel3, _flags(30))


def test_setcensored_refuses_features_and_probit(B):
    rel = _relation(B)
    rel.F = np.ones((40, 2))
    with pytest.raises(B.ArgumentError):
        B.setCensored(rel, _flags(40))
    vals = (np.arange(40) % 2).astype(np.float64)
    ids = np.stack([np.arange(40) % 8 + 1, np.arange(40) % 6 + 1], axis=1)

    def binary():
        return B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": vals}, "bin", [B.Entity("u"), B.Entity("v")], dims=[8, 6])

    rel = binary()
    B.setProbit(rel)
    with pytest.raises(B.ArgumentError):
        B.setCensored(rel, _flags(40))
    rel = binary()
    B.setCensored(rel, _flags(40))
    with pytest.raises(B.ArgumentError):
        B.setProbit(rel)
    assert rel.model.probit is False


def test_samplers_refuse_what_the_censored_model_does_not_cover(B):
    rel = _relation(B, test=np.arange(1, 6))
    B.setCensored(rel, _flags(35))
    rd = B.RelationData(rel)
    with pytest.raises(B.ArgumentError):
        B.bpmf_vb(rd, num_latent=4, verbose=False, niter=1)
    with pytest.raises(B.ArgumentError):
        B.macau_hmc(rd, num_latent=4, verbose=False, burnin=1, psamples=1)
    with pytest.raises(B.ArgumentError):
        B.GibbsEngine(rd, 4, shard=(0, 2))
    with pytest.raises(B.ArgumentError):
        B.macau(rd, num_latent=4, burnin=1, psamples=1, verbose=False, rmse_train=True)
    # changed behind setCensored's back: the engine looks again (check_censored)
    from bdf_amd.relation_data import check_censored
    keep = rel.model.censor
    rel.model.censor = keep[:-1]
    with pytest.raises(B.ArgumentError):
        B.GibbsEngine(rd, 4)
    rel.model.censor = np.full(35, 3)
    with pytest.raises(B.ArgumentError):
        check_censored(rel)
    rel.model.censor = keep
    rel.F = np.ones((35, 2))
    with pytest.raises(B.ArgumentError):
        B.GibbsEngine(rd, 4)
    rel.F = None
    rel.model.probit = True
    with pytest.raises(B.ArgumentError):
        check_censored(rel)
    rel.model.probit = False
    check_censored(rel)


def test_tostr_counts_the_censored_rows_and_leaves_the_others_alone(B):
    rel = _relation(B, alpha=2.0)
    assert B.toStr(rel) == "rati[α=2.0]"
    c = np.zeros(40, dtype=int)
    c[:7], c[7:12] = 1, -1
    B.setCensored(rel, c)
    assert B.toStr(rel) == "rati[α=2.0 cens:12]"
    B.setCensored(rel, np.zeros(40, dtype=int))
    assert B.toStr(rel) == "rati[α=2.0 cens:0]"


# ---- the restated map ---------------------------------------------------------------------------------------------------------
def test_purpose_number_matches_the_header(B):
    h = open(os.path.join(ROOT, "include", "bdf.h")).read()
    assert re.search(r"#define BDF_P_CENSORED\s+13\b", h)
    from bdf_amd import _lib
    assert _lib.P_CENSORED == CR.P_CENSORED == 13


def test_uniforms_are_the_library_stream(O):
    for seed, sweep, tag in ((42, 1, 1), (0xDEADBEEF12345, 7, 3)):
        u = CR.uniforms(seed, sweep, tag, 50)
        for k in (0, 1, 17, 49):
            o = O.draw(seed, sweep, CR.P_CENSORED, 0x800000 | tag, k, 0)
            x = (int(o[1]) << 32) | int(o[0])
            assert u[k] == ((x >> 11) + 0.5) * 2.0 ** -53
    import probit_restatement as PR
    assert not np.array_equal(CR.uniforms(1, 1, 1, 8), PR.uniforms(1, 1, 1, 8))         # a stream of its own


@pytest.mark.parametrize("alpha", [0.04, 5.0, 900.0])
@pytest.mark.parametrize("t", [-6.0, -2.0, 0.0, 1.5, 5.0, 9.0])
@pytest.mark.parametrize("c", [1, -1])
def test_draw_z_mean_matches_the_truncated_normal(t, c, alpha):
    """stratified u = (k + 1/2) / n: the mean of the draws is the midpoint rule for the integral of the quantile function, which
    is E[z] = m + s phi(t) / (Phi(t) sqrt(alpha)), t = s (m - y) sqrt(alpha).  The quantile is unbounded at one end (like
    sqrt(-2 log u)): with n = 2^20 strata the rule's error is a few 1e-6 standard deviations; 1e-4 leaves room and still separates
    any wrong branch or a misplaced sqrt(alpha) (off by order 1)."""
    n = 1 << 20
    u = (np.arange(n) + 0.5) / n
    ra, y = np.sqrt(alpha), 0.7
    m = y + c * t / ra
    z = CR.draw_z(np.full(n, m), np.full(n, y), np.full(n, c), alpha, u)
    expect = m + c * norm.pdf(t) / (norm.cdf(t) * ra)
    assert np.all(np.isfinite(z)) and np.all(c * (z - y) >= 0)
    assert abs(z.mean() - expect) * ra <= 1e-4 * max(1.0, abs(t)), (z.mean(), expect)
    assert np.all(np.diff(c * z) >= 0)                 # the map runs from the bound outward, monotone in u


def test_draw_z_is_finite_and_on_the_right_side_everywhere():
    t = np.linspace(-45.0, 45.0, 18001)
    for alpha in (1e-2, 0.3, 1.0, 40.0, 1e3):
        ra = np.sqrt(alpha)
        for u in (2.0 ** -54, 1.0 - 2.0 ** -53, 1.0, 0.5):     # the smallest uniform, the largest below 1, and 1 itself (rounding)
            for c in (1, -1):
                for y in (0.0, -3.25, 1e3):
                    m = y + c * t / ra
                    z = CR.draw_z(m, np.full_like(t, y), np.full(t.shape, c), alpha, np.full_like(t, u))
                    assert np.all(np.isfinite(z))
                    assert np.all(c * (z - y) >= 0)
    # below the underflow of Phi(t) the draw is at or near the bound: the exact law lies within about sd / 37 of it
    z = CR.draw_z(np.array([-45.0, -40.0]), np.zeros(2), np.ones(2, dtype=int), 1.0, np.array([0.5, 0.999]))
    assert np.all(z >= 0.0) and np.all(z <= 1.0 / 37.0)


def test_exact_observations_keep_their_value():
    rng = np.random.default_rng(0)
    m, y, u = rng.standard_normal(100) * 50, rng.standard_normal(100), rng.random(100)
    assert np.array_equal(CR.draw_z(m, y, np.zeros(100, dtype=int), 3.0, u), y)


def test_draw_z_matches_scipy_where_scipy_is_accurate():
    """|t| <= 8 only: there truncnorm.ppf is itself accurate.  For c = +1 the map is the quantile at u of N(m, 1 / alpha) on
    [y, inf); for c = -1 it runs from the bound outward, so it is the quantile at 1 - u on (-inf, y].  The uniforms are multiples
    of 2^-12, for which 1 - u is exact.  Bound: the project's 1e-9 for a kernel against its restatement, in standard deviations."""
    rng = np.random.default_rng(11)
    n = 20000
    u = rng.integers(1, 4096, n) / 4096.0
    worst = 0.0
    for alpha in (1e-2, 0.5, 4.0, 1e3):
        sd = 1.0 / np.sqrt(alpha)
        t = rng.uniform(-8.0, 8.0, n)
        y = rng.standard_normal(n) * 3.0
        for c in (1, -1):
            m = y + c * t * sd
            z = CR.draw_z(m, y, np.full(n, c), alpha, u)
            if c > 0:
                ref = truncnorm.ppf(u, (y - m) / sd, np.inf, loc=m, scale=sd)
            else:
                ref = truncnorm.ppf(1.0 - u, -np.inf, (y - m) / sd, loc=m, scale=sd)
            worst = max(worst, np.abs(z - ref).max() / sd)
    print(f"draw_z against scipy.stats.truncnorm.ppf over |t| <= 8: worst |z - ref| sqrt(alpha) = {worst:.3e}")
    assert worst <= 1e-9


# ---- the resource listings ----------------------------------------------------------------------------------------------------
# (VGPRs, scratch bytes per lane, waves per SIMD) of the kernels of k_probit.hip before group_dots and BDF_BY_SHAPE moved to
# pair_gather.h: the move must not change them
PROBIT_KERNELS = {
    "15k_predict_finalEiPKdPd": (22, 0, 8),
    "14k_predict_linkILi2ELi1ELi1EEEvNS_8PredArgsE": (125, 0, 4),
    "14k_predict_linkILi2ELi4ELi1EEEvNS_8PredArgsE": (178, 0, 2),
    "14k_predict_linkILi2ELi4ELi2EEEvNS_8PredArgsE": (179, 0, 2),
    "14k_predict_linkILi3ELi1ELi1EEEvNS_8PredArgsE": (131, 0, 3),
    "14k_predict_linkILi3ELi4ELi1EEEvNS_8PredArgsE": (213, 0, 2),
    "14k_predict_linkILi3ELi4ELi2EEEvNS_8PredArgsE": (212, 0, 2),
    "14k_predict_linkILi4ELi1ELi1EEEvNS_8PredArgsE": (139, 0, 3),
    "14k_predict_linkILi4ELi4ELi1EEEvNS_8PredArgsE": (185, 0, 2),
    "14k_predict_linkILi4ELi4ELi2EEEvNS_8PredArgsE": (245, 0, 2),
    "13k_probit_drawILi2ELi1ELi1EEEvNS_8DrawArgsE": (137, 0, 3),
    "13k_probit_drawILi2ELi4ELi1EEEvNS_8DrawArgsE": (168, 0, 3),
    "13k_probit_drawILi2ELi4ELi2EEEvNS_8DrawArgsE": (168, 0, 3),
    "13k_probit_drawILi3ELi1ELi1EEEvNS_8DrawArgsE": (139, 0, 3),
    "13k_probit_drawILi3ELi4ELi1EEEvNS_8DrawArgsE": (168, 0, 3),
    "13k_probit_drawILi3ELi4ELi2EEEvNS_8DrawArgsE": (168, 0, 3),
    "13k_probit_drawILi4ELi1ELi1EEEvNS_8DrawArgsE": (142, 0, 3),
    "13k_probit_drawILi4ELi4ELi1EEEvNS_8DrawArgsE": (168, 0, 3),
    "13k_probit_drawILi4ELi4ELi2EEEvNS_8DrawArgsE": (243, 0, 2),
}


def test_censored_kernels_use_no_scratch_and_the_shared_units_kept_their_resources():
    assert _resources("k_predict") == PREDICT_KERNELS
    assert _resources("k_probit") == PROBIT_KERNELS
    draws = _resources("k_censored")
    assert len(draws) == 9 and all("k_censored_draw" in k for k in draws)
    for k, v in draws.items():
        assert v[1] == 0 and v[2] >= 2, (k, v)
    assert draws["15k_censored_drawILi2ELi4ELi1EEEvNS_8CensArgsE"][2] >= 3      # two modes, D <= 32: the MovieLens draw
    path = os.path.join(ROOT, "bayesiandatafusion.jl_amd", "csrc", "k_censored.o.res")
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", open(path).read())]
    assert len(lds) == 9 and not any(lds)
