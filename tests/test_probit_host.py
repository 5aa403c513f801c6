"""The probit noise model on the host (no GPU): setProbit and what it guards, the restated draw map of
tests/probit_restatement.py against closed forms, its Philox uniforms against the oracle, and the resource listings the build
leaves for the prediction kernels."""
import glob
import os
import re

import numpy as np
import pytest
from scipy.stats import norm

import probit_restatement as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _relation(B, values=None, n=40, test=None, alpha=2.0):
    rng = np.random.default_rng(3)
    ids = np.stack([rng.integers(1, 9, n), rng.integers(1, 7, n)], axis=1)
    vals = (rng.random(n) < 0.5).astype(np.float64) if values is None else np.asarray(values, dtype=np.float64)
    rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": vals}, "ratings", [B.Entity("u"), B.Entity("v")], alpha=alpha, dims=[8, 6])
    if test is not None:
        B.assignToTest(rel, test)
    return rel


def _is_probit(rel):
    m = rel.model
    return (m.probit is True and m.alpha == 1.0 and m.alpha_sample is False and m.mean_value == 0.0 and rel.class_cut == 0.5
            and np.array_equal(rel.test_label, rel.test_vec.values < 0.5))


def test_default_is_gaussian(B):
    rel = _relation(B)
    assert rel.model.probit is False and B.RelationModel().probit is False


def test_setprobit_after_assign_to_test(B):
    rel = _relation(B, test=np.arange(1, 11))
    assert rel.class_cut == 0.0 and not rel.test_label.any()          # labels under the default cut: nothing is below 0
    B.setProbit(rel)
    assert _is_probit(rel) and len(rel.test_label) == 10
    assert np.array_equal(rel.test_label, rel.test_vec.values == 0.0)


def test_setprobit_before_assign_to_test_and_set_test(B):
    rel = _relation(B)
    B.setProbit(rel)
    assert _is_probit(rel) and len(rel.test_label) == 0
    B.assignToTest(rel, np.arange(1, 11))
    assert _is_probit(rel) and len(rel.test_label) == 10
    rel2 = _relation(B)
    B.setProbit(rel2)
    B.setTest(rel2, {"u": [1, 2, 3], "v": [1, 1, 2], "y": [0.0, 1.0, 1.0]})
    assert _is_probit(rel2) and rel2.test_label.tolist() == [True, False, False]
    with pytest.raises(B.ArgumentError):
        B.setTest(rel2, {"u": [1, 2], "v": [1, 1], "y": [0.0, 0.5]})


def test_setprobit_errors(B):
    vals = (np.arange(40) % 2).astype(np.float64)
    bad = vals.copy()
    bad[7] = 0.5
    with pytest.raises(B.ArgumentError):
        B.setProbit(_relation(B, values=bad))
    bad_test = vals.copy()
    bad_test[2] = 2.0                                 # the offending value sits in the test set
    with pytest.raises(B.ArgumentError):
        B.setProbit(_relation(B, values=bad_test, test=np.array([3, 4])))
    rel = _relation(B, values=vals)
    rel.F = np.ones((40, 2))
    with pytest.raises(B.ArgumentError):
        B.setProbit(rel)
    rel = _relation(B, values=vals)
    rel.model.alpha_sample = True
    with pytest.raises(B.ArgumentError):
        B.setProbit(rel)
    rel = _relation(B, values=vals)
    B.setProbit(rel)
    with pytest.raises(B.ArgumentError):
        B.setPrecision(rel, 3.0)
    assert rel.model.alpha == 1.0


def test_other_samplers_refuse_a_probit_relation(B):
    rel = _relation(B, test=np.arange(1, 6))
    B.setProbit(rel)
    rd = B.RelationData(rel)
    with pytest.raises(B.ArgumentError):
        B.bpmf_vb(rd, num_latent=4, verbose=False, niter=1)
    with pytest.raises(B.ArgumentError):
        B.macau_hmc(rd, num_latent=4, verbose=False, burnin=1, psamples=1)
    with pytest.raises(B.ArgumentError):
        B.GibbsEngine(rd, 4, shard=(0, 2))
    with pytest.raises(B.ArgumentError):
        B.macau(rd, num_latent=4, burnin=1, psamples=1, verbose=False, full_prediction=True)
    rel.model.alpha_sample = True                     # changed behind setProbit's back: the engine looks again
    with pytest.raises(B.ArgumentError):
        B.GibbsEngine(rd, 4)


def test_tostr_marks_probit_and_leaves_gaussian_alone(B):
    rel = _relation(B, alpha=2.0)
    assert B.toStr(rel) == "rati[α=2.0]"
    rel.model.alpha = 12.345
    assert B.toStr(rel) == "rati[α=12.3]"
    B.setProbit(rel)
    assert B.toStr(rel) == "rati[probit]"


@pytest.mark.parametrize("m", [-6.0, -2.0, 0.0, 1.5, 5.0, 9.0])
@pytest.mark.parametrize("y", [0.0, 1.0])
def test_draw_z_mean_matches_the_truncated_normal(m, y):
    """stratified u = (k + 1/2) / n: the mean of the draws is the midpoint rule for the integral of the quantile function, which
    is E[z] = m + s phi(m) / Phi(s m).  The quantile is unbounded at one end (like sqrt(-2 log u)): with n = 2^20 strata the
    rule's error is a few 1e-6; 1e-4 leaves room and still separates any wrong branch (which is off by order 1)."""
    n = 1 << 20
    u = (np.arange(n) + 0.5) / n
    z = PR.draw_z(np.full(n, m), np.full(n, y), u)
    s = 1.0 if y > 0.5 else -1.0
    expect = m + s * norm.pdf(m) / norm.cdf(s * m)
    assert np.all(np.isfinite(z)) and np.all((z > 0) == (y > 0.5))
    assert abs(z.mean() - expect) <= 1e-4 * max(1.0, abs(expect)), (z.mean(), expect)
    assert np.all(np.diff(s * z) >= 0)                 # the map is monotone in u


def test_draw_z_is_finite_and_on_the_right_side_everywhere():
    m = np.linspace(-40.0, 40.0, 16001)
    for u in (2.0 ** -54, 1.0 - 2.0 ** -54, 0.5):       # the smallest and the largest uniform bdf_u01 can return
        for y in (0.0, 1.0):
            z = PR.draw_z(m, np.full_like(m, y), np.full_like(m, u))
            assert np.all(np.isfinite(z))
            assert np.all(z > 0) if y else np.all(z < 0)


def test_uniforms_are_the_library_stream(O):
    for seed, sweep, tag in ((42, 1, 1), (0xDEADBEEF12345, 7, 3)):
        u = PR.uniforms(seed, sweep, tag, 50)
        for k in (0, 1, 17, 49):
            o = O.draw(seed, sweep, PR.P_PROBIT, 0x800000 | tag, k, 0)
            x = (int(o[1]) << 32) | int(o[0])
            assert u[k] == ((x >> 11) + 0.5) * 2.0 ** -53
    assert 0.0 < PR.uniforms(1, 1, 1, 1000).min() and PR.uniforms(1, 1, 1, 1000).max() < 1.0


def test_purpose_number_matches_the_header(B):
    h = open(os.path.join(ROOT, "include", "bdf.h")).read()
    assert re.search(r"#define BDF_P_PROBIT\s+12\b", h)
    from bdf_amd import _lib
    assert _lib.P_PROBIT == PR.P_PROBIT == 12


# (VGPRs, scratch bytes per lane, waves per SIMD) of the prediction kernels before the probit link was added: the link lives in
# kernels of its own (k_probit.hip) and these, which the benchmark's iteration runs, must not move
PREDICT_KERNELS = {
    "14k_predict_runsENS_8PredArgsE": (126, 0, 4),
    "15k_predict_finalEiPKdPd": (22, 0, 8),
    "13k_predict_allENS_11PredAllArgsE": (28, 0, 8),
    "9k_predictILi1ELi1ELi1EEEvNS_8PredArgsE": (54, 0, 8),
    "9k_predictILi2ELi1ELi1EEEvNS_8PredArgsE": (64, 0, 8),
    "9k_predictILi3ELi1ELi1EEEvNS_8PredArgsE": (70, 0, 7),
    "9k_predictILi4ELi1ELi1EEEvNS_8PredArgsE": (78, 0, 6),
    "9k_predictILi2ELi4ELi1EEEvNS_8PredArgsE": (117, 0, 4),
    "9k_predictILi3ELi4ELi1EEEvNS_8PredArgsE": (152, 0, 3),
    "9k_predictILi4ELi4ELi1EEEvNS_8PredArgsE": (124, 0, 4),
    "9k_predictILi2ELi4ELi2EEEvNS_8PredArgsE": (118, 0, 4),
    "9k_predictILi3ELi4ELi2EEEvNS_8PredArgsE": (151, 0, 3),
    "9k_predictILi4ELi4ELi2EEEvNS_8PredArgsE": (185, 0, 2),
}


def _resources(unit):
    path = os.path.join(ROOT, "bayesiandatafusion.jl_amd", "csrc", unit + ".o.res")
    assert glob.glob(path), "no csrc/%s.o.res: build with __graft_entry__.build() (make)" % unit
    res, name = {}, None
    for line in open(path):
        m = re.search(r"remark: \s*(Function Name|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = m.group(2).replace("_ZN12_GLOBAL__N_1", "")
            res[name] = {}
        elif name is not None:
            res[name][m.group(1).split(" ")[0]] = int(m.group(2))
    return {k: (v["VGPRs"], v["ScratchSize"], v["Occupancy"]) for k, v in res.items()}


def test_prediction_kernels_kept_their_resources_and_the_probit_kernels_use_no_scratch():
    assert _resources("k_predict") == PREDICT_KERNELS
    probit = _resources("k_probit")
    draws = {k: v for k, v in probit.items() if "k_probit_draw" in k}
    links = {k: v for k, v in probit.items() if "k_predict_link" in k}
    assert len(draws) == 9 and len(links) == 9
    for k, v in {**draws, **links}.items():
        assert v[1] == 0 and v[2] >= 2, (k, v)
    assert draws["13k_probit_drawILi2ELi4ELi1EEEvNS_8DrawArgsE"][2] >= 3      # two modes, D <= 32: the MovieLens draw
