"""AUC_ROC on the device (csrc/k_auc.hip) as far as it can be checked without one: the exact-count restatement the GPU tests
hold the kernels to agrees with driver.AUC_ROC (src/ROC.jl:1-11), its key order is numpy's stable order, the workspace size,
and the kernels' resource usage.  No GPU needed."""
import glob
import math
import os
import re

import numpy as np
import pytest

import auc_restatement as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(a, b, tol):
    return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= tol


@pytest.mark.parametrize("name", [c[0] for c in A.cases(np.random.default_rng(0))])
def test_restatement_matches_host_auc(B, name):
    from bdf_amd import driver
    lab, s = {c[0]: c[1:] for c in A.cases(np.random.default_rng(0))}[name]
    got, exp = A.auc(lab, s), driver.AUC_ROC(lab, s)
    assert _same(got, exp, 1e-15), (name, got, exp)


@pytest.mark.parametrize("name", [c[0] for c in A.cases(np.random.default_rng(1))])
def test_key_order_is_numpys_stable_order(name):
    """ties (-0.0 with +0.0, NaN with NaN, equal values) keep the caller's order, as argsort(kind="stable") and sortperm"""
    _, s = {c[0]: c[1:] for c in A.cases(np.random.default_rng(1))}[name]
    assert np.array_equal(A.order(s), np.argsort(s, kind="stable"))


@pytest.mark.parametrize("n", [1, 2, 7, 64, 300])
def test_pair_count_is_the_brute_force_count(n):
    rng = np.random.default_rng(n)
    lab = rng.random(n) < 0.5
    for s in (rng.standard_normal(n), np.round(rng.random(n) * 3.0), np.where(rng.random(n) < 0.5, 0.0, -0.0)):
        C, P, Nn = A.counts(lab, s)
        assert isinstance(C, int) and P == int(lab.sum()) and Nn == n - P
        assert C == A.brute_force_count(lab, s)


def test_auc_is_one_rounding_of_the_count():
    rng = np.random.default_rng(5)
    lab = rng.random(100_000) < 0.3
    s = np.round(rng.standard_normal(100_000), 2)
    C, P, Nn = A.counts(lab, s)
    assert A.auc(lab, s) == C / (P * Nn)
    from bdf_amd import driver
    assert abs(A.auc(lab, s) - driver.AUC_ROC(lab, s)) < 1e-15


def test_workspace_size(B):
    f = B.lib().bdf_auc_workspace_bytes
    assert f(-1) == -1
    for n in (0, 1, 4095, 4096, 4097, 500_000, 5_000_000):
        assert f(n) >= 18 * n + 256 * 4 * ((n + 4095) // 4096), n
    assert f(5_000_000) < 19 * 5_000_000


def test_auc_kernels_use_no_scratch():
    """the build's resource report (csrc/k_auc.o.res): no k_auc_* / k_norm2_* kernel keeps registers in scratch memory"""
    res = {}
    for f in glob.glob(os.path.join(ROOT, "bayesiandatafusion.jl_amd", "csrc", "k_auc.o.res")):
        name = None
        for line in open(f):
            m = re.search(r"remark: \s*(Function Name|ScratchSize \[bytes/lane\]|VGPRs Spill): (\S+)", line)
            if not m:
                continue
            if m.group(1) == "Function Name":
                name = m.group(2)
                res[name] = {}
            elif name is not None:
                res[name][m.group(1)] = int(m.group(2))
    for k in ("k_auc_keys", "k_auc_plan", "k_auc_count", "k_auc_scan", "k_auc_scatter", "k_auc_sum", "k_auc_finish",
              "k_norm2_part", "k_norm2_final"):
        assert any(k in name for name in res), (k, sorted(res))
    for k, v in res.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v.get("VGPRs Spill", 0) == 0, (k, v)
