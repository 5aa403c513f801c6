"""AUC_ROC and the verbose report of macau() on the device (csrc/k_auc.hip): bdf_auc_roc against the exact-count restatement
(tests/auc_restatement.py) and the host function, bdf_pairs_auc on sorted pairs (ties broken by the caller's index), and a
verbose macau() that never copies a factor matrix or the running average to the host inside its loop."""
import math
import re

import numpy as np
import pytest

import auc_restatement as A

pytestmark = pytest.mark.gpu


def _host_auc(lab, s):
    from bdf_amd import driver
    return driver.AUC_ROC(np.asarray(lab, dtype=bool), np.asarray(s, dtype=np.float64))


def _same(a, b, tol):
    return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= tol


def _device(lab, s, label_dtype="bool"):
    import torch
    from bdf_amd.engine import device_auc_roc
    t_lab = torch.as_tensor(np.asarray(lab, dtype=bool), device="cuda")
    if label_dtype == "uint8":
        t_lab = t_lab.to(torch.uint8) * 7              # any nonzero byte is a positive
    t_s = torch.as_tensor(np.asarray(s, dtype=np.float64), device="cuda")
    return device_auc_roc(t_lab, t_s), t_lab, t_s


def _large_cases():
    rng = np.random.default_rng(11)
    out = []
    for n in (1, 2, 4095, 4096, 4097, 500_000, 5_000_000):
        lab = rng.random(n) < 0.35
        out.append((f"random_{n}", lab, rng.standard_normal(n)))
    n = 500_000
    lab = rng.random(n) < 0.5
    out.append(("ties_500k", lab, np.round(rng.random(n) * 20.0) / 4.0))           # 81 distinct values
    out.append(("narrow_500k", lab, -3.5 - 1e-3 * rng.random(n)))                  # predictions sharing their top bytes
    return out


@pytest.mark.parametrize("case", A.cases(np.random.default_rng(0)) + _large_cases(), ids=lambda c: c[0])
def test_auc_roc_counts_exact_and_auc_matches_host(B, case):
    name, lab, s = case
    (auc, C, P, Nn), t_lab, t_s = _device(lab, s, "uint8" if name.startswith("random_4") else "bool")
    assert (C, P, Nn) == A.counts(lab, s), name
    assert _same(auc, _host_auc(lab, s), 1e-12), (name, auc, _host_auc(lab, s))
    # through the public function: a float, and the same bits on a rerun
    a1, a2 = B.AUC_ROC(t_lab, t_s), B.AUC_ROC(t_lab, t_s)
    assert isinstance(a1, float)
    assert np.array_equal(np.float64(a1).view(np.uint64), np.float64(auc).view(np.uint64))
    assert np.array_equal(np.float64(a2).view(np.uint64), np.float64(auc).view(np.uint64))


def test_auc_roc_numpy_input_stays_on_the_host(B, monkeypatch):
    from bdf_amd import engine

    def no(*a, **k):
        raise AssertionError("numpy input went to the device")
    monkeypatch.setattr(engine, "device_auc_roc", no)
    rng = np.random.default_rng(3)
    lab, s = rng.random(500) < 0.5, rng.standard_normal(500)
    assert B.AUC_ROC(lab, s) == _host_auc(lab, s)


def test_auc_roc_rejects_wrong_dtypes(B):
    import torch
    with pytest.raises(B.ArgumentError):
        B.AUC_ROC(torch.ones(4, dtype=torch.bool, device="cuda"), torch.ones(4, dtype=torch.float32, device="cuda"))
    with pytest.raises(B.DimensionMismatch):
        B.AUC_ROC(torch.ones(3, dtype=torch.bool, device="cuda"), torch.ones(4, dtype=torch.float64, device="cuda"))


def test_pairs_auc_breaks_ties_by_the_callers_index(B, ctx):
    """pairs stored sorted by their first mode, predictions with two values only: breaking the ties in storage order would
    give another C than breaking them in the caller's order, as the host AUC_ROC over the caller's order does"""
    import torch
    from bdf_amd.engine import DevicePairs
    rng = np.random.default_rng(21)
    N1, N2, n, cut = 400, 300, 20_000, 0.3
    ids = np.stack([rng.integers(1, N1 + 1, n), rng.integers(1, N2 + 1, n)], axis=1)
    vals = rng.standard_normal(n)
    U = torch.as_tensor(rng.integers(0, 2, (N1, 1)).astype(np.float64), device="cuda")
    V = torch.ones(N2, 1, dtype=torch.float64, device="cuda")
    pairs = DevicePairs(ctx, ids, vals).sort(0)
    order = pairs._order.copy()
    assert not np.array_equal(order, np.arange(n))
    pairs.update(1, [U, V], 0.25, 0, [], cut)
    counts = torch.zeros(3, dtype=torch.int64, device="cuda")
    pairs.auc(cut, counts=counts)
    ctx.sync()
    got = pairs.report[4].item()
    avg, _ = pairs.state()
    lab, score = vals < cut, -avg
    exp = A.counts(lab, score)
    # the same ranking with ties in storage order: another count
    storage_perm = order[np.argsort(A.keys(score[order]), kind="stable")]
    assert A.counts(lab, score, storage_perm) != exp
    assert tuple(counts.cpu().numpy().tolist()) == exp
    assert abs(got - _host_auc(lab, score)) <= 1e-12
    assert np.array_equal(np.unique(avg), [0.25, 1.25])
    pairs.close()


def _relation(B, seed, features):
    rng = np.random.default_rng(seed)
    N1, N2, nnz = 220, 150, 6000
    ids = np.stack([rng.integers(1, N1 + 1, nnz), rng.integers(1, N2 + 1, nnz)], axis=1)
    vals = np.clip(np.round(3.0 + rng.standard_normal(nnz)), 1, 5)
    e1 = B.Entity("users", F=rng.standard_normal((N1, 12)) if features else None)
    rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": vals}, "ratings", [e1, B.Entity("movies")], dims=[N1, N2],
                     class_cut=3.5)
    B.setPrecision(rel, 1.5)
    B.assignToTest(rel, 1500, rng=np.random.default_rng(seed + 1))
    return B.RelationData(rel)


@pytest.mark.parametrize("features", [False, True])
def test_verbose_macau_reports_from_the_device(B, monkeypatch, capsys, features):
    """verbose macau(): no host AUC and no host copy of an entity's arrays inside the loop; the reported ROC is the host AUC
    of the final average, and every printed U: / β: norm is vecnorm of the array, formatted as before"""
    from bdf_amd import driver, engine
    rd = _relation(B, 5, features)

    def no_host_auc(*a, **k):
        raise AssertionError("driver.AUC_ROC called in the loop")

    def no_host_copy(self, name):
        raise AssertionError(f"EntityState.host({name!r}) called in the loop")
    monkeypatch.setattr(driver, "AUC_ROC", no_host_auc)
    monkeypatch.setattr(engine.EntityState, "host", no_host_copy)
    res = B.macau(rd, num_latent=8, burnin=4, psamples=5, verbose=True, seed=2)
    out = capsys.readouterr().out
    monkeypatch.undo()
    rel = rd.relations[0]
    assert not math.isnan(res["ROC"])
    assert abs(res["ROC"] - _host_auc(rel.test_label, -np.asarray(res["predictions"]["pred"]))) <= 1e-12
    lines = [ln for ln in out.splitlines() if re.match(r"\s*\d+: ROC=", ln)]
    assert len(lines) == 9
    last = lines[-1]
    assert f"ROC={res['ROC']:6.4f}" in last
    for en in rd.entities:
        assert f"U:{np.linalg.norm(en.model.sample):6.2f}" in last, (last, en.name)
    if features:
        assert f" β:{np.linalg.norm(rd.entities[0].model.beta):3.2f}" in last, last


def test_norm2_is_vecnorm_and_repeatable(B, ctx):
    import ctypes as C
    import torch
    from bdf_amd._lib import check, lib
    rng = np.random.default_rng(9)
    for n in (0, 1, 1000, 4097, 3_000_001):
        x = rng.standard_normal(n)
        t = torch.as_tensor(x, device="cuda")
        out = torch.zeros(2, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        for k in range(2):
            check(lib().bdf_norm2(ctx.handle, n, C.c_void_p(t.data_ptr()), C.c_void_p(out.data_ptr() + 8 * k)))
        ctx.sync()
        got = out.cpu().numpy()
        assert got[0].view(np.uint64) == got[1].view(np.uint64)
        assert abs(got[0] - np.linalg.norm(x)) <= 1e-12 * max(1.0, np.linalg.norm(x)), n


def test_movielens_device_roc_equals_host_auc_of_the_final_average(B):
    """MovieLens-1M, 500,000 held out, D = 10, 100 + 400 iterations: the ROC macau() reports (bdf_pairs_auc on the sorted
    test pairs) equals the host AUC_ROC of the final running average"""
    from bdf_amd import datasets
    rd, source = datasets.movielens_relation_data(B)
    if source != "movielens_1m.mat":
        pytest.skip("bundled data file missing")
    res = B.macau(rd, burnin=100, psamples=400, num_latent=10, verbose=False, seed=3)
    rel = rd.relations[0]
    exp = _host_auc(rel.test_label, -np.asarray(res["predictions"]["pred"]))
    assert abs(res["ROC"] - exp) <= 1e-12, (res["ROC"], exp)
    assert 0.5 < res["ROC"] < 1.0
