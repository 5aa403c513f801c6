"""bpmf_vb on the device (csrc/k_vb.hip, csrc/bdf_vb.hip) against the numpy restatement of src/macau_vb.jl
(tests/vb_restatement.py), iteration for iteration from the same initial means."""
import re

import numpy as np
import pytest

import vb_restatement as R

pytestmark = pytest.mark.gpu


def _rel_err(x, y):
    x, y = np.asarray(x), np.asarray(y)
    return np.max(np.abs(x - y)) / max(np.max(np.abs(y)), 1e-300)


def _restate(B, rd, D, niter, seed, clamp=(), vectorised=False, log=None):
    init = B.bpmf_vb(rd, num_latent=D, niter=0, seed=seed)
    rel = rd.relations[0]
    ids, tids = rel.data.ids, rel.test_vec.ids
    return R.run(init["Umodel"], init["Vmodel"], ids[:, 0], ids[:, 1], rel.data.values, tids[:, 0], tids[:, 1],
                 rel.test_vec.values, rel.model.alpha, niter, clamp=clamp, vectorised=vectorised, log=log)


@pytest.mark.parametrize("Nu,Nv,D,clamp", [(300, 200, 10, ()), (257, 123, 32, ()), (90, 140, 7, (1.0, 5.0)), (64, 80, 64, ()),
                                           (50, 40, 1, ())])
def test_parity_with_the_restatement(B, Nu, Nv, D, clamp):
    rd = R.relation_data(B, R.make_case(Nu, Nv, 12 * (Nu + Nv), seed=Nu + D), Nu, Nv)
    out = B.bpmf_vb(rd, num_latent=D, niter=5, verbose=False, clamp=clamp, seed=D)
    U, V, rmse, rmse_train = _restate(B, rd, D, 5, seed=D, clamp=clamp)
    for got, exp in ((out["Umodel"], U), (out["Vmodel"], V)):
        for f in ("mu_u", "Euu", "mu_N", "W_N"):
            assert _rel_err(getattr(got, f), getattr(exp, f)) < 1e-9, (f, _rel_err(getattr(got, f), getattr(exp, f)))
        assert got.nu_N == exp.nu_N and got.b_N == exp.b_N
    assert abs(out["rmse"] - rmse) < 1e-10 and abs(out["rmse_train"] - rmse_train) < 1e-10
    assert out["alpha"] == 2.0


def test_runs_are_bit_identical_and_niter_zero_is_the_start(B):
    Nu, Nv, D = 300, 200, 16
    rd = R.relation_data(B, R.make_case(Nu, Nv, 4000, seed=2), Nu, Nv)
    a = B.bpmf_vb(rd, num_latent=D, niter=4, verbose=False, seed=7)
    b = B.bpmf_vb(rd, num_latent=D, niter=4, verbose=False, seed=7)
    for k in ("Umodel", "Vmodel"):
        for f in ("mu_u", "Euu", "mu_N", "W_N"):
            assert np.array_equal(getattr(a[k], f), getattr(b[k], f)), (k, f)
    assert a["rmse"] == b["rmse"] and a["rmse_train"] == b["rmse_train"]
    z = B.bpmf_vb(rd, num_latent=D, niter=0, seed=7)
    rng = np.random.default_rng(7)
    assert np.array_equal(z["Umodel"].mu_u, B.VBModel(D, Nu, rng).mu_u)
    assert np.array_equal(z["Vmodel"].mu_u, B.VBModel(D, Nv, rng).mu_u)
    assert not np.array_equal(z["Umodel"].mu_u, a["Umodel"].mu_u)


def test_verbose_lines_have_the_reference_format(B, capsys):
    Nu, Nv, D = 60, 50, 4
    rd = R.relation_data(B, R.make_case(Nu, Nv, 600, seed=3), Nu, Nv)
    out = B.bpmf_vb(rd, num_latent=D, niter=3, verbose=True, seed=1)
    lines = capsys.readouterr().out.rstrip("\n").splitlines()
    log = []
    _restate(B, rd, D, 3, seed=1, log=log)
    assert len(lines) == 3
    pat = re.compile(r"^ {0,2}(\d+): \|U\|=(\S+)  \|V\|=(\S+)  RMSE=(\d+\.\d{4})  RMSE\(train\)=(\d+\.\d{4})  \[took \d+\.\d\ds\]$")
    for i, (line, (nu, nv, r, rt)) in enumerate(zip(lines, log), 1):
        m = pat.match(line)
        assert m and len(line.split(":")[0]) == 3, line
        assert int(m.group(1)) == i
        assert m.group(2) == "%.4e" % nu and m.group(3) == "%.4e" % nv, (line, nu, nv)
        assert m.group(4) == "%.4f" % r and m.group(5) == "%.4f" % rt, (line, r, rt)
    assert repr(out["Umodel"]).startswith("VBModel of 60 instances: |mu_u|=")


def test_no_test_rows_gives_nan_rmse(B):
    Nu, Nv = 40, 30
    uid, vid, vals, *_ = R.make_case(Nu, Nv, 300, seed=4)
    rel = B.Relation({"u": uid, "v": vid, "y": vals}, "r", [B.Entity("u"), B.Entity("v")], dims=[Nu, Nv])
    out = B.bpmf_vb(B.RelationData(rel), num_latent=3, niter=2, verbose=False)
    assert np.isnan(out["rmse"]) and np.isfinite(out["rmse_train"])


def test_movielens_d32(B):
    """MovieLens-1M, the bench's 500,000-rating test split, D = 32: three iterations against the vectorised restatement,
    then 20 iterations beat the mean predictor on the test set"""
    from bdf_amd import datasets
    rd, source = datasets.movielens_relation_data(B)
    D = 32
    out = B.bpmf_vb(rd, num_latent=D, niter=3, verbose=False, seed=0)
    U, V, rmse, rmse_train = _restate(B, rd, D, 3, seed=0, vectorised=True)
    for got, exp in ((out["Umodel"], U), (out["Vmodel"], V)):
        for f in ("mu_u", "Euu", "mu_N", "W_N"):
            assert _rel_err(getattr(got, f), getattr(exp, f)) < 1e-8, (f, _rel_err(getattr(got, f), getattr(exp, f)))
    assert abs(out["rmse"] - rmse) < 1e-8 and abs(out["rmse_train"] - rmse_train) < 1e-8
    out = B.bpmf_vb(rd, num_latent=D, niter=20, verbose=False, seed=0)
    rel = rd.relations[0]
    mean_rmse = float(np.sqrt(np.mean((rel.test_vec.values - np.mean(rel.data.values)) ** 2)))
    print(f"\nVB MovieLens-1M ({source}) D=32, 20 iterations: test RMSE {out['rmse']:.4f} (mean predictor {mean_rmse:.4f}), "
          f"train RMSE {out['rmse_train']:.4f}")
    assert out["rmse"] < mean_rmse
