"""bpmf_vb at the edges of its kernels (csrc/k_vb.hip, csrc/bdf_vb.hip) against the row-by-row numpy restatement
(tests/vb_restatement.py), at the tolerances of tests/test_gpu_vb.py.  The inputs are tests/two_mode_edge_inputs.py's, whose
properties tests/test_two_mode_edge_inputs_host.py asserts without a GPU.

  k_vb_rows, gather    degrees 0 .. 5 (waves that hold only zeros), P - 1, P, P + 1, 2P - 1, 2P, 2P + 1, 4P + 1 and Nv - 1 around the
                       pass of P = 4 U neighbours (16; 8 at DP = 64), duplicates on the last neighbour and on the first of the
                       second pass: test_degree_ladder, on U's launch and (transposed) on V's
  padded tiles         D = 16, 17, 32, 33, 63; at D = 17 and 33 the double2 astride Euu | mu lies past the first 128 doubles
  rows per workgroup   N < G, N = G + 1, a single observation: test_fewer_rows_than_a_workgroup_takes
  k_vb_prior_reduce    31, 32, 33 and 34 blocks over VB_SLICES = 32 slices: test_block_counts_around_the_slices
  fixed summation      test_a_ladder_run_is_bit_identical
"""
import numpy as np
import pytest

import two_mode_edge_inputs as I
import vb_restatement as R
from test_gpu_vb import _rel_err, _restate

pytestmark = pytest.mark.gpu

_reference = {}


def _expected(B, key, rd, D, niter, clamp):
    """the restatement's run of a case, computed once per session and left unchanged"""
    if key not in _reference:
        _reference[key] = _restate(B, rd, D, niter, seed=D, clamp=clamp, vectorised=False)
    return _reference[key]


def _worst_row(got, exp, deg):
    """the row (last axis) furthest from the restatement, its degree and its position in the launch's degree-descending order"""
    d = np.abs(np.asarray(got) - np.asarray(exp))
    per_row = d.reshape(-1, d.shape[-1]).max(axis=0)
    n = int(np.argmax(per_row))
    pos = int(np.nonzero(I.launch_order(deg) == n)[0][0])
    return "worst row %d: degree %d, position %d of %d in the launch order, |diff| %.3e" % (n, deg[n], pos, len(deg), per_row[n])


def _run_and_compare(B, key, case, Nu, Nv, D, niter, clamp=()):
    rd = R.relation_data(B, case, Nu, Nv)
    out = B.bpmf_vb(rd, num_latent=D, niter=niter, verbose=False, clamp=clamp, seed=D)
    U, V, rmse, rmse_train = _expected(B, key, rd, D, niter, clamp)
    degs = I.degrees_of(case, Nu, Nv)
    for name, got, exp, deg in (("U", out["Umodel"], U, degs[0]), ("V", out["Vmodel"], V, degs[1])):
        for f in ("mu_u", "Euu"):
            err = _rel_err(getattr(got, f), getattr(exp, f))
            print("%s %s.%s %.3e" % (key, name, f, err))
            assert err < 1e-9, (name, f, err, _worst_row(getattr(got, f), getattr(exp, f), deg))
        for f in ("mu_N", "W_N"):
            err = _rel_err(getattr(got, f), getattr(exp, f))
            print("%s %s.%s %.3e" % (key, name, f, err))
            assert err < 1e-9, (name, f, err)
        assert got.nu_N == exp.nu_N and got.b_N == exp.b_N
    print("%s rmse %.3e rmse_train %.3e" % (key, abs(out["rmse"] - rmse), abs(out["rmse_train"] - rmse_train)))
    assert abs(out["rmse"] - rmse) < 1e-10 and abs(out["rmse_train"] - rmse_train) < 1e-10
    return out


@pytest.mark.parametrize("niter", [1, 3])
@pytest.mark.parametrize("D", I.VB_LADDER_D)
def test_degree_ladder(B, D, niter):
    case, Nu, Nv = I.vb_ladder_case(D)
    clamp = (1.0, 5.0) if D == I.VB_LADDER_CLAMPED_D else ()
    _run_and_compare(B, ("ladder", D, niter), case, Nu, Nv, D, niter, clamp)


@pytest.mark.parametrize("niter", [1, 3])
def test_degree_ladder_on_the_second_entity(B, niter):
    """the same observations transposed: the ladder's rows are V's, updated by the e = 1 launch from the U just written"""
    D = I.VB_LADDER_TRANSPOSED_D
    case, Nu, Nv = I.vb_ladder_case(D, True)
    _run_and_compare(B, ("ladder-transposed", D, niter), case, Nu, Nv, D, niter)


@pytest.mark.parametrize("D,Nu", [(D, Nu) for D, Nu, _ in I.VB_TAIL_CASES])
def test_fewer_rows_than_a_workgroup_takes(B, D, Nu):
    """N_u below, at one less than and one above G = 4 (D = 4) or 2 (D = 20): blocks whose groups are mostly not live; the cases of
    one user have one observation (two_mode_edge_inputs.VB_TAIL_CASES says why)"""
    _run_and_compare(B, ("tail", D, Nu), I.vb_tail_case(D, Nu), Nu, I.VB_TAIL_NV, D, 3)


@pytest.mark.parametrize("D,Nu,Nv", I.VB_SLICE_CASES)
def test_block_counts_around_the_slices(B, D, Nu, Nv):
    """the prior's reduce over 31, 32, 33 blocks (slices empty, one block each, one slice of two) and 34 (two slices of two)"""
    _run_and_compare(B, ("slices", D, Nu), I.vb_slice_case(D, Nu, Nv), Nu, Nv, D, 2)


def test_a_ladder_run_is_bit_identical(B):
    D = 33
    case, Nu, Nv = I.vb_ladder_case(D)
    rd = R.relation_data(B, case, Nu, Nv)
    a, b = (B.bpmf_vb(rd, num_latent=D, niter=3, verbose=False, clamp=(1.0, 5.0), seed=D) for _ in range(2))
    for k in ("Umodel", "Vmodel"):
        for f in ("mu_u", "Euu", "mu_N", "W_N"):
            assert np.array_equal(getattr(a[k], f), getattr(b[k], f)), (k, f)
    assert a["rmse"] == b["rmse"] and a["rmse_train"] == b["rmse_train"]
