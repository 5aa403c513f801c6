"""Host checks of the inputs of tests/test_gpu_vb_edges.py and tests/test_gpu_hmc_edges.py (tests/two_mode_edge_inputs.py): every
case has the degrees, block counts and duplicates its GPU test relies on, and every HMC case the accept / reject / adapt sequence
and the Metropolis margin, by the restatement alone.  A seed edited later cannot turn an edge case into an ordinary one unnoticed.
No GPU."""
import math

import numpy as np
import pytest

import two_mode_edge_inputs as I
import vb_restatement as R


def _check_duplicates(case, Nu, Nv, deg_u, P):
    """rows longer than a pass list their first neighbour of the second pass and their last neighbour twice; no other row lists
    any pair twice, and no pair is listed three times"""
    dup = I.duplicate_positions(case, Nu, Nv)
    long_rows = {int(u) for u in np.nonzero(deg_u > P)[0]}
    assert set(dup) == long_rows and long_rows
    for u, pos in dup.items():
        assert pos == sorted({P, int(deg_u[u]) - 1}), (u, pos, deg_u[u])
    uid, vid = case[0], case[1]
    assert len(uid) == deg_u.sum() + sum(len(p) for p in dup.values())


def test_generator_basics():
    Nu, Nv = 9, 30
    deg = [0, 1, 29, 17, 16, 5, 0, 18, 2]
    case = I.make_edge_case(Nu, Nv, deg, seed=1, ntest=40, pass_size=16)
    uid, vid, vals, tu, tv, tval = case
    du, dv = I.degrees_of(case, Nu, Nv)
    assert np.array_equal(du, deg) and dv[-1] == 0 and dv.sum() == sum(deg)
    assert uid.min() >= 1 and uid.max() <= Nu and vid.min() >= 1 and vid.max() <= Nv - 1
    assert vals.min() >= 1.0 and vals.max() <= 5.0 and tval.min() >= 1.0 and tval.max() <= 5.0 and len(tval) == 40
    assert np.any(np.diff(uid) < 0)                                        # shuffled: the library sorts by row itself
    # the row of degree 17 = 16 + 1: its last neighbour is its first of the second pass, one duplicate
    assert I.duplicate_positions(case, Nu, Nv) == {2: [16, 28], 3: [16], 7: [16, 17]}
    # the restatement's sparse matrix counts the same degrees
    S = R.sparse_data(uid, vid, vals, Nu, Nv)
    assert np.array_equal(np.diff(S.indptr), deg)
    # transpose swaps the modes and nothing else
    t = I.transpose(case)
    assert t[0] is vid and t[1] is uid and t[3] is tv and t[4] is tu
    tdu, tdv = I.degrees_of(t, Nv, Nu)
    assert np.array_equal(tdu, dv) and np.array_equal(tdv, du)
    assert list(I.launch_order([3, 5, 3, 9])) == [3, 1, 0, 2]
    assert [I.padded(D) for D in (1, 16, 17, 32, 33, 64)] == [16, 16, 32, 32, 64, 64]
    assert [I.vb_pass(D) for D in (16, 32, 33)] == [16, 16, 8] and [I.hmc_pass(D) for D in (16, 32, 33)] == [64, 32, 16]


def test_the_training_rows_reach_the_library_in_the_case_s_order(B):
    """hmc_expected runs the restatement on the case's own arrays; the GPU test hands the library R.relation_data of them: the
    same rows in the same order, so the same mean to the bit"""
    case, Nu, Nv = I.hmc_ladder_case(16)
    rel = R.relation_data(B, case, Nu, Nv).relations[0]
    assert np.array_equal(rel.data.ids[:, 0], case[0]) and np.array_equal(rel.data.ids[:, 1], case[1])
    assert np.array_equal(rel.data.values, case[2])
    assert np.array_equal(rel.test_vec.ids[:, 0], case[3]) and np.array_equal(rel.test_vec.ids[:, 1], case[4])
    assert np.array_equal(rel.test_vec.values, case[5])


@pytest.mark.parametrize("D", I.VB_LADDER_D)
def test_vb_ladder_cases(D):
    case, Nu, Nv = I.vb_ladder_case(D)
    P, G = I.vb_pass(D), I.vb_rows_per_block(D)
    assert P == (16 if D <= 32 else 8) and Nv >= 4 * P + 3
    du, dv = I.degrees_of(case, Nu, Nv)
    want = {0, 1, 2, 3, 4, 5, P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1, 4 * P + 1, Nv - 1, 7}
    assert set(du) == want and dv[-1] == 0
    assert (du == 7).sum() == Nu - 14 + (P == 8)                           # the filler rows (P - 1 = 7 at P = 8)
    # the last block of the U launch has live and dead groups wherever a block takes more than one row
    assert G == 1 or Nu % G != 0
    assert I.vb_row_blocks(D, Nu) == -(-Nu // G) < I.VB_SLICES
    # T = D (D + 1) / 2: odd and past the first 128-double stretch at D = 17 and 33, so the double2 astride Euu | mu is in a later chunk
    T = D * (D + 1) // 2
    assert (D not in (17, 33)) or (T % 2 == 1 and T > 128)
    _check_duplicates(case, Nu, Nv, du, P)


def test_vb_transposed_ladder():
    D = I.VB_LADDER_TRANSPOSED_D
    case, Nu, Nv = I.vb_ladder_case(D, True)
    base, bNu, bNv = I.vb_ladder_case(D)
    assert (Nu, Nv) == (bNv, bNu)
    du, dv = I.degrees_of(case, Nu, Nv)
    bu, bv = I.degrees_of(base, bNu, bNv)
    assert np.array_equal(dv, bu) and np.array_equal(du, bv) and du[-1] == 0
    assert D == 17 and I.vb_rows_per_block(D) == 2


def test_vb_row_tail_cases():
    seen = set()
    for D, Nu, deg in I.VB_TAIL_CASES:
        case = I.vb_tail_case(D, Nu)
        du, dv = I.degrees_of(case, Nu, I.VB_TAIL_NV)
        assert np.array_equal(du, deg) and du.min() >= 1 and dv[-1] == 0
        seen.add((I.vb_rows_per_block(D), Nu))
    assert seen == {(4, 1), (4, 2), (4, 3), (4, 5), (2, 1), (2, 3)}
    assert len(I.vb_tail_case(4, 1)[0]) == 1 and len(I.vb_tail_case(20, 1)[0]) == 1      # one row, one observation


def test_vb_slice_cases():
    blocks = []
    for D, Nu, Nv in I.VB_SLICE_CASES:
        case = I.vb_slice_case(D, Nu, Nv)
        du, dv = I.degrees_of(case, Nu, Nv)
        assert du.min() >= 1 and dv[-1] == 0
        blocks.append((I.vb_rows_per_block(D), I.vb_row_blocks(D, Nu)))
    S = I.VB_SLICES
    assert blocks == [(1, S - 1), (1, S), (1, S + 1), (4, S + 2)]
    # 34 blocks over 32 slices: slices of one and of two blocks, and the last block of the launch has one live group of four
    sizes = {34 * (s + 1) // S - 34 * s // S for s in range(S)}
    assert sizes == {1, 2} and (4 * 33 + 1) % 4 == 1
    assert {31 * (s + 1) // S - 31 * s // S for s in range(S)} == {0, 1}   # below VB_SLICES a slice is empty


@pytest.mark.parametrize("D", list(I.HMC_LADDER_EPS))
def test_hmc_ladder_cases(D):
    case, Nu, Nv = I.hmc_ladder_case(D)
    NG, P = I.hmc_groups(D), I.hmc_pass(D)
    assert (NG, P) == {16: (16, 64), 32: (8, 32), 64: (4, 16)}[I.padded(D)]
    du, dv = I.degrees_of(case, Nu, Nv)
    assert set(du) == {0, 1, 2, NG - 1, NG, NG + 1, P - 1, P, P + 1, 2 * P + 1, Nv - 1, 7} and dv[-1] == 0
    assert (du < NG).any() and (dv < NG).any()                             # groups that get no neighbour at all, in both launches
    # the accept kernel's loop over a launch's blocks (one per row) takes a second and a third trip with a tail
    for n in (Nu, Nv):
        assert n > 64 and n % 64 != 0
    assert Nv > 128
    # the restore launch: both entities past one block of 256 and unequal; the predict launch past one block by one pair
    assert Nu * D > 256 and Nv * D > 256 and Nu * D != Nv * D
    assert len(case[5]) == 257
    _check_duplicates(case, Nu, Nv, du, P)
    assert list(I.HMC_LADDER_EPS) == [16, 17, 32, 33, 63]


def test_hmc_small_and_transposed_and_predict_cases():
    Nu, Nv = I.HMC_SMALL_SHAPE
    D = I.HMC_SMALL_D
    NG, P = I.hmc_groups(D), I.hmc_pass(D)
    du, dv = I.degrees_of(I.hmc_small_case(), Nu, Nv)
    assert set(du) == {0, 1, 2, NG - 1, NG, NG + 1, P - 1, P, P + 1, Nv - 1} and dv[-1] == 0
    _check_duplicates(I.hmc_small_case(), Nu, Nv, du, P)
    assert I.HMC_L_CASES == [(1, 1), (1, 3), (2, 2), (2, 3)]
    case, tNu, tNv = I.hmc_ladder_case(I.HMC_LADDER_TRANSPOSED_D, True)
    assert (tNu, tNv) == (I.HMC_NV, I.HMC_NU) and tNu * 16 > tNv * 16 > 256      # n[0] > n[1] in the restore launch
    tdu, tdv = I.degrees_of(case, tNu, tNv)
    assert tdv.max() == tNu - 1 and tdu[-1] == 0                            # the long rows are V's
    pcase = I.hmc_scenarios()["predict"][0]
    assert len(pcase[5]) == 600 and -(-600 // 256) == 3 and 600 % 256 != 0
    kw = I.hmc_scenarios()["predict"][5]
    assert kw["burnin"] == 2 and kw["psamples"] == 4 and kw["clamp"] == ()


def test_every_hmc_decision_has_a_margin():
    """every iteration with dH < 0 decides by more than a rounding difference: |uniform - exp(dH)| >= 1e-6 max(uniform, exp(dH))"""
    for name in I.hmc_scenarios():
        exp = I.hmc_expected(name)
        for i, (m, r) in enumerate(zip(I.metropolis_margins(exp), exp["records"]), 1):
            assert math.isfinite(r["dH"]), (name, i)
            assert m is None or m >= 1e-6, (name, i, r["dH"], r["uniform"])
            assert r["accepted"] == (r["dH"] >= 0 or r["uniform"] < math.exp(r["dH"]))


def test_hmc_ladders_accept_most_iterations():
    for name in I.hmc_scenarios():
        if name.startswith("ladder"):
            acc = [r["accepted"] for r in I.hmc_expected(name)["records"]]
            assert len(acc) == 5 and sum(acc) >= 3, (name, acc)
    for L, Li in I.HMC_L_CASES:
        rec = I.hmc_expected("steps-%d-%d" % (L, Li))["records"]
        assert all(r["L"] == L for r in rec) and any(r["accepted"] for r in rec)
    assert any(r["accepted"] for r in I.hmc_expected("predict")["records"][2:])   # the running mean takes new samples


def test_the_adaptation_scenarios_run_as_written():
    rec = I.hmc_expected("adapt-then-onward")["records"]
    assert [r["accepted"] for r in rec] == [False, False, True, True, False, True]
    assert [(r["eps"], r["L"]) for r in rec] == [(0.2, 3), (0.1, 5), (0.05, 8), (0.05, 8), (0.05, 8), (0.05, 8)]
    assert [(r["eps_new"], r["L_new"]) for r in rec] == [(0.1, 5), (0.05, 8)] + [(0.05, 8)] * 4
    assert rec[0]["dH"] < -1000 and -410 < rec[1]["dH"] < -400
    # the fifth is rejected on the uniform, not adapted: 0.514 against exp(-1.99) = 0.137
    assert -6 < rec[4]["dH"] < -1.9 and abs(rec[4]["uniform"] - 0.514) < 1e-3 and abs(math.exp(rec[4]["dH"]) - 0.137) < 1e-3
    assert 2 * 8 + 1 + 14 == 31                                             # reduction tasks of k_hmc_accept at L = 8: two trips of 16 waves
    rec = I.hmc_expected("adapt-five-times")["records"]
    assert [r["accepted"] for r in rec] == [True] + [False] * 5
    assert [r["L"] for r in rec] == [2, 2, 4, 7, 12, 20] and [r["L_new"] for r in rec] == [2, 4, 7, 12, 20, 32]
    assert all(r["dH"] < -6 for r in rec[1:]) and rec[-1]["eps_new"] == 0.1 / 32


def test_the_restore_cases_reject_their_third_iteration():
    for name in ("restore", "restore-transposed"):
        rec = I.hmc_expected(name)["records"]
        assert [r["accepted"] for r in rec] == [True, True, False]
        assert rec[2]["eps"] == I.RESTORE_EPS and rec[2]["dH"] < -6 and (rec[2]["eps_new"], rec[2]["L_new"]) == (I.RESTORE_EPS / 2, 4)
        st = I.hmc_expected(name)["state"]
        assert np.any(st.U != 0.0) and np.any(st.V != 0.0)                  # what is restored is not the zero start
