"""macau_hmc at the edges of its kernels (csrc/k_hmc.hip, csrc/bdf_hmc.hip) against the row-by-row numpy restatement
(tests/hmc_restatement.py): every iteration's record through the C ABI, one iteration at a time, then the final state by
tests/test_gpu_hmc.py's _compare at 1e-9.  The inputs and the restatement's runs are tests/two_mode_edge_inputs.py's;
tests/test_two_mode_edge_inputs_host.py asserts their degrees, block counts, duplicates, accept / reject sequences and Metropolis
margins without a GPU.

  k_hmc_leap's neighbour loop    degrees 0, 1, 2, NG - 1, NG, NG + 1 (groups without a neighbour), P - 1, P, P + 1, 2P + 1, Nv - 1 around
                                 the pass of P = 4 NG neighbours, duplicates on the last neighbour and the first of the second pass,
                                 D = 16, 17, 32, 33, 63: test_degree_ladder (the long rows on V: the transposed case)
  k_hmc_accept's block loop      70 and 140 blocks per launch: test_degree_ladder; 31 reduction tasks (L = 8), 55 (L = 20): the adaptation tests
  k_hmc_predict, bdf_hmc_stats   257 test pairs (test_degree_ladder), 600 through the copy phase into the running mean (test_prediction_blocks)
  k_hmc_restore                  1,120 and 2,240 doubles, either entity the longer one: test_restore_past_one_block
  hmc_reserve, hmc_settle        L 3 -> 5 -> 8 and three kinds of iteration after it; L 2 -> 4 -> 7 -> 12 -> 20: the adaptation tests
  L = 1, L_inner > 1             test_steps_and_inner_steps
  HMC_FLAG_ENERGY                test_a_non_finite_energy_is_reported
"""
import ctypes as C
import types

import numpy as np
import pytest

import two_mode_edge_inputs as I
import vb_restatement as R
from test_gpu_hmc import _compare

pytestmark = pytest.mark.gpu

LOG_CAP = 2 * 32 + 1 + 4                   # room for the momentum log of L = 32, and a few doubles that must stay NaN


def _drive(B, name):
    """the scenario `name` through bdf_hmc_*, one iteration at a time -> (per iteration: (stats, momentum log, U, V)), out, where
    out is what macau_hmc returns of the final state (for _compare)"""
    from bdf_amd import _lib, _two_mode
    lib, check = _lib.lib(), _lib.check
    case, Nu, Nv, D, seed, kw = I.hmc_scenarios()[name]
    rd = R.relation_data(B, case, Nu, Nv)
    lo, hi = _two_mode.clamp_bounds(kw["clamp"])
    phases = kw.get("phases", {})
    N = (Nu, Nv)
    its = []
    with _two_mode.trainer(rd, D, lib.bdf_hmc_create, lib.bdf_hmc_destroy, (2.0,), seed=seed, device=None) as (h, test):
        check(lib.bdf_hmc_set_test(h, test, lo, hi))
        check(lib.bdf_hmc_set_params(h, kw["L"], kw["L_inner"], kw["prior_freq"], kw["eps"], kw["burnin"]))
        for i in range(1, kw["burnin"] + kw["psamples"] + 1):
            if i in phases:
                check(lib.bdf_hmc_set_params(h, phases[i][1], kw["L_inner"], kw["prior_freq"], phases[i][0], kw["burnin"]))
            check(lib.bdf_hmc_iterate(h, 1))
            st, log = np.zeros(16), np.zeros(LOG_CAP)
            check(lib.bdf_hmc_stats(h, st.ctypes.data_as(_lib.c_dp), log.ctypes.data_as(_lib.c_dp), LOG_CAP))
            S = [np.empty((n, D)) for n in N]
            for e in range(2):
                check(lib.bdf_hmc_model(h, e, S[e].ctypes.data_as(_lib.c_dp), None, None, None))
            its.append((st, log, S[0], S[1]))
        out = {"accepted": [bool(st[8] != 0.0) for st, *_ in its], "eps": float(its[-1][0][9]), "L": int(its[-1][0][10]),
               "rmse": float(its[-1][0][14]), "rmse_avg": float(its[-1][0][15]), "mu": [], "Lambda": []}
        for e in range(2):
            samp, mom, mu, Lam = np.empty((N[e], D)), np.empty((N[e], D)), np.empty(D), np.empty((D, D))
            check(lib.bdf_hmc_model(h, e, samp.ctypes.data_as(_lib.c_dp), mom.ctypes.data_as(_lib.c_dp), mu.ctypes.data_as(_lib.c_dp),
                                    Lam.ctypes.data_as(_lib.c_dp)))
            out["UV"[e] + "sample"] = samp.T
            out["UV"[e] + "model"] = types.SimpleNamespace(momentum=mom.T)
            out["mu"].append(mu)
            out["Lambda"].append(Lam.T)
    return its, out


def _expected_log(r):
    """the momentum log of an iteration, in launch order U0, V1, U2, ..., V(2L-1), U(2L), from the restatement's record"""
    L = r["L"]
    log = np.zeros(2 * L + 1)
    log[0] = r["norm0"]
    for l in range(1, L + 1):
        log[2 * l - 1] = r["norms"][l - 1][1]
        if l < L:
            log[2 * l] = r["norms"][l - 1][0]
    log[2 * L] = r["norms"][L][0]
    assert L > 1 or r["norms"][0][0] == r["norm0"]                # at L = 1 the reference prints launch 0's norm itself
    return log


def _close(got, want, tol):
    return abs(got - want) <= tol * abs(want)


def _compare_records(name, its, exp):
    assert len(its) == len(exp["records"])
    for i, ((st, log, _, _), r) in enumerate(zip(its, exp["records"]), 1):
        where = (name, "iteration %d" % i)
        L = r["L"]
        assert st[0] == i, where
        got = (st[1], st[2], st[8] != 0.0, st[9], st[10])
        assert got == (r["eps"], L, r["accepted"], r["eps_new"], r["L_new"]), (where, got, r)
        for k, f in ((3, "kin_s"), (4, "kin_f"), (5, "pot_s"), (6, "pot_f")):
            print(name, i, f, "%.3e" % (abs(st[k] - r[f]) / abs(r[f])))
            assert _close(st[k], r[f], 1e-9), (where, f, st[k], r[f])
        scale = abs(r["kin_s"]) + abs(r["kin_f"]) + abs(r["pot_s"]) + abs(r["pot_f"])
        print(name, i, "dH", "%.3e" % (abs(st[7] - r["dH"]) / scale))
        assert abs(st[7] - r["dH"]) <= 1e-9 * scale, (where, "dH", st[7], r["dH"])
        want = _expected_log(r)
        for s in range(2 * L + 1):
            assert _close(log[s], want[s], 1e-9), (where, "momentum norm of launch %d" % s, log[s], want[s])
        assert np.all(np.isnan(log[2 * L + 1:])), where
        for k, f in ((11, "normU"), (12, "normV")):
            assert _close(st[k], r[f], 1e-9), (where, f, st[k], r[f])
        for k, f in ((14, "rmse"), (15, "rmse_avg")):
            print(name, i, f, "%.3e" % abs(st[k] - r[f]))
            assert abs(st[k] - r[f]) < 1e-9, (where, f, st[k], r[f])


def _rejections_restore_the_bits(its, N, D):
    """after every rejected iteration both samples are the previous iteration's (the zero start before the first), bit for bit"""
    prev = [np.zeros((n, D)) for n in N]
    rejected = 0
    for i, (st, _, U, V) in enumerate(its, 1):
        if st[8] == 0.0:
            rejected += 1
            assert np.array_equal(U, prev[0]) and np.array_equal(V, prev[1]), i
        else:
            assert not np.array_equal(U, prev[0]) and not np.array_equal(V, prev[1]), i
        prev = [U, V]
    return rejected


def _run(B, name):
    its, out = _drive(B, name)
    exp = I.hmc_expected(name)
    _compare_records(name, its, exp)
    _compare(out, exp, 1e-9)
    return its, exp


@pytest.mark.parametrize("D", list(I.HMC_LADDER_EPS))
def test_degree_ladder(B, D):
    _run(B, "ladder-%d" % D)


def test_degree_ladder_on_the_second_entity(B):
    """the long rows are V's: their launches carry no data term, and V is the shorter entity in the restore launch"""
    _run(B, "ladder-%d-transposed" % I.HMC_LADDER_TRANSPOSED_D)


@pytest.mark.parametrize("L,L_inner", I.HMC_L_CASES)
def test_steps_and_inner_steps(B, L, L_inner):
    """at L = 1 launch 1 (V) both draws the momentum and sums the final energies; L_inner > 1 at D = 17"""
    _run(B, "steps-%d-%d" % (L, L_inner))


def test_prediction_blocks(B):
    """600 test pairs in three blocks, unclamped: rmse and rmse_avg of every iteration, two that copy and four that average"""
    its, exp = _run(B, "predict")
    assert len(its) == 6 and any(abs(st[14] - st[15]) > 1e-6 for st, *_ in its[3:])


def test_adaptation_then_onward(B):
    """two adapting rejections (L 3 -> 5 -> 8: the partial sums and the record grow twice), then two accepts, a rejection on the
    uniform without adaptation and an accept, all with the adapted eps and L"""
    its, exp = _run(B, "adapt-then-onward")
    assert [int(st[10]) for st, *_ in its] == [5, 8, 8, 8, 8, 8]
    assert _rejections_restore_the_bits(its, I.ADAPT_SHAPE, I.ADAPT_D) == 3


def test_adaptation_five_times(B):
    """one accept, then five adapting rejections, L = 2, 4, 7, 12, 20: after each the samples are the accepted ones bit for bit"""
    its, exp = _run(B, "adapt-five-times")
    assert [int(st[2]) for st, *_ in its] == [2, 2, 4, 7, 12, 20]
    assert _rejections_restore_the_bits(its, I.ADAPT_SHAPE, I.ADAPT_D) == 5
    assert np.array_equal(its[-1][2], its[0][2]) and np.array_equal(its[-1][3], its[0][3]) and np.any(its[0][2] != 0.0)


@pytest.mark.parametrize("name", ["restore", "restore-transposed"])
def test_restore_past_one_block(B, name):
    """two accepted iterations, then one at eps = 0.3 (dH < -6): both samples, 70 x 16 and 140 x 16 doubles, five and nine blocks of
    the restore launch, are those before it bit for bit (the momenta are the rejected trajectory's and are compared as such)"""
    its, exp = _run(B, name)
    Nu, Nv = I.hmc_scenarios()[name][1:3]
    assert its[2][0][7] < -6.0 and its[2][0][8] == 0.0
    assert _rejections_restore_the_bits(its, (Nu, Nv), 16) == 1


def test_a_non_finite_energy_is_reported(B):
    """eps = 1e200 is finite and positive, so bdf_hmc_set_params takes it; the energies overflow, the accept kernel raises the
    flag, the next bdf_hmc_stats returns the error, and the trainer and the context then close"""
    from bdf_amd import _lib, _two_mode
    lib, check = _lib.lib(), _lib.check
    Nu, Nv, D = 20, 15, 3
    rd = R.relation_data(B, R.make_case(Nu, Nv, 120, seed=6, ntest=10), Nu, Nv)
    ctx = B.Context(seed=1)
    h = C.c_void_p()
    try:
        check(lib.bdf_hmc_create(ctx.handle, D, *_two_mode.create_args(rd), 2.0, C.byref(h)))
        check(lib.bdf_hmc_set_params(h, 2, 1, 1000, 1e200, 0))
        check(lib.bdf_hmc_iterate(h, 1))
        st = np.zeros(16)
        with pytest.raises(_lib.NotPositiveDefinite, match="energy"):
            check(lib.bdf_hmc_stats(h, st.ctypes.data_as(_lib.c_dp), None, 0))
        ctx.sync()                                                  # the flag is reported once
        check(lib.bdf_hmc_stats(h, st.ctypes.data_as(_lib.c_dp), None, 0))
        assert st[0] == 1 and st[8] == 0.0 and not np.isfinite(st[7])
        S = np.ones((Nu, D))
        check(lib.bdf_hmc_model(h, 0, S.ctypes.data_as(_lib.c_dp), None, None, None))
        assert not S.any()                                          # rejected: the sample is the zero start again
    finally:
        rc = lib.bdf_hmc_destroy(h) if h else 0
        ctx.close()
    assert rc == 0 and not ctx.handle
