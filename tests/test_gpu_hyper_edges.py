"""The hyperprior kernels (K6: csrc/k_hyper.hip, csrc/hyper_job.h) through their public entry points, at the edges of their three
widths, the 4-row step, the 128-row chunk, the 16 chains of the final sum and the chunk loops of a workgroup, against the long-double
restatement (tests/hyper_restatement.py).  The cases are tests/hyper_edge_inputs.py's; tests/test_hyper_edge_inputs_host.py pins them
to their edges and measures E_D, the double-precision oracle's own distance from the restatement, without a GPU.

  sums      |got - ref| <= N 2^-52 sum_k |u_ki u_kj| per element (any order of a double-precision sum), exact symmetry, NaN rows behind
            the entity's never read, every output element written
  draw      mu_N, the whole W, Lambda and mu within 1000 E_D of the restatement run on the device's own sums and random part; the
            pack's image exactly that of the returned Lambda
  draws     the indexing of (row, entry, purpose, tag) against the oracle's streams
The one-launch chain of the native sweep is tests/test_gpu_hyper_chain_edges.py's.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import hyper_edge_inputs as I
import hyper_restatement as R

pytestmark = pytest.mark.gpu

SWEEP, TAG = 12, 5
ERR_ARG = -1


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _nan(ctx, *shape):
    """an output buffer of NaN: every element must be overwritten"""
    with torch.cuda.stream(ctx.stream):
        return torch.full(shape, float("nan"), dtype=torch.float64, device=ctx.device)


def _padded(ctx, a, N, D):
    """a's N rows on the device with HS_ROWS rows of NaN behind them (N = 0: a live buffer all the same)"""
    buf = np.full((N + R.HS_ROWS, D), np.nan)
    buf[:N] = a
    return ctx.tensor(buf)


def _device_sums(ctx, D, N, S, uh):
    from bdf_amd._lib import check, lib
    S_t = _padded(ctx, S, N, D)
    uh_t = _padded(ctx, uh, N, D) if uh is not None else None
    sumU, UUt = _nan(ctx, D), _nan(ctx, D, D)
    check(lib().bdf_hyper_sums(ctx.handle, D, N, _p(S_t), _p(uh_t), _p(sumU), _p(UUt)))
    ctx.sync()
    return sumU, UUt


def _check_sums(key, sumU, UUt, S, uh):
    want_s, want_uu, b_s, b_uu = R.sums(S, uh)
    got_s, got_uu = sumU.cpu().numpy(), UUt.cpu().numpy()
    assert not np.isnan(got_s).any() and not np.isnan(got_uu).any(), key
    assert np.array_equal(got_uu, got_uu.T), key
    e_s, e_uu = np.abs(got_s - want_s).astype(float), np.abs(got_uu - want_uu).astype(float)
    with np.errstate(invalid="ignore", divide="ignore"):
        worst = max(np.nanmax(e_s / b_s, initial=0.0), np.nanmax(e_uu / b_uu, initial=0.0))
    print("%s sums: worst |diff| / bound %.3f" % (key, worst))
    assert np.all(e_s <= b_s) and np.all(e_uu <= b_uu), (key, worst)


# ---- a. sums at the width and row edges ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", I.WIDTHS_D)
def test_sums_at_the_row_edges(ctx, D):
    for N in I.SUMS_ROWS:
        S, uh = I.sums_inputs(D, N, True)
        for with_uhat in (False, True):
            sumU, UUt = _device_sums(ctx, D, N, S, uh if with_uhat else None)
            _check_sums("D %d N %d uhat %d" % (D, N, with_uhat), sumU, UUt, S, uh if with_uhat else None)


@pytest.mark.parametrize("D", I.WIDTHS_D)
def test_sums_of_no_rows(ctx, D):
    """N = 0 with a live buffer of NaN (the masked lanes read element 0): exact zeros; a NULL sample is refused before any launch"""
    from bdf_amd._lib import lib
    for with_uhat in (False, True):
        sumU, UUt = _device_sums(ctx, D, 0, np.zeros((0, D)), np.zeros((0, D)) if with_uhat else None)
        got_s, got_uu = sumU.cpu().numpy(), UUt.cpu().numpy()
        assert not got_s.any() and not got_uu.any() and not np.isnan(got_s).any() and not np.isnan(got_uu).any()
    sumU, UUt = _nan(ctx, D), _nan(ctx, D, D)
    assert lib().bdf_hyper_sums(ctx.handle, D, 0, None, None, _p(sumU), _p(UUt)) == ERR_ARG
    assert lib().bdf_hyper_sums(ctx.handle, D, 5, None, None, _p(sumU), _p(UUt)) == ERR_ARG
    ctx.sync()
    assert np.isnan(sumU.cpu().numpy()).all() and np.isnan(UUt.cpu().numpy()).all()


# ---- b. several chunks per workgroup ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,N,with_uhat", sorted(I.SUMS_LARGE))
def test_sums_with_several_chunks_per_workgroup(ctx, D, N, with_uhat):
    S, uh = I.sums_inputs(D, N, with_uhat)
    sumU, UUt = _device_sums(ctx, D, N, S, uh)
    _check_sums("D %d N %d: %s" % (D, N, I.SUMS_LARGE[D, N, with_uhat][0]), sumU, UUt, S, uh)


# ---- c. the random part -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,N,nu", I.DRAWS_CASES)
def test_random_part_against_the_oracle_streams(ctx, D, N, nu):
    from bdf_amd._lib import check, lib
    total, guard = D * D + D, 64
    out = _nan(ctx, total + guard)
    ctx.set_sweep(SWEEP)
    check(lib().bdf_hyper_draws(ctx.handle, D, N, nu, TAG, _p(out)))
    ctx.sync()
    got = out.cpu().numpy()
    assert not np.isnan(got[:total]).any() and np.isnan(got[total:]).all()      # all of it and nothing behind it
    A = got[:D * D].reshape(D, D)
    assert not np.triu(A, 1).any() and np.all(np.diag(A) > 0)
    np.testing.assert_allclose(got[:total], R.draws(D, nu + N, ctx.seed, SWEEP, TAG), rtol=1e-7, atol=1e-9)


# ---- d. the draw at every width ---------------------------------------------------------------------------------------------------
def _device_draw(ctx, D, N, sumU, UUt, mu0, b0, Tinv, nu, draws_t):
    """bdf_hyper_sample into NaN-filled buffers -> params, Lambda, mu, pack (numpy)"""
    from bdf_amd._lib import check, lib
    mu_t, Lam_t, par_t, pack_t = _nan(ctx, D), _nan(ctx, D, D), _nan(ctx, D + D * D), _nan(ctx, lib().bdf_prior_pack_doubles(D))
    mu0_t, Tinv_t = ctx.tensor(mu0), ctx.tensor(Tinv)
    ctx.set_sweep(SWEEP)
    check(lib().bdf_hyper_sample(ctx.handle, D, N, _p(sumU), _p(UUt), _p(mu0_t), b0, _p(Tinv_t), nu, TAG, _p(mu_t), _p(Lam_t), _p(par_t),
                                 _p(pack_t), _p(draws_t)))
    ctx.sync()
    return tuple(t.cpu().numpy() for t in (par_t, Lam_t, mu_t, pack_t))


def check_draw(key, D, want, par, Lam, mu, pack, bound):
    """the draw's four outputs against the restatement `want` (hyper_edge_inputs.restated_draw), each distance printed"""
    for a in (par, Lam, mu, pack):
        assert not np.isnan(a).any(), key
    W = par[D:].reshape(D, D)
    assert np.array_equal(Lam, Lam.T), key
    dist = {"mu_N": I.rel_distance(par[:D], want["mu_N"], 1.0), "W": I.rel_distance(W, want["W"]),
            "Lambda": I.rel_distance(Lam, want["Lambda"]), "mu": I.rel_distance(mu, want["mu"], 1.0)}
    print("%s draw: " % key + " ".join("%s %.2e" % kv for kv in dist.items()) + " bound %.2e" % bound)
    assert len(pack) == R.pack_doubles(D)
    np.testing.assert_allclose(pack[:D], Lam @ mu, rtol=1e-12, atol=1e-12)
    assert np.array_equal(pack[D:], R.pack_image(Lam, mu, D)[D:]), key
    for name, d in dist.items():
        assert d <= bound, (key, name, d, bound)
    return dist


@pytest.mark.parametrize("D", I.WIDTHS_D)
def test_draw_from_the_devices_own_sums_and_random_part(ctx, D):
    from bdf_amd._lib import check, lib
    worst = {}
    for N in I.DRAW_ROWS:
        S, mu0, Tinv, b0, nu = I.draw_inputs(D, N)
        sumU, UUt = _device_sums(ctx, D, N, S, None)
        draws_t = _nan(ctx, D * D + D)
        ctx.set_sweep(SWEEP)
        check(lib().bdf_hyper_draws(ctx.handle, D, N, nu, TAG, _p(draws_t)))
        ahead = _device_draw(ctx, D, N, sumU, UUt, mu0, b0, Tinv, nu, draws_t)
        want = I.restated_draw(sumU.cpu().numpy(), UUt.cpu().numpy(), N, mu0, b0, Tinv, nu, draws_t.cpu().numpy())
        dist = check_draw("D %d N %d" % (D, N), D, want, *ahead, I.device_bound(D))
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in dist.items()}
        # the random part made inside the call: the same bits
        inside = _device_draw(ctx, D, N, sumU, UUt, mu0, b0, Tinv, nu, None)
        for a, b in zip(ahead, inside):
            assert a.tobytes() == b.tobytes()
    print("D %d worst: " % D + " ".join("%s %.2e" % kv for kv in worst.items()) + " E_D %.2e bound %.2e" % (I.E(D), I.device_bound(D)))


# ---- e. the reference's mean map (BDF_HYPER_MEAN=reference is read once per process: a fresh child) --------------------------------
MEAN_REF_CHILD = r"""
import ctypes as C, sys
import numpy as np
import os
out, tests_dir = sys.argv[1], sys.argv[2]
sys.path[:0] = [tests_dir, os.path.dirname(tests_dir)]
import bdf_amd as B
from bdf_amd._lib import check, lib
import hyper_edge_inputs as I
p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
ctx = B.Context(seed=1234)
res = {}
for D in I.MEAN_REF_D:
    N = 129
    S, mu0, Tinv, b0, nu = I.draw_inputs(D, N)
    S_t, mu0_t, Tinv_t = ctx.tensor(S), ctx.tensor(mu0), ctx.tensor(Tinv)
    sumU, UUt, draws = ctx.zeros(D), ctx.zeros(D, D), ctx.zeros(D * D + D)
    mu, Lam, par, pack = ctx.zeros(D), ctx.zeros(D, D), ctx.zeros(D + D * D), ctx.zeros(lib().bdf_prior_pack_doubles(D))
    ctx.set_sweep(12)
    check(lib().bdf_hyper_sums(ctx.handle, D, N, p(S_t), None, p(sumU), p(UUt)))
    check(lib().bdf_hyper_draws(ctx.handle, D, N, nu, 5, p(draws)))
    check(lib().bdf_hyper_sample(ctx.handle, D, N, p(sumU), p(UUt), p(mu0_t), b0, p(Tinv_t), nu, 5, p(mu), p(Lam), p(par), p(pack), p(draws)))
    ctx.sync()
    for name, t in (("sumU", sumU), ("UUt", UUt), ("draws", draws), ("mu", mu), ("Lambda", Lam), ("params", par), ("pack", pack)):
        res["%s_%d" % (name, D)] = t.cpu().numpy()
ctx.close()
np.savez(out, **res)
"""


def test_reference_mean_map_in_a_fresh_process(ctx, monkeypatch):
    import os
    from both_paths import child
    monkeypatch.setenv("BDF_HYPER_MEAN", "reference")
    got = child(MEAN_REF_CHILD, os.path.dirname(os.path.abspath(__file__)), no_native=False)
    monkeypatch.delenv("BDF_HYPER_MEAN")
    for D in I.MEAN_REF_D:
        N = 129
        S, mu0, Tinv, b0, nu = I.draw_inputs(D, N)
        g = {k: got["%s_%d" % (k, D)] for k in ("sumU", "UUt", "draws", "mu", "Lambda", "params", "pack")}
        want = I.restated_draw(g["sumU"], g["UUt"], N, mu0, b0, Tinv, nu, g["draws"], "reference")
        check_draw("reference map D %d" % D, D, want, g["params"], g["Lambda"], g["mu"], g["pack"], I.device_bound(D))
        # this process draws by the default map: the same Lambda from the same sums and random part, another mean
        par, Lam, mu, pack = _device_draw(ctx, D, N, ctx.tensor(g["sumU"]), ctx.tensor(g["UUt"]), mu0, b0, Tinv, nu, ctx.tensor(g["draws"]))
        assert Lam.tobytes() == g["Lambda"].tobytes() and par.tobytes() == g["params"].tobytes()
        default = I.restated_draw(g["sumU"], g["UUt"], N, mu0, b0, Tinv, nu, g["draws"], "factor")
        assert I.rel_distance(mu, default["mu"], 1.0) <= I.device_bound(D)
        # (the two maps are different functions of the same normals: they lie far further apart than the bound can blur)
        assert not np.any(mu == g["mu"]) and I.rel_distance(g["mu"], default["mu"], 1.0) > 1e3 * I.device_bound(D)
