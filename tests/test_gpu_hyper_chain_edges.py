"""The one-launch chain of the hyperprior update (k_hyper_chain) as bdf_gibbs_sweep runs it: a native GibbsEngine over one
two-entity relation of a few thousand cells (most rows are sampled from the prior: the row launch is cheap), sweeps 1 and 2, and
after each everything the chain read and wrote, read back.  The cases (tests/hyper_edge_inputs.py: CHAIN_CASES) sit on the chain's
per-D cap of partial sums, on 13 and 16 chunks per workgroup, on the 16,384-row limit and one row past it, on the hand-over by
counter and by event; tests/test_hyper_edge_inputs_host.py pins them there.

  1  draws       == bdf_hyper_draws' bits (the chain's draw workgroups, k_hyper_draws_batch and k_hyper_draws are one function)
  2  sumU, UUt   within N 2^-52 sum |u u| of the long-double sums of the read-back rows; where the chain's partition is the unfused
                 one, bdf_hyper_sums' bits
  3  params, mu, Lambda, prior_pack == bdf_hyper_sample's bits from the engine's own sums and random part (the fused head against
                 the generic one)
  4  the same four within 1000 E_D of the restatement
  5  no flag: sync() raises on a spin bound or a refused pivot
"""
import numpy as np
import pytest

import hyper_edge_inputs as I
import hyper_restatement as R
from test_gpu_hyper_edges import _nan, _p, check_draw

pytestmark = pytest.mark.gpu


def _build(B, seed, D, Nu, Nv, feats):
    rng = np.random.default_rng(Nu + Nv)
    cells = rng.choice(Nu * Nv, size=I.CHAIN_CELLS, replace=False)
    ids = np.stack([cells // Nv + 1, cells % Nv + 1], axis=1).astype(np.int64)
    F = rng.standard_normal((Nu, I.CHAIN_FEATURES)) if feats else None
    u, v = B.Entity("u", F=F), B.Entity("v")
    rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": rng.standard_normal(I.CHAIN_CELLS)}, "r", [u, v], alpha=2.5, dims=[Nu, Nv])
    rd = B.RelationData()
    B.addRelation(rd, rel)
    return B.GibbsEngine(rd, D, seed=seed)


def _check_entity(ctx, eng, st, sweep, key):
    from bdf_amd._lib import check, lib
    L, D, N = lib(), eng.D, st.N
    assert N == st.n_real
    has_f = st.F is not None
    nu = st.nu0 + (st.numF if has_f and eng.full_lambda_u else 0)
    Tinv_t = st.Tinv if has_f and eng.full_lambda_u else st.WI
    host = {n: getattr(st, n).cpu().numpy() for n in ("draws", "sumU", "UUt", "params", "mu", "Lambda", "prior_pack", "mu0")}
    S, uh, Tinv = st.sample.cpu().numpy(), (st.uhat.cpu().numpy() if has_f else None), Tinv_t.cpu().numpy()
    ctx.set_sweep(sweep)
    # 1. the random part
    d_t = _nan(ctx, D * D + D)
    check(L.bdf_hyper_draws(ctx.handle, D, st.n_real, nu, st.tag, _p(d_t)))
    # 2. the sums on their own, from the same rows
    s_t, uu_t = _nan(ctx, D), _nan(ctx, D, D)
    check(L.bdf_hyper_sums(ctx.handle, D, N, _p(st.sample), _p(st.uhat) if has_f else None, _p(s_t), _p(uu_t)))
    # 3. the draw's kernel on its own, from the engine's sums and random part
    mu_t, Lam_t, par_t, pack_t = _nan(ctx, D), _nan(ctx, D, D), _nan(ctx, D + D * D), _nan(ctx, L.bdf_prior_pack_doubles(D))
    check(L.bdf_hyper_sample(ctx.handle, D, st.n_real, _p(st.sumU), _p(st.UUt), _p(st.mu0), st.b0, _p(Tinv_t), nu, st.tag, _p(mu_t), _p(Lam_t),
                             _p(par_t), _p(pack_t), _p(st.draws)))
    ctx.sync()
    assert d_t.cpu().numpy().tobytes() == host["draws"].tobytes(), (key, "draws")
    want_s, want_uu, b_s, b_uu = R.sums(S, uh)
    assert np.array_equal(host["UUt"], host["UUt"].T), key
    e_s, e_uu = np.abs(host["sumU"] - want_s).astype(float), np.abs(host["UUt"] - want_uu).astype(float)
    print("%s sums: worst |diff| / bound %.3f" % (key, max((e_s / b_s).max(), (e_uu / b_uu).max())))
    assert np.all(e_s <= b_s) and np.all(e_uu <= b_uu), key
    if R.chain_partition(D, N) == R.unfused_partition(N):
        assert s_t.cpu().numpy().tobytes() == host["sumU"].tobytes() and uu_t.cpu().numpy().tobytes() == host["UUt"].tobytes(), (key, "sums")
    for name, t in (("params", par_t), ("mu", mu_t), ("Lambda", Lam_t), ("prior_pack", pack_t)):
        assert t.cpu().numpy().tobytes() == host[name].tobytes(), (key, name)
    want = I.restated_draw(host["sumU"], host["UUt"], st.n_real, host["mu0"], st.b0, Tinv, nu, host["draws"])
    return check_draw(key, D, want, host["params"], host["Lambda"], host["mu"], host["prior_pack"], I.device_bound(D))


@pytest.mark.parametrize("name", list(I.CHAIN_CASES))
def test_chain_as_the_sweep_runs_it(B, ctx, monkeypatch, name):
    (D, Nu, Nv, feats, no_poll), _ = I.CHAIN_CASES[name]
    if no_poll:
        monkeypatch.setenv("BDF_NO_POLL", "1")
    eng = _build(B, ctx.seed, D, Nu, Nv, feats)
    try:
        assert eng.native and (eng.ent[0].F is not None) == feats
        worst = {}
        for sweep in (1, 2):
            eng.sweep(sweep)
            eng.sync()                                         # 5. raises if a flag was set
            for st, who in zip(eng.ent, "uv"):
                dist = _check_entity(ctx, eng, st, sweep, "%s sweep %d %s (D %d, %d rows)" % (name, sweep, who, D, st.N))
                worst = {k: max(x, worst.get(k, 0.0)) for k, x in dist.items()}
        print("%s worst: " % name + " ".join("%s %.2e" % kv for kv in worst.items()) + " bound %.2e" % I.device_bound(D))
    finally:
        eng.close()
