"""The spike-and-slab prior of an entity's rows without a GPU: the restated sweep leaves the exact
conditional of the inclusion pattern invariant, the restated hyper draw has the Beta and Gamma moments, the setter's guards, the
stream numbers in include/bdf.h, the new row kernel's resource usage, and the near-tie margins of the GPU tests' inputs."""
import glob
import itertools
import os
import re

import numpy as np
import pytest

import robust_restatement as RR
import spike_restatement as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- (a) the sweep leaves the exact conditional invariant ---------------------------------------------------------------------
def _pattern_masses(P, c, pi, tau):
    """mass of every inclusion pattern s of D = 3: prod pi_d^s_d (1 - pi_d)^(1 - s_d) sqrt(det diag(tau)_s / det P_ss)
    exp(c_s' P_ss^-1 c_s / 2), normalised; pattern s has index sum s_d 2^d"""
    D = len(c)
    mass = np.zeros(2 ** D)
    for bits in itertools.product((0, 1), repeat=D):
        s = np.array(bits, dtype=bool)
        m = np.prod(np.where(s, pi, 1.0 - pi))
        if s.any():
            Pss, cs = P[np.ix_(s, s)], c[s]
            m *= np.sqrt(np.prod(tau[s]) / np.linalg.det(Pss)) * np.exp(0.5 * cs @ np.linalg.solve(Pss, cs))
        mass[int(np.sum(s * 2 ** np.arange(D)))] = m
    return mass / mass.sum()


@pytest.mark.parametrize("corr", [0.05, 0.9])
def test_sweep_leaves_the_exact_conditional_invariant(corr):
    """D = 3, fixed (P, c, pi, tau): a chain of 200,000 restated sweeps, each from the output of the one before; every pattern's
    frequency within 5 binomial standard errors of its mass (the bound follows from the count).  P = diag(tau) + K with K's
    off-diagonal correlation `corr`: nearly diagonal, and strongly correlated."""
    n = 200_000
    rng = np.random.default_rng(11 if corr < 0.5 else 12)
    tau, pi = np.array([0.8, 1.5, 2.5]), np.array([0.3, 0.6, 0.45])
    sd = np.array([1.2, 0.9, 1.1])
    K = corr * np.outer(sd, sd)
    K[np.diag_indices(3)] = sd * sd
    P = np.diag(tau) + K
    c = np.array([0.9, -0.7, 0.5])
    state = np.stack([pi, tau, np.log(pi) - np.log1p(-pi), np.log(tau)])
    mass = _pattern_masses(P, c, pi, tau)
    Z, U = rng.standard_normal((n, 3)), rng.random((n, 3))
    u = np.zeros(3)
    hits = np.zeros(8)
    w = 2 ** np.arange(3)
    for t in range(n):
        u, _ = SR.sweep_row(P, c, u, Z[t], U[t], state)
        hits[int(np.sum((u != 0) * w))] += 1
    freq = hits / n
    se = np.sqrt(mass * (1.0 - mass) / n)
    print(f"corr {corr}: masses {np.round(mass, 4)}, worst deviation {np.max(np.abs(freq - mass) / se):.2f} standard errors")
    assert np.all(mass > 1e-3)
    assert np.all(np.abs(freq - mass) <= 5.0 * se), (freq, mass, se)


def test_the_two_restated_sweeps_and_row_systems_agree():
    """sweep_row (scalar) against sweep_rows (all rows at once), and row_systems against robust_restatement.row_system_terms"""
    rng = np.random.default_rng(3)
    N, D = 9, 6
    A = rng.standard_normal((N, D, D))
    P, c = A @ A.transpose(0, 2, 1) + np.eye(D), rng.standard_normal((N, D))
    u0, z, U = rng.standard_normal((N, D)) * (rng.random((N, D)) < 0.6), rng.standard_normal((N, D)), rng.random((N, D))
    st = SR.initial_state(D)
    st[2], st[3] = rng.standard_normal(D), np.log(st[1])
    u, margin = SR.sweep_rows(P, c, u0, z, U, st)
    m1 = np.inf
    for i in range(N):
        ui, mi = SR.sweep_row(P[i], c[i], u0[i], z[i], U[i], st)
        np.testing.assert_allclose(ui, u[i], rtol=1e-12, atol=1e-14)
        m1 = min(m1, mi)
    assert abs(m1 - margin) <= 1e-12 and np.any(u == 0) and np.any(u != 0)
    dims = [N, 7, 4]
    n = 80
    ids = np.stack([rng.integers(1, d + 1, n) for d in dims], axis=1)
    vals, w = rng.standard_normal(n), rng.random(n) + 0.5
    S = [rng.standard_normal((d, D)) for d in dims]
    terms = [(ids, vals, w, 0, 1.7, 0.2, S), (ids[:, :2], vals, None, 0, 0.4, 0.0, S[:2])]
    Lam = np.diag(rng.random(D) + 0.5)
    Pn, bn = SR.row_systems(terms, N, D, Lam, np.zeros(D))
    for i in range(N):
        Pi, bi = RR.row_system_terms(terms, i, np.zeros(D), Lam)
        np.testing.assert_allclose(Pn[i], Pi, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(bn[i], bi, rtol=1e-12, atol=1e-12)


# ---- (b) the hyper draw's moments ---------------------------------------------------------------------------------------------
def test_hyper_draw_moments():
    """20,000 restated draws (sweep numbers 1 .. 20,000) at fixed (n, q): the means of pi and tau within 5 standard errors of the
    means of Beta(a + n, b + N - n) and Gamma(shape + n / 2, rate + q / 2)"""
    draws, N = 20_000, 30
    n, q = np.array([0, 7, 30]), np.array([0.0, 5.5, 41.0])
    a, b, shape, rate = 1.0, 2.0, 0.5, 0.7
    out = np.stack([SR.hyper_draw_nq(n, q, N, a, b, shape, rate, 77, t, 3)[:2] for t in range(1, draws + 1)])
    A, Bb = a + n, b + (N - n)
    mean_pi, var_pi = A / (A + Bb), A * Bb / ((A + Bb) ** 2 * (A + Bb + 1.0))
    k, r = shape + 0.5 * n, rate + 0.5 * q
    mean_tau, var_tau = k / r, k / r ** 2
    dev_pi = np.abs(out[:, 0].mean(axis=0) - mean_pi) / np.sqrt(var_pi / draws)
    dev_tau = np.abs(out[:, 1].mean(axis=0) - mean_tau) / np.sqrt(var_tau / draws)
    print(f"hyper draw: deviations of the means in standard errors: pi {np.round(dev_pi, 2)}, tau {np.round(dev_tau, 2)}")
    assert np.all(dev_pi <= 5.0) and np.all(dev_tau <= 5.0)


# ---- (c) the setter's guards --------------------------------------------------------------------------------------------------
def _model(B, F=None):
    rng = np.random.default_rng(0)
    ids = np.stack([rng.integers(1, 21, 200), rng.integers(1, 11, 200)], axis=1)
    ids[:20, 0], ids[:10, 1] = np.arange(1, 21), np.arange(1, 11)
    ents = [B.Entity("u"), B.Entity("v", F=F)]
    rel = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": rng.standard_normal(200)}, "r", ents, dims=[20, 10])
    return ents, rel, B.RelationData(rel)


def test_setter_guards(B):
    ents, rel, rd = _model(B)
    assert ents[1].spike is None
    B.setSpikeAndSlab(ents[1])
    assert ents[1].spike == {"incl_a": 1.0, "incl_b": 1.0, "shape": 1.0, "rate": 1.0} and ents[0].spike is None
    B.setSpikeAndSlab(ents[0], incl_a=0.5, incl_b=3, shape=2.5, rate=1e-3)
    assert ents[0].spike == {"incl_a": 0.5, "incl_b": 3.0, "shape": 2.5, "rate": 1e-3}
    for name in ("incl_a", "incl_b", "shape"):
        for bad in (0.49, -1.0, float("inf"), float("nan"), "1", True):
            with pytest.raises(B.ArgumentError, match=rf"Entity v: {name} = .* must be a finite number, at least 0\.5 \(setSpikeAndSlab\)"):
                B.setSpikeAndSlab(ents[1], **{name: bad})
    for bad in (0.0, -2.0, float("inf"), float("nan"), None):
        with pytest.raises(B.ArgumentError, match=r"Entity v: rate = .* must be a finite number above 0 \(setSpikeAndSlab\)"):
            B.setSpikeAndSlab(ents[1], rate=bad)
    with pytest.raises(B.ArgumentError, match="setSpikeAndSlab takes an Entity"):
        B.setSpikeAndSlab("v")
    # no side information on the entity
    fents, frel, frd = _model(B, F=np.ones((10, 2)))
    with pytest.raises(B.ArgumentError, match=r"Entity v has features: the spike-and-slab prior \(setSpikeAndSlab\) does not take side information"):
        B.setSpikeAndSlab(fents[1])
    assert fents[1].spike is None                     # a refused call leaves the entity as it was
    from bdf_amd._two_mode import relation_of
    relation_of(frd, 4, "bpmf_vb")                    # ... so the trainers that refuse the prior still take the data
    B.setSpikeAndSlab(fents[0])                       # ... the other entity may have it
    # no background on the entity's relations
    bents, brel, brd = _model(B)
    ids = np.unique(np.asarray(brel.data.ids), axis=0)
    brel2 = B.Relation({"u": ids[:, 0], "v": ids[:, 1], "y": np.ones(len(ids))}, "b", [B.Entity("u"), B.Entity("v")], dims=[20, 10])
    brd2 = B.RelationData(brel2)
    B.setBackground(brel2, 0.1)
    with pytest.raises(B.ArgumentError, match=r"Relation b has a background \(setBackground\): its entity v does not take the spike-and-slab prior"):
        B.setSpikeAndSlab(brel2.entities[1])
    assert brel2.entities[1].spike is None
    # ... checked again when a sampler is built (the background may come after the setter), and one rank only
    from bdf_amd.relation_data import check_spike
    B.setSpikeAndSlab(ents[1])
    check_spike(ents[1])
    with pytest.raises(B.ArgumentError, match=r"Entity v has the spike-and-slab prior \(setSpikeAndSlab\): one rank only"):
        check_spike(ents[1], world=2)
    ents[1].spike["shape"] = 0.1
    with pytest.raises(B.ArgumentError, match="shape = 0.1"):
        check_spike(ents[1])
    # the two-mode trainers refuse it
    ents[1].spike["shape"] = 1.0
    for who in ("bpmf_vb", "macau_hmc"):
        with pytest.raises(B.ArgumentError, match=rf"{who} has the Normal-Wishart prior only; . has the spike-and-slab prior"):
            relation_of(rd, 4, who)
    assert B.toStr(ents[1]) == "v[]"                   # no model yet: what it was


# ---- (d) the stream numbers ---------------------------------------------------------------------------------------------------
def test_stream_numbers_in_the_header(B):
    h = open(os.path.join(ROOT, "include", "bdf.h")).read()
    got = {name: int(v) for name, v in re.findall(r"#define (BDF_P_SPIKE\w*)\s+(\d+)", h)}
    assert got == {"BDF_P_SPIKE_N": 21, "BDF_P_SPIKE_U": 22, "BDF_P_SPIKE": 23}
    from bdf_amd import _lib
    assert (_lib.P_SPIKE_N, _lib.P_SPIKE_U, _lib.P_SPIKE) == (21, 22, 23) == (SR.P_SPIKE_N, SR.P_SPIKE_U, SR.P_SPIKE)
    every = [int(v) for v in re.findall(r"#define BDF_P_\w+\s+(\d+)", h)]
    assert len(every) == len(set(every))               # no stream number is used twice


# ---- (e) the new row kernel's resource usage ----------------------------------------------------------------------------------
def test_row_kernel_uses_no_scratch():
    """every instantiation of k_rows_ss in the build's csrc/*.o.res: DP in {16, 32, 64}, weighted and not -- no scratch, no spill"""
    res, name = {}, None
    for f in glob.glob(os.path.join(ROOT, "bayesiandatafusion.jl_amd", "csrc", "*.o.res")):
        for line in open(f):
            m = re.search(r"remark: \s*(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill|Occupancy \[waves/SIMD\]): (\S+)", line)
            if not m:
                continue
            if m.group(1) == "Function Name":
                name = m.group(2)
                res[name] = {}
            elif name is not None:
                res[name][m.group(1)] = int(m.group(2))
    assert res, "no csrc/*.o.res: build with __graft_entry__.build() (make)"
    ss = {k: v for k, v in res.items() if "9k_rows_ssILi" in k}
    want = {"_ZN12_GLOBAL__N_19k_rows_ssILi%dELb%dEEEv10SampleArgs7PlanDev" % (dp, w) for dp in (16, 32, 64) for w in (0, 1)}
    assert set(ss) == want, sorted(ss)
    for k, v in ss.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["VGPRs"] <= 256, (k, v)
        print(k, v)


# ---- (f) the GPU tests' inputs: no decision near a tie ------------------------------------------------------------------------
def test_near_tie_margins_of_the_gpu_inputs(O):
    """tests/test_gpu_spike.py holds the device to the restatement's inclusion pattern when no decision is nearer a tie than 1e-9:
    checked here for every row case (numpy row systems, the oracle's streams) and every whole-iteration model"""
    worst = np.inf
    for D, n_modes, mode, variant in SR.row_cases():
        u, margin = SR.row_case_reference(SR.row_case(D, n_modes, mode, variant), D, mode)
        assert margin >= 1e-9, (D, n_modes, mode, variant, margin)
        assert np.any(u == 0) and np.any(u != 0)
        worst = min(worst, margin)
    for name in SR.CHAIN_MODELS:
        dims, rels, spike, feats, n_test = SR.chain_model(name)
        train = [dict(r, ids=r["ids"][n_test:], values=r["values"][n_test:]) if i == 0 else r for i, r in enumerate(rels)]
        out = SR.run_chain(train, dims, SR.CHAIN_D, SR.CHAIN_SEED, 6, spike, feats=feats, burnin=3)
        assert out["margin"] >= 1e-9, (name, out["margin"])
        worst = min(worst, out["margin"])
    print(f"smallest near-tie margin of the GPU tests' inputs: {worst:.3e}")
