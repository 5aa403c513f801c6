"""Hamiltonian Monte Carlo BPMF: macau_hmc and HMCModel (src/macau_hmc.jl).

HMCModel is the reference's host-side model (momentum and the diagonal mass G, both D x N).  macau_hmc runs the iterations on
the device through the library's bdf_hmc_* entry points (csrc/bdf_hmc.hip, csrc/k_hmc.hip) and returns host copies.  One
GPU, one two-mode relation without side information: HMC on several GPUs, on tensors or with features is out of scope.
"""
import math
import time

import numpy as np

from . import _lib, _two_mode
from ._lib import ArgumentError, check, lib
from .relation_data import hasFeatures


class HMCModel:
    """HMCModel(num_latent, N, Ldiag) (macau_hmc.jl:13-18): momentum zeros(D, N), G = repmat(Ldiag, 1, N)."""

    def __init__(self, num_latent, N, Ldiag):
        D, N = int(num_latent), int(N)
        Ldiag = np.asarray(Ldiag, dtype=np.float64).reshape(-1)
        if len(Ldiag) != D:
            raise ArgumentError(f"Ldiag has {len(Ldiag)} entries, num_latent is {D}")
        self.momentum = np.zeros((D, N))
        self.G = np.tile(Ldiag[:, None], (1, N))

    def __repr__(self):
        return "HMCModel of %d instances: |momentum|=%0.3e" % (self.momentum.shape[1], np.linalg.norm(self.momentum))


def _check_args(data, num_latent, L, L_inner, prior_freq, eps, burnin, psamples, reset_model, clamp):
    """every ArgumentError macau_hmc raises, before any device is touched"""
    D, rel = _two_mode.relation_of(data, num_latent, "macau_hmc")
    if any(hasFeatures(en) for en in rel.entities) or hasFeatures(rel):
        raise ArgumentError("macau_hmc does not use side information: the relation or its entities have features")
    for name, v in (("L", L), ("L_inner", L_inner), ("prior_freq", prior_freq)):
        if int(v) != v or int(v) < 1:
            raise ArgumentError(f"{name}={v} must be an integer of at least 1")
    if not (isinstance(eps, (int, float, np.floating)) and math.isfinite(eps) and eps > 0):
        raise ArgumentError(f"eps={eps} must be positive and finite")
    for name, v in (("burnin", burnin), ("psamples", psamples)):
        if int(v) != v or int(v) < 0:
            raise ArgumentError(f"{name}={v} must be a non-negative integer")
    if not reset_model:
        raise ArgumentError("macau_hmc starts from reset!: reset_model=false (a model carried over from an earlier run) is "
                            "not supported")
    return D, rel, _two_mode.clamp_bounds(clamp)


def macau_hmc(data, num_latent=10, verbose=True, burnin=100, psamples=100, L=10, L_inner=1, prior_freq=8, eps=0.01,
              reset_model=True, clamp=(), seed=0, device=None):
    """macau_hmc(data; num_latent=10, verbose=true, burnin=100, psamples=100, L=10, L_inner=1, prior_freq=8, eps=0.01,
    reset_model=true, clamp=Float64[]) (macau_hmc.jl:20-137) on the device.

    Uses data.relations[0] only; its precision alpha is fixed.  seed keys the Philox streams of the momenta, the Metropolis
    uniforms and the prior draws.  Returns the reference's {"rmse", "rmse_train" (NaN), "alpha"} and "rmse_avg", the final
    "eps" and "L", "accepted" (one bool per iteration), "Usample" / "Vsample" (D x N), "Umodel" / "Vmodel" (HMCModel) and
    "mu" / "Lambda" (one per entity)."""
    D, rel, (lo, hi) = _check_args(data, num_latent, L, L_inner, prior_freq, eps, burnin, psamples, reset_model, clamp)
    L, L_inner, prior_freq, burnin, psamples, eps = int(L), int(L_inner), int(prior_freq), int(burnin), int(psamples), float(eps)
    verbose and print("Model setup")
    N = [data.entities[0].count, data.entities[1].count]
    # reset!: Lambda = 5 I, so G = 5 everywhere
    models = [HMCModel(D, n, np.full(D, 5.0)) for n in N]
    alpha = float(rel.model.alpha)
    out = {"rmse": float("nan"), "rmse_train": float("nan"), "alpha": alpha, "rmse_avg": float("nan"), "eps": eps, "L": L,
           "accepted": [], "Umodel": models[0], "Vmodel": models[1]}

    with _two_mode.trainer(data, D, lib().bdf_hmc_create, lib().bdf_hmc_destroy, (alpha,), seed=seed, device=device) as (hmc, test):
        check(lib().bdf_hmc_set_test(hmc, test, lo, hi))
        check(lib().bdf_hmc_set_params(hmc, L, L_inner, prior_freq, eps, burnin))
        st = np.zeros(16)
        log = np.zeros(1)
        for i in range(1, burnin + psamples + 1):
            t0 = time.time()
            check(lib().bdf_hmc_iterate(hmc, 1))
            if len(log) < 2 * L + 1:
                log = np.zeros(2 * L + 1)
            check(lib().bdf_hmc_stats(hmc, st.ctypes.data_as(_lib.c_dp), log.ctypes.data_as(_lib.c_dp), len(log)))
            t1 = time.time()
            Lused, acc, Lnew = int(st[2]), st[8] != 0.0, int(st[10])
            out["accepted"].append(bool(acc))
            if verbose:
                _print_iteration(i, burnin, prior_freq, st, log, Lused, acc, Lnew, t1 - t0)
            L = Lnew
        out["rmse"], out["rmse_avg"], out["eps"], out["L"] = float(st[14]), float(st[15]), float(st[9] if burnin + psamples else eps), L
        out["mu"], out["Lambda"] = [], []
        for e, m in enumerate(models):
            n = N[e]
            samp, mom = np.empty((n, D)), np.empty((n, D))
            mu, Lam = np.empty(D), np.empty((D, D))
            check(lib().bdf_hmc_model(hmc, e, samp.ctypes.data_as(_lib.c_dp), mom.ctypes.data_as(_lib.c_dp),
                                      mu.ctypes.data_as(_lib.c_dp), Lam.ctypes.data_as(_lib.c_dp)))
            out["Usample" if e == 0 else "Vsample"] = np.asfortranarray(samp.T)
            m.momentum = np.asfortranarray(mom.T)
            out["mu"].append(mu)
            out["Lambda"].append(np.asfortranarray(Lam.T))
    return out


def _print_iteration(i, burnin, prior_freq, st, log, L, accepted, Lnew, took):
    """the reference's verbose lines of iteration i (macau_hmc.jl:63-131)"""
    if i == burnin + 1:
        print("================== Burnin complete ===================")
    print("======= Step %d =======" % i)
    print("eps = %.2e" % st[1])
    # after step l: U's momentum of its latest launch (2l, or 2l - 2 at l = L), V's of launch 2l - 1
    for l in range(1, L + 1):
        print("  Momentum %d: |r_U| = %.4e, |r_V| = %.4e" % (l, log[2 * l if l < L else 2 * l - 2], log[2 * l - 1]))
    print("  Momentum L: |r_U| = %.4e, |r_V| = %.4e" % (log[2 * L], log[2 * L - 1]))
    dH = st[7]
    print("  ΔH = %.4e  ΔKin = %.4e  ΔPot = %.4e" % (-dH, st[4] - st[3], st[6] - st[5]))
    if accepted:
        print("-> ACCEPTED!")
    else:
        print("-> REJECTED!")
        if dH < -6:
            print("Reducing eps from %.2e to %.2e." % (st[1], st[9]))
            print("Increasing L from %d to %d." % (L, Lnew))
    if i % prior_freq == 0:
        print("Updating priors...")
    print("% 3d: |U|=%.4e  |V|=%.4e  RMSE=%.4f  RMSE(avg)=%.4f [took %.2fs]" % (i, st[11], st[12], st[14], st[15], took))
