"""Variational BPMF: bpmf_vb and VBModel (src/macau_vb.jl).

VBModel is the reference's host-side model (same field names; mu_u is D x N, Euu D x D x N).  bpmf_vb runs the iterations on
the device through the library's bdf_vb_* entry points (csrc/bdf_vb.hip, csrc/k_vb.hip) and returns host VBModels.  One GPU,
one two-mode relation: VB on several GPUs and on tensors is out of scope.
"""
import time

import numpy as np

from . import _lib, _two_mode
from ._lib import check, lib


class VBModel:
    """VBModel(num_latent, N) (macau_vb.jl:20-37).  seed: an int, None or a numpy Generator (numpy.random.default_rng(seed))
    for mu_u = randn(num_latent, N)."""

    def __init__(self, num_latent, N, seed=None):
        D, N = int(num_latent), int(N)
        rng = np.random.default_rng(seed)
        self.mu_u = rng.standard_normal((D, N))
        self.nu_N = float(D + N)
        self.W_N = 1.0 / N * np.eye(D)
        self.mu_N = np.zeros(D)
        self.b_N = 2.0 + N
        self.Winv_0 = np.eye(D)
        self.mu_0 = np.zeros(D)
        self.b_0 = 2.0
        # E[u u'] = inv(L_u_i) + mu_u mu_u'
        self.Euu = np.linalg.inv(self.W_N)[:, :, None] + self.mu_u[:, None, :] * self.mu_u[None, :, :]

    def __repr__(self):
        return "VBModel of %d instances: |mu_u|=%0.3e" % (self.mu_u.shape[1], np.linalg.norm(self.mu_u))


def bpmf_vb(data, num_latent=10, verbose=True, niter=100, clamp=(), seed=0, device=None):
    """bpmf_vb(data; num_latent=10, verbose=true, niter=100, clamp=Float64[]) (macau_vb.jl:39-90) on the device.

    Uses data.relations[0] only; its precision alpha is fixed.  The initial means are drawn with
    numpy.random.default_rng(seed), U's first.  Returns {"Umodel", "Vmodel", "rmse", "rmse_train", "alpha"}."""
    D, rel = _two_mode.relation_of(data, num_latent, "bpmf_vb")
    lo, hi = _two_mode.clamp_bounds(clamp)
    niter = int(niter)
    rng = np.random.default_rng(seed)
    Umodel = VBModel(D, data.entities[0].count, rng)
    Vmodel = VBModel(D, data.entities[1].count, rng)
    alpha = float(rel.model.alpha)
    out = {"Umodel": Umodel, "Vmodel": Vmodel, "rmse": float("nan"), "rmse_train": float("nan"), "alpha": alpha}
    if niter <= 0:
        return out

    mu_u, mu_v = np.asfortranarray(Umodel.mu_u), np.asfortranarray(Vmodel.mu_u)
    extra = (alpha, mu_u.ctypes.data_as(_lib.c_dp), mu_v.ctypes.data_as(_lib.c_dp))
    with _two_mode.trainer(data, D, lib().bdf_vb_create, lib().bdf_vb_destroy, extra, seed=0, device=device) as (vb, test):
        check(lib().bdf_vb_set_test(vb, test, lo, hi))
        st = np.zeros(4)
        stp = st.ctypes.data_as(_lib.c_dp)
        if verbose:
            for i in range(1, niter + 1):
                t0 = time.time()
                check(lib().bdf_vb_iterate(vb, 1))
                check(lib().bdf_vb_stats(vb, stp))
                t1 = time.time()
                print("% 3d: |U|=%.4e  |V|=%.4e  RMSE=%.4f  RMSE(train)=%.4f  [took %.2fs]" % (i, st[2], st[3], st[0], st[1], t1 - t0))
        else:
            check(lib().bdf_vb_iterate(vb, niter))
            check(lib().bdf_vb_stats(vb, stp))
        out["rmse"], out["rmse_train"] = float(st[0]), float(st[1])
        for e, m in enumerate((Umodel, Vmodel)):
            N = m.mu_u.shape[1]
            mu = np.empty((N, D))
            Euu = np.empty((N, D, D))
            prior = np.empty(D + D * D + 2)
            check(lib().bdf_vb_model(vb, e, mu.ctypes.data_as(_lib.c_dp), Euu.ctypes.data_as(_lib.c_dp),
                                     prior.ctypes.data_as(_lib.c_dp)))
            m.mu_u = np.asfortranarray(mu.T)
            m.Euu = np.asfortranarray(Euu.transpose(2, 1, 0))
            m.mu_N = prior[:D].copy()
            m.W_N = np.asfortranarray(prior[D:D + D * D].reshape(D, D).T)
            m.nu_N, m.b_N = float(prior[D + D * D]), float(prior[D + D * D + 1])
    return out
