"""What the trainers on one two-mode relation (bpmf_vb in vb.py, macau_hmc in hmc.py) share: their argument checks, the
training data as bdf_vb_create / bdf_hmc_create read it, and the device objects of a run."""
import contextlib
import ctypes as C

import numpy as np

from . import _lib
from ._lib import ArgumentError, check
from .model_options import ENTITY, RELATION, present


def relation_of(data, num_latent, who):
    """(D, data.relations[0]) once num_latent is in range and the relation is a matrix; who names the trainer in the errors"""
    D = int(num_latent)
    if not 1 <= D <= _lib.BDF_MAX_D:
        raise ArgumentError(f"num_latent={D} must be in 1..{_lib.BDF_MAX_D}")
    if not data.relations:
        raise ArgumentError(f"{who} needs a relation")
    rel = data.relations[0]
    if rel.data.ids.shape[1] != 2 or len(data.entities) < 2:
        raise ArgumentError(f"{who} works on a matrix relation (2 modes); {rel.name} has {rel.data.ids.shape[1]}")
    for owner in [rel] + list(data.entities):
        for opt in present(owner, RELATION if owner is rel else ENTITY):
            if opt.trainer is not None:
                raise ArgumentError(f"{who} {opt.trainer}; {owner.name} {opt.has or 'has ' + opt.phrase} (use macau)")
    return D, rel


def clamp_bounds(clamp):
    """(lo, hi) of clamp = [] or [lo, hi]; lo > hi means no clamping"""
    clamp = [float(x) for x in clamp]
    if not clamp:
        return 1.0, 0.0
    if len(clamp) != 2:
        raise ArgumentError("clamp must be empty or [lo, hi]")
    return clamp[0], clamp[1]


def create_args(data):
    """(dims, nnz, ids, id_bytes, values) of data.relations[0] for bdf_vb_create / bdf_hmc_create: the int64 sizes of
    data.entities[0] and [1], the F-ordered int64 ids and the float64 values.  Each pointer keeps its array alive."""
    rel = data.relations[0]
    ids = np.asfortranarray(rel.data.ids, dtype=np.int64)
    vals = np.ascontiguousarray(rel.data.values, dtype=np.float64)
    dims = np.array([data.entities[0].count, data.entities[1].count], dtype=np.int64)
    return dims.ctypes.data_as(_lib.c_i64p), len(vals), ids.ctypes.data_as(C.c_void_p), 8, vals.ctypes.data_as(_lib.c_dp)


@contextlib.contextmanager
def trainer(data, D, create, destroy, extra, seed, device):
    """One run's device objects: a Context keyed by seed, the trainer create(ctx, D, *create_args(data), *extra, &handle)
    makes, and the test pairs of data.relations[0] (none if it has no test set).  Yields (trainer handle, test pairs handle or
    None); closes the trainer, the test pairs and the context, in that order."""
    from .engine import Context, DevicePairs
    rel = data.relations[0]
    ctx = Context(device=device, seed=seed)
    handle, test = C.c_void_p(), None
    try:
        check(create(ctx.handle, D, *create_args(data), *extra, C.byref(handle)))
        if len(rel.test_vec) > 0:
            test = DevicePairs(ctx, rel.test_vec.ids, rel.test_vec.values)
        yield handle, test.handle if test is not None else None
    finally:
        if handle:
            destroy(handle)
        if test is not None:
            test.close()
        ctx.close()
