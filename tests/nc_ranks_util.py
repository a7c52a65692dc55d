"""Helpers of the tests of hanging-node spaces across ranks: rank threads over linalg.LocalGroup (the scheme of
tests/test_multirank_local_gpu.py), cached spaces / partitions / views, and the device objects of one rank."""
import threading

import numpy as np

from palace_amd.fem import rcb
from palace_amd.fem.ncpart import PartitionedNCSpace
from tests import nc_util as nu

_cache = {}
_lock = threading.Lock()


def partition(name, how):
    """(part, world): 'rcbN', or on mesh A 'hand': the eight children on rank 0, the rest on rank 1."""
    mesh = nu.nc_mesh(name)
    if how == "hand":
        return np.where(mesh.child >= 0, 0, 1).astype(np.int32), 2
    world = int(how[3:])
    return rcb.rcb(mesh.elem_coords().mean(axis=1), world), world


def views(name, kind, p, how):
    """(global NCSpace, [view of rank r]) -- built once per (mesh, kind, order, partition) and shared by the rank threads."""
    key = (name, kind, p, how)
    with _lock:
        if key not in _cache:
            s = nu.nc_space(name, kind, p)
            part, world = partition(name, how)
            _cache[key] = (s, [PartitionedNCSpace(s, part, r, world) for r in range(world)])
        return _cache[key]


def run_ranks(world, rank_main, timeout=120):
    """rank_main(ctx, rank) -> result on `world` rank threads joined by an in-process group (world 1: no communicator).  A
    failing rank aborts the group, so the others leave their barriers; returns the list of results."""
    import torch

    from palace_amd import linalg

    group = linalg.LocalGroup(world) if world > 1 else None
    out, errors = [None] * world, []

    def main(rank):
        try:
            torch.cuda.set_device(0)
            ctx = linalg.Context()
            if world > 1:
                ctx.init_comm_local(group, rank)
            out[rank] = rank_main(ctx, rank)
            ctx.synchronize()
        except Exception as e:  # a failing rank must not leave the others waiting at a barrier for ever
            import traceback

            errors.append((rank, repr(e), traceback.format_exc()))
            if group is not None:
                group.abort()

    threads = [threading.Thread(target=main, args=(r,), daemon=True) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=timeout)
    assert not errors, errors
    assert all(not t.is_alive() for t in threads), "a rank thread is stuck (collective sequence out of step?)"
    return out


def rank_conforming(ctx, view, world):
    """(Conforming that carries the halo, the Halo or None) of one rank's view."""
    from palace_amd import linalg

    halo = linalg.Halo(ctx, view.nbr, view.send, view.recv) if world > 1 else None
    return linalg.Conforming(ctx, view, halo=halo, n_shared=view.n_shared), halo

