"""The rig law over ranks (dist.rig_velocity: one all-reduce of the 28 normal-equation doubles) on world_size-2 gloo, CPU only:
each rank holds the normal equations of its shard of the rig's cameras, and every rank must end with the single-process
stacked law's twist."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import vitvs_amd  # noqa: F401
from vitvs_amd import dist as vdist

import rig_ref as rg

LAM = 0.35


def _rig(n_cams, dead):
    Ls, es, Ws, _ = rg.scenario(40 + n_cams, n_cams=n_cams, pairs=24)
    rng = np.random.default_rng(n_cams)
    es = [e + 1e-3 * rng.standard_normal(e.shape) for e in es]      # not exactly consistent: a real least-squares problem
    return Ls, es, Ws, [2 if i in dead else 0 for i in range(n_cams)]


def _worker(rank, world, port, n_cams, dead, ret):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    Ls, es, Ws, sts = _rig(n_cams, dead)
    b, e = vdist.shard_range(n_cams, rank, world)
    local = rg.normal_packed(*rg.stacked(Ls[b:e], es[b:e], Ws[b:e], sts[b:e]))    # what this rank's rig call reports
    ret[rank] = vdist.rig_velocity(torch.from_numpy(local), LAM).clone()
    dist.destroy_process_group()


@pytest.mark.parametrize("n_cams,dead", [(2, ()), (8, ()), (5, (3,)), (3, (1, 2)), (2, (0, 1))])
def test_rig_velocity_two_ranks(n_cams, dead):
    """Even and ragged shards; a failed camera; a rank none of whose cameras contributes; no camera at all (zeros)."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_worker, args=(2, port, n_cams, dead, ret), nprocs=2, join=True)
    Ls, es, Ws, sts = _rig(n_cams, dead)
    ref = rg.rig_law(Ls, es, Ws, sts, LAM)
    want = ref["v_rig"]
    assert torch.equal(ret[0], ret[1])                               # the same twist on every rank, bit for bit
    got = ret[0].numpy()
    if ref["rows"] == 0:
        assert np.array_equal(got, np.zeros(6))
        return
    assert rg.ldlt_margin(ref["M"]) >= 100                            # well conditioned: the cut-off on G plays no part
    err = np.linalg.norm(got - want) / np.linalg.norm(want)
    assert err <= 1e-9, err


def test_unpack_normal_round_trip():
    Ls, es, Ws, _ = rg.scenario(1)
    M, e = rg.stacked(Ls, es, Ws, [0, 0, 0])
    G, g = vdist.unpack_normal(torch.from_numpy(rg.normal_packed(M, e)))
    assert np.allclose(G.numpy(), M.T @ M, rtol=0, atol=0) and np.array_equal(g.numpy(), M.T @ e)
