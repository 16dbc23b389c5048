"""The pose rig law over ranks (dist.pose_rig_velocity: one all-reduce of the 18 moments) on world_size-2 gloo, CPU only: each
rank holds the moments of its shard of the rig's cameras (from tests/pose_rig_ref.py, every camera's pose in the common rig frame),
and every rank must end with the single-process plain law's twist."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import vitvs_amd  # noqa: F401
from vitvs_amd import dist as vdist

import pose_ref as pr
import pose_rig_ref as rr

LAM = 0.35


def _rig(n_cams, dead, collinear=False):
    rng = np.random.default_rng(60 + n_cams)
    rig = rr.seeded_rig(rng, n_cams)
    R, t = rr.seeded_displacement(rng)
    if collinear:
        X = (np.outer(np.linspace(-0.3, 0.3, 12 * n_cams), rr.unit([1.0, 2.0, 0.5])) + np.array([0.0, 0.0, 0.8])).reshape(n_cams, 12, 3)
    else:
        X = np.concatenate([rng.uniform(-0.4, 0.4, (n_cams, 12, 2)), rng.uniform(0.5, 1.0, (n_cams, 12, 1))], 2)
    P, Q = rr.camera_points(X, rig, R, t)
    if not collinear:
        P = P + 0.002 * rng.standard_normal(P.shape)                  # not exactly consistent: a real least-squares problem
    usable = np.ones((n_cams, 12), np.int32)
    usable[:, 5] = -1
    return P, Q, usable, rig, [2 if i in dead else 0 for i in range(n_cams)]


def _worker(rank, world, port, n_cams, dead, collinear, ret):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    P, Q, usable, rig, sts = _rig(n_cams, dead, collinear)
    b, e = vdist.shard_range(n_cams, rank, world)
    if e > b:
        local = rr.pose_rig_law(P[b:e], Q[b:e], usable[b:e], rig[b:e], sts[b:e], LAM)["moments"]   # what this rank's call reports
    else:
        local = np.zeros(18)
    ret[rank] = vdist.pose_rig_velocity(torch.from_numpy(local), LAM).clone()
    dist.destroy_process_group()


@pytest.mark.parametrize("n_cams,dead,collinear", [(2, (), False), (8, (), False), (5, (3,), False), (3, (1, 2), False),
                                                   (2, (0, 1), False), (4, (), True)])
def test_pose_rig_velocity_two_ranks(n_cams, dead, collinear):
    """Even and ragged shards; a failed camera; a rank none of whose cameras contributes; no camera at all (zeros); a collinear
    stack (degenerate: zeros)."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_worker, args=(2, port, n_cams, dead, collinear, ret), nprocs=2, join=True)
    P, Q, usable, rig, sts = _rig(n_cams, dead, collinear)
    ref = rr.pose_rig_law(P, Q, usable, rig, sts, LAM)
    assert torch.equal(ret[0], ret[1])                               # the same twist on every rank, bit for bit
    got = ret[0].numpy()
    if ref["status"] != pr.OK:
        assert (ref["info"][0] == 0 or ref["info"][5] == 1) and np.array_equal(got, np.zeros(6))
        return
    assert min(ref["gaps"]) >= 1e-3                                   # far from the degeneracy rule: centring after the sum keeps it
    err = np.linalg.norm(got - ref["v"]) / np.linalg.norm(ref["v"])
    assert err <= 1e-9, err
