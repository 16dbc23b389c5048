"""Multi-GPU layout of the hot path: independent frame pairs sharded contiguously over ranks, one
process per GPU, weights replicated, and a single collective per update — the all-gather of the
6-double twists (48 bytes per pair; latency-bound, so a flat gather, never a ring of buckets).
A rigid rig that wants ONE twist instead sums its cameras' normal equations (``rig_velocity``: one all-reduce of 28 doubles).

The reference has no distributed code; this is the 8-camera-rig layout of
BASELINE.json configs[3].  ``torch.distributed`` backend "nccl" is RCCL on ROCm; the same code runs
on "gloo" for the CPU tests (tests/test_dist_gloo.py).
"""
from __future__ import annotations

from typing import Tuple

import math

import torch


def shard_range(n_pairs: int, rank: int, world: int) -> Tuple[int, int]:
    """[begin, end) of the pairs rank ``rank`` owns: contiguous, sizes differ by at most one."""
    if not 0 <= rank < world:
        raise ValueError("rank outside the world")
    base, extra = divmod(n_pairs, world)
    begin = rank * base + min(rank, extra)
    return begin, begin + base + (1 if rank < extra else 0)


def gather_velocities(v_local: torch.Tensor, n_pairs: int, group=None, out: torch.Tensor = None) -> torch.Tensor:
    """All ranks receive v_c of every pair, [n_pairs, 6] float64, in global pair order.

    ``v_local`` is this rank's [n_local, 6] block (n_local from ``shard_range``).  Equal shards use
    one ``all_gather_into_tensor``; ragged shards are padded to the largest shard first."""
    import torch.distributed as dist
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    sizes = [shard_range(n_pairs, r, world) for r in range(world)]
    n_max = max(e - b for b, e in sizes)
    b, e = sizes[rank]
    if v_local.shape != (e - b, 6):
        raise ValueError(f"rank {rank} should hold {(e - b, 6)}, got {tuple(v_local.shape)}")
    if v_local.is_cuda and dist.get_backend(group) == "gloo":
        # rehearsal path (several ranks sharing one GPU, gloo): stage the 48-byte rows through the host
        full_cpu = gather_velocities(v_local.detach().cpu(), n_pairs, group)
        if out is not None:
            out.copy_(full_cpu)
            return out
        return full_cpu.to(v_local.device)
    if all(e2 - b2 == n_max for b2, e2 in sizes):
        full = out if out is not None else torch.empty((n_pairs, 6), dtype=v_local.dtype, device=v_local.device)
        dist.all_gather_into_tensor(full, v_local.contiguous(), group=group)
        return full
    padded = torch.zeros((n_max, 6), dtype=v_local.dtype, device=v_local.device)
    padded[: e - b] = v_local
    buf = torch.empty((world * n_max, 6), dtype=v_local.dtype, device=v_local.device)
    dist.all_gather_into_tensor(buf, padded, group=group)
    full = out if out is not None else torch.empty((n_pairs, 6), dtype=v_local.dtype, device=v_local.device)
    for r, (b2, e2) in enumerate(sizes):
        full[b2:e2] = buf[r * n_max: r * n_max + (e2 - b2)]
    return full


def unpack_normal(normal: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(G [6, 6] symmetric, g [6]) of the 28 doubles ``vitvs_rig_velocity_dev`` writes: G's upper triangle row-major, g, rows."""
    iu = torch.triu_indices(6, 6, device=normal.device)
    G = torch.zeros((6, 6), dtype=normal.dtype, device=normal.device)
    G[iu[0], iu[1]] = normal[:21]
    G = G + torch.triu(G, 1).T
    return G, normal[21:27]


def rig_velocity(normal_local: torch.Tensor, lam: float, group=None, robust_iterations: int = 0) -> torch.Tensor:
    """The rig law (include/vitvs.h, vitvs_rig_velocity_dev) for a rig spread over ranks: one camera, or one shard of cameras,
    per GPU.  ``normal_local`` is the 28 doubles this rank's rig call left (``Engine.rig_velocity(...)[2]["normal"]``: the normal
    equations G = M^T M, g = M^T e of ITS cameras' stacked rows, and their row count; all zeros when none of its cameras
    contributed).  The project's second collective beside the ``v_c`` gather: ONE ``all_reduce(SUM)`` of the 28 doubles (G and g
    of a stack are the sums of its parts'), then ``v_rig = -lam * pinv(G) g`` in fp64 torch on every rank — the same [6] tensor
    everywhere, all zeros when no rank contributed a row.

    ``torch.linalg.pinv(G, hermitian=True)`` applies its cut-off (eigenvalues below ~6 eps |lambda|_max) to G, whose condition is
    that of M squared — not numpy's rcond = 1e-15 on M as the single-GPU kernel's Jacobi path does: the two agree for the
    well-conditioned stacks a rig produces (tests/test_rig_gloo.py, <= 1e-9) and differ for a stack whose smallest singular value
    is below ~1e-8 of its largest, which the sum of normal equations cannot resolve.

    ``robust_iterations`` > 0 raises ``ValueError``: the robust rig law (``Engine.rig_velocity(..., robust_iterations=N)``) takes
    one median over ALL cameras' residuals per re-weighting, which across ranks is another collective per iteration and is not
    built; it runs on one GPU."""
    if int(robust_iterations) != 0:
        raise ValueError("the robust rig law is not built across ranks (a median over all ranks' residuals per re-weighting); "
                         "run the rig's cameras on one handle: Engine.rig_velocity(..., robust_iterations=N)")
    import torch.distributed as dist
    if normal_local.shape != (28,) or normal_local.dtype != torch.float64:
        raise ValueError("normal_local is the float64 [28] a rig call writes")
    total = normal_local.clone()
    if total.is_cuda and dist.get_backend(group) == "gloo":   # rehearsal path, as gather_velocities
        host = total.cpu()
        dist.all_reduce(host, op=dist.ReduceOp.SUM, group=group)
        total = host.to(normal_local.device)
    else:
        dist.all_reduce(total, op=dist.ReduceOp.SUM, group=group)
    G, g = unpack_normal(total)
    if float(total[27]) == 0.0:
        return torch.zeros(6, dtype=torch.float64, device=normal_local.device)
    return -float(lam) * (torch.linalg.pinv(G, hermitian=True) @ g)


def pose_rig_velocity(moments_local: torch.Tensor, lam: float, group=None, robust_iterations: int = 0) -> torch.Tensor:
    """The pose rig law (include/vitvs.h, vitvs_pose_rig_velocity_dev) for a rig spread over ranks: one camera, or
    one shard of cameras, per GPU, every rank calling the law on ITS cameras with their poses in the common rig frame.
    ``moments_local`` is the 18 doubles that call left (``Engine.pose_rig_velocity(...)[2]["moments"]``: sum w, sum w P', sum w Q',
    sum w P' Q'^T, sum w |P'|^2, sum w |Q'|^2 over its stack; zeros when none of its cameras contributed).  ONE ``all_reduce(SUM)``
    of the 18 doubles (the sums of a stack are the sums of its parts'), then on every rank in fp64 torch: the centroids pc, qc,
    S = sum w P' Q'^T - sw pc qc^T and the two scatters likewise, Horn's 4 x 4 matrix, ``torch.linalg.eigh``, the quaternion of the
    largest eigenvalue with q_w >= 0, t = qc - R pc and ``v_rig = -lam (R^T t, theta u)`` - the same [6] tensor everywhere.  All
    zeros when no rank contributed a row or the stack is degenerate by the kernel's rule (ev_1 - ev_2 <= 1e-8 of the two scatters).

    Raw moments lose the digits the centroid costs: centring AFTER the sum subtracts sw pc qc^T from a sum of the same size, so
    about log10(|pc|^2 / scatter per point) digits of S go, where the single-GPU kernel centres every point first.  For a rig
    whose points lie within a few metres and spread over decimetres that is two or three of sixteen digits
    (tests/test_pose_rig_gloo.py: <= 1e-9 against the single-process law).

    ``robust_iterations`` > 0 raises ``ValueError``: the robust form takes one median over ALL cameras' residuals per
    re-weighting, which across ranks is another collective per iteration and is not built; it runs on one GPU."""
    if int(robust_iterations) != 0:
        raise ValueError("the robust pose rig law is not built across ranks (a median over all ranks' residuals per re-weighting); "
                         "run the rig's cameras on one handle: Engine.pose_rig_velocity(..., robust_iterations=N)")
    import torch.distributed as dist
    if moments_local.shape != (18,) or moments_local.dtype != torch.float64:
        raise ValueError("moments_local is the float64 [18] a pose rig call writes")
    total = moments_local.clone()
    if total.is_cuda and dist.get_backend(group) == "gloo":   # rehearsal path, as gather_velocities
        host = total.cpu()
        dist.all_reduce(host, op=dist.ReduceOp.SUM, group=group)
        total = host.to(moments_local.device)
    else:
        dist.all_reduce(total, op=dist.ReduceOp.SUM, group=group)
    zero = torch.zeros(6, dtype=torch.float64, device=moments_local.device)
    m = total.cpu()
    sw = float(m[0])
    if sw <= 0.0:
        return zero
    pc, qc = m[1:4] / sw, m[4:7] / sw
    S = m[7:16].reshape(3, 3) - sw * torch.outer(pc, qc)
    scatter = float((m[16] - sw * (pc @ pc)) + (m[17] - sw * (qc @ qc)))
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = S.tolist()
    N = torch.tensor([[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
                      [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
                      [Szx - Sxz, Sxy + Syx, Syy - Sxx - Szz, Syz + Szy],
                      [Sxy - Syx, Szx + Sxz, Syz + Szy, Szz - Sxx - Syy]], dtype=torch.float64)
    ev, V = torch.linalg.eigh(N)                              # ascending
    if float(ev[3] - ev[2]) <= 1e-8 * scatter:
        return zero
    q = V[:, 3] / torch.linalg.norm(V[:, 3])
    if float(q[0]) < 0.0:
        q = -q
    a, b, c, d = q.tolist()
    R = torch.tensor([[a * a + b * b - c * c - d * d, 2.0 * (b * c - a * d), 2.0 * (b * d + a * c)],
                      [2.0 * (b * c + a * d), a * a - b * b + c * c - d * d, 2.0 * (c * d - a * b)],
                      [2.0 * (b * d - a * c), 2.0 * (c * d + a * b), a * a - b * b - c * c + d * d]], dtype=torch.float64)
    t = qc - R @ pc
    nv = float(torch.linalg.norm(q[1:]))
    theta_u = torch.zeros(3, dtype=torch.float64) if nv == 0.0 else (2.0 * math.atan2(nv, a) / nv) * q[1:]
    return (-float(lam) * torch.cat([R.T @ t, theta_u])).to(moments_local.device)


class VelocityGather:
    """The per-update ``v_c`` all-gather issued asynchronously (opt-in: ``bench.py`` with VITVS_ASYNC_GATHER=1).

    Measured on one MI355X in a world of one rank (round 1): slower than the synchronous gather (0.577 vs 0.464 ms per
    update) — the extra queue's events cost more than the wait they remove; kept for multi-GPU experiments, where the
    collective's latency is longer.  With several updates in flight (vit-vs_amd/pipeline.py) each update's gather simply
    follows it on its own stream and overlaps the other updates.

    ``post(v_local)`` issues the collective asynchronously: with RCCL it runs on the communicator's own stream behind an
    event of the caller's stream, so the next update's launches do not wait for it; the previous update's collective is
    waited for first (it finished long before), and results alternate between two output buffers, so a buffer is never
    rewritten while a collective may still touch it.  The caller alternates its ``v_local`` buffers the same way
    (``slot`` = update index & 1).  ``finish()`` waits for the outstanding collective; ``latest`` is the last complete
    [n_pairs, 6] table.  Equal shards only (the benchmark's layout); ragged shards use ``gather_velocities``.
    """

    def __init__(self, n_pairs: int, device, dtype=torch.float64, group=None):
        import torch.distributed as dist
        self.group = group
        world = dist.get_world_size(group)
        if n_pairs % world != 0:
            raise ValueError("VelocityGather needs equal shards")
        self.n_pairs = n_pairs
        self.out = [torch.zeros((n_pairs, 6), dtype=dtype, device=device) for _ in range(2)]
        self.pending = None
        self.pending_slot = -1
        self.latest = self.out[0]

    def post(self, v_local: torch.Tensor, slot: int):
        import torch.distributed as dist
        self.finish()
        self.pending = dist.all_gather_into_tensor(self.out[slot & 1], v_local, group=self.group, async_op=True)
        self.pending_slot = slot & 1

    def finish(self):
        if self.pending is not None:
            self.pending.wait()
            self.latest = self.out[self.pending_slot]
            self.pending = None
        return self.latest
