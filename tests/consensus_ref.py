"""What the consensus starts of the pose law and the homography law share, in fp64 numpy: the statement the phase of
csrc/consensus_core.h is tested against, in the kernel's order of arithmetic.  pose_consensus_ref and homography_consensus_ref bind
it to their models (the rows a hypothesis draws, its closed-form fit, its squared residual) and state the rules in full.
"""
from __future__ import annotations

import numpy as np

MAX_HYP = 4096
DRAWS = 64
_M32 = np.uint64(0xFFFFFFFF)


def mix(x):
    """lowbias32 on an array of 32-bit values held in uint64."""
    x = np.asarray(x, np.uint64) & _M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & _M32
    return x ^ (x >> np.uint64(16))


def draw(seed, n_hyp, n_us, k):
    """-> (pos int64 [n_hyp, k] ascending, ok bool [n_hyp]) for the hypotheses j = 0 .. n_hyp - 1; a function of (seed, j, n_us)."""
    j = np.arange(n_hyp, dtype=np.uint64)
    base = mix(((np.uint64(int(seed) & 0xFFFFFFFF) * np.uint64(0x9E3779B9)) & _M32) + j)
    pos = np.full((n_hyp, k), -1, np.int64)
    cnt = np.zeros(n_hyp, np.int64)
    for c in range(DRAWS):
        r = (mix(base + np.uint64(c)) % np.uint64(n_us)).astype(np.int64)
        new = (cnt < k) & ~(pos == r[:, None]).any(1)
        rows = np.nonzero(new)[0]
        pos[rows, cnt[rows]] = r[rows]
        cnt[rows] += 1
    ok = cnt == k
    return np.where(ok[:, None], np.sort(pos, 1), -1), ok


def consensus(points, usable, T, n_hyp, seed, k, fit, residual_sq):
    """The consensus phase on one pair's ``points`` (arrays [n, .]) with the cut-off ``T``, for hypotheses of ``k`` rows:
    ``fit(*points of the drawn sets [n_hyp, k, .])`` -> (*model, ok [n_hyp]) and ``residual_sq(*model, *points of the usable rows)``
    -> q [n_hyp, n_us].  -> dict(winner (j + 1, or 0), start [n] weights, n_start, costs [n_hyp], gap, edge_T, model (the winner's,
    or None)): ``gap`` = (C' - C) / C' with C the winner's cost and C' the best cost of a hypothesis with another row set (inf when
    there is none), ``edge_T`` = the closest |rho_k / T - 1| of a usable row with a finite rho_k under the winner."""
    us = np.asarray(usable).reshape(-1) > 0
    rows = np.nonzero(us)[0]
    n_us = len(rows)
    out = dict(winner=0, start=np.where(us, 1.0, 0.0), n_start=0, costs=np.full(n_hyp, np.inf), gap=np.inf, edge_T=np.inf, model=None)
    if n_hyp < 1 or n_us < k:
        return out
    out["n_start"] = n_us
    T2 = T * T
    pos, ok = draw(seed, n_hyp, n_us, k)
    sets = rows[np.where(ok[:, None], pos, 0)]
    *model, solved = fit(*(p[sets] for p in points))
    ok &= solved
    q = residual_sq(*model, *(p[rows] for p in points))
    with np.errstate(all="ignore"):
        terms = np.where(q < T2, q, T2)
        costs = np.zeros(n_hyp)
        for i in range(n_us):                                # ascending rows, one after the other
            costs = costs + terms[:, i]
    costs = np.where(ok, costs, np.inf)
    costs = np.where(costs >= 0.0, costs, np.inf)            # (a NaN cost ranks with the skipped ones)
    out["costs"] = costs
    j = int(np.argmin(costs))                                # the first of equal minima: ties go to the smallest j
    if not costs[j] < np.inf:
        return out
    other = ok & (pos != pos[j]).any(1)
    if other.any():
        c2 = float(costs[other].min())
        out["gap"] = (c2 - float(costs[j])) / c2 if c2 < np.inf and c2 > 0.0 else (np.inf if c2 == np.inf else 0.0)
    rho = np.full(len(us), np.inf)
    rho[rows] = np.sqrt(q[j])
    start = np.where(us & (rho <= T), 1.0, 0.0)
    finite = us & np.isfinite(rho)
    out.update(winner=j + 1, start=start, n_start=int(start.sum()), model=tuple(a[j] for a in model),
               edge_T=float(np.abs(rho[finite] / T - 1.0).min()) if finite.any() else np.inf)
    return out
