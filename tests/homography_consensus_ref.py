"""The consensus start of the homography law in fp64 numpy ("The consensus start"): the statement the consensus phase of
csrc/consensus_core.h is tested against on csrc/homography.hip's four-point model, in the kernel's order of arithmetic.  The draw,
the score, the winner and the start are consensus_ref's, shared with pose_consensus_ref.

Per pair, with the usable rows in ascending order, n_us of them, and the cut-off T = 4.6851 sigma_min:

  draw      hypothesis j draws positions r_c = mix(mix(seed 0x9e3779b9 + j) + c) mod n_us for c = 0 .. 63 (32-bit integers), rejects
            repeats and stops at 4 distinct ones; without 4 it is skipped.  The 4 positions are then taken in ascending order, so a
            row set gives one H whatever the order it was drawn in.
  solve     H_j = B(m*) adj(B(m)) on the raw normalised points, B(p) = A diag(adj(A) (x3, y3, 1)) with A's columns (x_i, y_i, 1); the
            sign that makes det H_j > 0; skipped when an entry is not finite or |det H_j| <= 1e-8 |H_j|_F^3, and when three of the
            four points are collinear in either image: twice a triangle's area (the l_i = adj(A) (x3, y3, 1) and their sum det A)
            <= 1e-8 (x extent + y extent)^2.  Of four collinear points every l_i is rounding noise, and so would H and det H be.
  score     C_j = sum over the usable rows, ascending, of min(q_k, T^2), q_k = |pi(H_j m_k) - m*_k|^2 (before the square root), T^2
            where the third component of H_j m_k is <= 0; a skipped hypothesis costs +inf.
  winner    the smallest C_j, ties to the smallest j.
  start     usable row k takes 1 if rho_k = sqrt(q_k) <= T under the winner, else 0; with every hypothesis skipped, all usable rows 1.

From the start weights the law's loop runs as homography_ref.homography_law states it: the weighted normalised DLT, n_iter Tukey
re-weightings with the MAD scale over all usable rows.  The rows the start left out count as weights of 0 (info[3]) from the start.
info[6] = the winner's j + 1 (0: n_hyp = 0, fewer than 4 usable rows, every hypothesis skipped), info[7] = the start weights at 1
(0 when the consensus phase did not run).
"""
from __future__ import annotations

import numpy as np

import consensus_ref as cs
import homography_ref as hr
from consensus_ref import DRAWS, MAX_HYP, mix  # noqa: F401

COLLINEAR_TOL = 1e-8   # a hypothesis with a triangle of its four points, in either image, of <= COLLINEAR_TOL extent^2 is skipped


def draw(seed, n_hyp, n_us):
    """consensus_ref.draw with 4 positions."""
    return cs.draw(seed, n_hyp, n_us, 4)


def _basis(x, y):
    """B = A diag(adj(A) (x3, y3, 1)) for x, y [.., 4] -> (the 9 entries, row-major, each [..], spread): the l_i and their sum
    (det A) are twice the signed areas of the four triangles; ``spread`` is False when one is <= 1e-8 of the squared extent."""
    x0, x1, x2, x3 = (x[..., i] for i in range(4))
    y0, y1, y2, y3 = (y[..., i] for i in range(4))
    l0 = ((y1 - y2) * x3 + (x2 - x1) * y3) + (x1 * y2 - x2 * y1)
    l1 = ((y2 - y0) * x3 + (x0 - x2) * y3) + (x2 * y0 - x0 * y2)
    l2 = ((y0 - y1) * x3 + (x1 - x0) * y3) + (x0 * y1 - x1 * y0)
    ex = np.maximum(np.maximum(x0, x1), np.maximum(x2, x3)) - np.minimum(np.minimum(x0, x1), np.minimum(x2, x3))
    ey = np.maximum(np.maximum(y0, y1), np.maximum(y2, y3)) - np.minimum(np.minimum(y0, y1), np.minimum(y2, y3))
    ext = ex + ey
    area = np.minimum(np.minimum(np.abs(l0), np.abs(l1)), np.minimum(np.abs(l2), np.abs((l0 + l1) + l2)))
    return [x0 * l0, x1 * l1, x2 * l2, y0 * l0, y1 * l1, y2 * l2, l0, l1, l2], area > COLLINEAR_TOL * (ext * ext)


def four_point(m4, ms4):
    """The closed-form homographies of [.., 4, 2] current and goal points -> (H [.., 3, 3] with det > 0, ok [..])."""
    m4, ms4 = np.asarray(m4, np.float64), np.asarray(ms4, np.float64)
    with np.errstate(all="ignore"):
        B, spread = _basis(m4[..., 0], m4[..., 1])
        S, spread_s = _basis(ms4[..., 0], ms4[..., 1])
        J = [B[4] * B[8] - B[5] * B[7], B[2] * B[7] - B[1] * B[8], B[1] * B[5] - B[2] * B[4],
             B[5] * B[6] - B[3] * B[8], B[0] * B[8] - B[2] * B[6], B[2] * B[3] - B[0] * B[5],
             B[3] * B[7] - B[4] * B[6], B[1] * B[6] - B[0] * B[7], B[0] * B[4] - B[1] * B[3]]
        H = [(S[3 * i] * J[k] + S[3 * i + 1] * J[3 + k]) + S[3 * i + 2] * J[6 + k] for i in range(3) for k in range(3)]
        det = (H[0] * (H[4] * H[8] - H[5] * H[7]) - H[1] * (H[3] * H[8] - H[5] * H[6])) + H[2] * (H[3] * H[7] - H[4] * H[6])
        fro2 = np.zeros_like(det)
        finite = np.ones(det.shape, bool)
        for h in H:
            fro2 = fro2 + h * h
            finite &= np.abs(h) < np.inf
        fro = np.sqrt(fro2)
        ok = spread & spread_s & finite & (np.abs(det) > hr.DEGENERATE_TOL * (fro * fro * fro))
        Hm = np.stack([np.where(det < 0.0, -h, h) for h in H], -1).reshape(det.shape + (3, 3))
    return Hm, ok


def transfer_sq(H, m, ms):
    """q [.., n] = |pi(H m) - m*|^2 for H [.., 3, 3] and points [n, 2]; +inf where the third component is <= 0."""
    x, y = m[:, 0], m[:, 1]
    h = lambda i, k: H[..., i, k][..., None]   # noqa: E731
    with np.errstate(all="ignore"):
        X = (h(0, 0) * x + h(0, 1) * y) + h(0, 2)
        Y = (h(1, 0) * x + h(1, 1) * y) + h(1, 2)
        Z = (h(2, 0) * x + h(2, 1) * y) + h(2, 2)
        front = Z > 0.0
        Zs = np.where(front, Z, 1.0)
        d0, d1 = X / Zs - ms[:, 0], Y / Zs - ms[:, 1]
        return np.where(front, d0 * d0 + d1 * d1, np.inf)


def consensus(m, ms, usable, sigma_min, n_hyp, seed):
    """consensus_ref.consensus on one pair's points with four_point and transfer_sq -> its dict with the winner's ``H`` (or None)
    for ``model``."""
    m, ms = np.asarray(m, np.float64).reshape(-1, 2), np.asarray(ms, np.float64).reshape(-1, 2)
    out = cs.consensus((m, ms), usable, hr.TUKEY_C * sigma_min, n_hyp, seed, 4, four_point, transfer_sq)
    (out["H"],) = out.pop("model") or (None,)
    return out


def homography_consensus_law(m, ms, usable, lam, depth_scale=1.0, n_iter=0, sigma_min=0.0, n_hyp=0, seed=0):
    """The law with the consensus start (the seam vitvs_op_homography_consensus_law) -> homography_ref.homography_law's dict with
    info[6], info[7] filled and ``start``, ``gap``, ``edge_T`` of the consensus phase added.  n_hyp = 0: homography_law itself."""
    m, ms = np.asarray(m, np.float64).reshape(-1, 2), np.asarray(ms, np.float64).reshape(-1, 2)
    us = np.asarray(usable).reshape(-1) > 0
    m, ms = np.where(us[:, None], m, 0.0), np.where(us[:, None], ms, 0.0)
    if n_hyp < 1:
        out = hr.homography_law(m, ms, usable, lam, depth_scale, n_iter, sigma_min)
        out.update(start=np.where(us, 1.0, 0.0), gap=np.inf, edge_T=np.inf)
        return out
    con = consensus(m, ms, us, sigma_min, n_hyp, seed)
    n_zero = int(us.sum()) - con["n_start"] if con["winner"] else 0
    out = hr.homography_law(m, ms, usable, lam, depth_scale, n_iter, sigma_min, start=con["start"], n_zero=n_zero)
    out["info"][6:8] = con["winner"], con["n_start"]
    out.update(start=con["start"], gap=con["gap"], edge_T=con["edge_T"])
    return out


def homography_consensus_from_details(det, b, cam_status, K, lam, depth_scale, n_iter, pitch_u, pitch_v, n_hyp, seed):
    """The law of pair ``b`` through the handle (vitvs_homography_consensus_velocity_dev) from ``Engine.last_details``' dict."""
    rows = det["selected"].shape[1]
    zero = dict(v=np.zeros(6), status=int(cam_status), H=np.eye(3), info=np.zeros(8, np.int32), weights=np.zeros(rows), sigma=0.0,
                ratios=[], gaps=[], edge=np.inf, start=np.zeros(rows), gap=np.inf, edge_T=np.inf)
    if int(cam_status) in (hr.NO_CORRESPONDENCE, hr.TOO_FEW):
        return zero
    if int(det["info"][b, 2]):
        zero["status"] = hr.OK
        return zero
    m, ms, usable = hr.points_from_details(det["selected"][b], det["s_uv"][b], det["feat"][b], det["info"][b, 1], K)
    sigma_min = 0.5 * max(pitch_u / float(K[0]), pitch_v / float(K[1]))
    return homography_consensus_law(m, ms, usable, lam, depth_scale, n_iter, sigma_min, n_hyp, seed)
