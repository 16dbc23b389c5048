"""The consensus start of the pose law in fp64 numpy ("The consensus start"): the statement the consensus phase of
csrc/consensus_core.h is tested against on csrc/pose_core.h's three-point model, in the kernel's order of arithmetic.  The draw, the
score, the winner and the start are consensus_ref's, shared with homography_consensus_ref.

Per pair, with the usable rows in ascending order, n_us of them (at least 3, else nothing is drawn), and the cut-off T = 4.6851
sigma_min:

  draw      hypothesis j draws positions r_c = mix(mix(seed 0x9e3779b9 + j) + c) mod n_us for c = 0 .. 63 (32-bit integers), rejects
            repeats and stops at 3 distinct ones; without 3 it is skipped.  The 3 positions are then taken in ascending order, so a
            row set gives one fit whatever the order it was drawn in.
  solve     a triad per cloud x0, x1, x2: a = x1 - x0, b = x2 - x0, n = a x b, e1 = a / |a|, e3 = n / |n|, e2 = e3 x e1;
            R = sum_m e_m(Q) e_m(P)^T, t = qm - R pm with the means of the three points.  Skipped when either cloud has
            |n|^2 <= 1e-8 |a|^2 |b|^2 (collinear or coincident points) or an entry of R or t is not finite.
  score     C_j = sum over the usable rows, ascending, one after the other, of min(q_k, T^2), q_k = |Q_k - (R P_k + t)|^2 (before
            the square root); a skipped hypothesis costs +inf.
  winner    the smallest C_j, ties to the smallest j.
  start     usable row k takes 1 if rho_k = sqrt(q_k) <= T under the winner, else 0; with every hypothesis skipped, all usable rows 1.

From the start weights the law's loop runs as pose_ref.pose_law states it: Horn's weighted alignment, n_iter Tukey re-weightings with
the MAD scale over all usable rows.  The rows the start left out count as weights of 0 (info[3]) from the start; fewer than 3 rows
with a weight are TOO_FEW.  info[6] = the winner's j + 1 (0: n_hyp = 0, fewer than 3 usable rows, every hypothesis skipped), info[7] =
the start weights at 1 (0 when the consensus phase did not run).
"""
from __future__ import annotations

import numpy as np

import consensus_ref as cs
import pose_ref as pr
from consensus_ref import DRAWS, MAX_HYP, mix  # noqa: F401

COLLINEAR_TOL = 1e-8   # a hypothesis with |a x b|^2 <= COLLINEAR_TOL |a|^2 |b|^2 in either cloud is skipped


def draw(seed, n_hyp, n_us):
    """consensus_ref.draw with 3 positions."""
    return cs.draw(seed, n_hyp, n_us, 3)


def _triad(x):
    """x [.., 3 points, 3] -> (e1, e2, e3 as lists of 3 components each [..], spread)."""
    a = [x[..., 1, c] - x[..., 0, c] for c in range(3)]
    b = [x[..., 2, c] - x[..., 0, c] for c in range(3)]
    n = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    aa = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
    bb = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]
    nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
    sa, sn = np.sqrt(aa), np.sqrt(nn)
    e1 = [a[c] / sa for c in range(3)]
    e3 = [n[c] / sn for c in range(3)]
    e2 = [e3[1] * e1[2] - e3[2] * e1[1], e3[2] * e1[0] - e3[0] * e1[2], e3[0] * e1[1] - e3[1] * e1[0]]
    return e1, e2, e3, nn > (COLLINEAR_TOL * aa) * bb


def three_point(P3, Q3):
    """The closed-form displacements of [.., 3, 3] current and goal points -> (R [.., 3, 3], t [.., 3], ok [..])."""
    P3, Q3 = np.asarray(P3, np.float64), np.asarray(Q3, np.float64)
    with np.errstate(all="ignore"):
        p1, p2, p3, spread = _triad(P3)
        q1, q2, q3, spread_q = _triad(Q3)
        R = [[(q1[i] * p1[j] + q2[i] * p2[j]) + q3[i] * p3[j] for j in range(3)] for i in range(3)]
        pm = [((P3[..., 0, c] + P3[..., 1, c]) + P3[..., 2, c]) / 3.0 for c in range(3)]
        qm = [((Q3[..., 0, c] + Q3[..., 1, c]) + Q3[..., 2, c]) / 3.0 for c in range(3)]
        t = [qm[i] - ((R[i][0] * pm[0] + R[i][1] * pm[1]) + R[i][2] * pm[2]) for i in range(3)]
        finite = np.ones(np.shape(t[0]), bool)
        for i in range(3):
            finite &= np.abs(t[i]) < np.inf
            for j in range(3):
                finite &= np.abs(R[i][j]) < np.inf
    Rm = np.stack([np.stack(row, -1) for row in R], -2)
    return Rm, np.stack(t, -1), spread & spread_q & finite


def residual_sq(R, t, P, Q):
    """q [.., n] = |Q - (R P + t)|^2 for R [.., 3, 3], t [.., 3] and points [n, 3], in pose_align's residual arithmetic."""
    r = lambda i, k: R[..., i, k][..., None]   # noqa: E731
    with np.errstate(all="ignore"):
        d = [Q[:, i] - (((r(i, 0) * P[:, 0] + r(i, 1) * P[:, 1]) + r(i, 2) * P[:, 2]) + t[..., i][..., None]) for i in range(3)]
        return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def consensus(P, Q, usable, sigma_min, n_hyp, seed):
    """consensus_ref.consensus on one pair's points with three_point and residual_sq -> its dict with the winner's ``R``, ``t`` (or
    None) for ``model``."""
    P, Q = np.asarray(P, np.float64).reshape(-1, 3), np.asarray(Q, np.float64).reshape(-1, 3)
    out = cs.consensus((P, Q), usable, pr.TUKEY_C * sigma_min, n_hyp, seed, 3, three_point, residual_sq)
    out["R"], out["t"] = out.pop("model") or (None, None)
    return out


def pose_consensus_law(P, Q, usable, lam, n_iter=0, sigma_min=0.0, n_hyp=0, seed=0):
    """The law with the consensus start (the seam vitvs_op_pose_consensus_law) -> pose_ref.pose_law's dict with info[6], info[7]
    filled and ``start``, ``cgap``, ``edge_T`` of the consensus phase added.  n_hyp = 0: pose_law itself."""
    P, Q = np.asarray(P, np.float64).reshape(-1, 3), np.asarray(Q, np.float64).reshape(-1, 3)
    usable = np.asarray(usable).reshape(-1)
    us = usable > 0
    P, Q = np.where(us[:, None], P, 0.0), np.where(us[:, None], Q, 0.0)
    if n_hyp < 1:
        out = pr.pose_law(P, Q, usable, lam, n_iter, sigma_min)
        out.update(start=np.where(us, 1.0, 0.0), cgap=np.inf, edge_T=np.inf)
        return out
    con = consensus(P, Q, us, sigma_min, n_hyp, seed)
    n_zero = int(us.sum()) - con["n_start"] if con["winner"] else 0
    out = pr.pose_law(P, Q, usable, lam, n_iter, sigma_min, start=con["start"], n_zero=n_zero)
    out["info"][6:8] = con["winner"], con["n_start"]
    out.update(start=con["start"], cgap=con["gap"], edge_T=con["edge_T"])
    return out


def pose_consensus_from_details(det, b, cam_status, K, table, lam, n_iter, pitch_u, pitch_v, n_hyp, seed):
    """The law of pair ``b`` through the handle (vitvs_pose_consensus_velocity_dev) from ``Engine.last_details``' dict."""
    rows = det["selected"].shape[1]
    zero = dict(v=np.zeros(6), status=int(cam_status), R=np.eye(3), t=np.zeros(3), info=np.zeros(8, np.int32),
                weights=np.zeros(rows), sigma=0.0, gap=0.0, scatter=0.0, gaps=[], edge=np.inf, start=np.zeros(rows), cgap=np.inf,
                edge_T=np.inf)
    if int(cam_status) != pr.OK or int(det["info"][b, 2]):
        return zero
    P, Q, usable = pr.points_from_details(det["selected"][b], det["s_uv"][b], det["feat"][b], det["info"][b, 1], K, table)
    sigma_min = 0.0
    if (n_iter > 0 or n_hyp > 0) and (usable > 0).any():
        sigma_min = 0.5 * max(pitch_u / float(K[0]), pitch_v / float(K[1])) * pr.median_middle(Q[usable > 0, 2])
    return pose_consensus_law(P, Q, usable, lam, n_iter, sigma_min, n_hyp, seed)
