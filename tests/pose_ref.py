"""The pose law in fp64 numpy: the statement csrc/pose.hip is tested against.

Two clouds of 3-D points with known pairing, P_k in the current camera's frame and Q_k in the goal camera's, define one rigid
displacement X_goal = R X_cam + t (Horn's closed form over the unit quaternion).  The law is ViSP's PBVS law on it,

    v_pose = -lambda (R^T t, theta u)

a twist in the current camera's own optical frame (tests/planar_sim.py integrates it as t += R v dt, R = R exp([w]x dt): |t| and
theta both shrink by (1 - lambda dt) per step, the camera moves on a straight line and turns about a fixed axis).

The sums run in the kernel's order (row r belongs to slice r mod 8, every slice is added in ascending rows, the slices in ascending
order), the 4 x 4 eigen-problem is the same cyclic Jacobi with the same stopping rule, so the sweep count can be compared exactly;
nothing else of the kernel is shared.  ``ibvs_velocity`` is the plain image-based law on the same points, for comparison.
"""
from __future__ import annotations

import numpy as np

from homography_ref import median_middle, rodrigues, sliced_sum, step  # noqa: F401  (re-exported)

OK, TOO_FEW = 0, 2
TUKEY_C = 4.6851
HOLE_Z = 100.0          # the camera law's depth of a pixel without a reading
GAP_TOL = 1e-8          # degenerate: ev_1 - ev_2 <= GAP_TOL (sum w |P - pc|^2 + sum w |Q - qc|^2)
JACOBI_TOL = 1e-40      # sweeps end when the off-diagonal squares are <= JACOBI_TOL of all squares
JACOBI_MAX = 32


def jacobi4(N: np.ndarray):
    """Cyclic Jacobi of a symmetric 4 x 4 matrix -> (diagonal, V with eigenvectors in columns, sweeps)."""
    A = np.array(N, np.float64)
    V = np.eye(4)
    normsq = 0.0
    for i in range(4):
        for j in range(4):
            normsq += A[i, j] * A[i, j]
    sweeps = 0
    for _ in range(JACOBI_MAX):
        off = 0.0
        for p in range(4):
            for q in range(p + 1, 4):
                off += A[p, q] * A[p, q]
        if off <= JACOBI_TOL * normsq:
            break
        sweeps += 1
        for p in range(4):
            for q in range(p + 1, 4):
                apq = A[p, q]
                if apq == 0.0:
                    continue
                theta = (A[q, q] - A[p, p]) / (2.0 * apq)
                t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                A[p, p] = A[p, p] - t * apq
                A[q, q] = A[q, q] + t * apq
                A[p, q] = A[q, p] = 0.0
                for r in range(4):
                    if r != p and r != q:
                        arp, arq = A[r, p], A[r, q]
                        A[r, p] = A[p, r] = c * arp - s * arq
                        A[r, q] = A[q, r] = s * arp + c * arq
                for r in range(4):
                    vrp, vrq = V[r, p], V[r, q]
                    V[r, p] = c * vrp - s * vrq
                    V[r, q] = s * vrp + c * vrq
    return np.array([A[i, i] for i in range(4)]), V, sweeps


def horn(P, Q, w):
    """The weighted alignment min sum w |Q - (R P + t)|^2 -> dict(R, t, q (w first), sweeps, gap, scatter, degenerate)."""
    P, Q, w = np.asarray(P, np.float64), np.asarray(Q, np.float64), np.asarray(w, np.float64)
    s1 = sliced_sum(np.concatenate([w[:, None], w[:, None] * P, w[:, None] * Q], 1))
    sw = s1[0]
    pc, qc = s1[1:4] / sw, s1[4:7] / sw
    dp, dq = P - pc, Q - qc
    cols = [w * dp[:, a] * dq[:, b] for a in range(3) for b in range(3)]
    cols.append(w * (dp[:, 0] * dp[:, 0] + dp[:, 1] * dp[:, 1] + dp[:, 2] * dp[:, 2]))
    cols.append(w * (dq[:, 0] * dq[:, 0] + dq[:, 1] * dq[:, 1] + dq[:, 2] * dq[:, 2]))
    s2 = sliced_sum(np.stack(cols, 1))
    S = s2[:9].reshape(3, 3)
    scatter = s2[9] + s2[10]
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = S
    N = np.array([[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
                  [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
                  [Szx - Sxz, Sxy + Syx, Syy - Sxx - Szz, Syz + Szy],
                  [Sxy - Syx, Szx + Sxz, Syz + Szy, Szz - Sxx - Syy]])
    ev, V, sweeps = jacobi4(N)
    i1 = 0
    for i in range(1, 4):
        if ev[i] > ev[i1]:
            i1 = i
    ev2 = max(ev[i] for i in range(4) if i != i1)
    gap = ev[i1] - ev2
    q = V[:, i1].copy()
    q = q / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    if q[0] < 0.0:
        q = -q
    a, b, c, d = q
    R = np.array([[a * a + b * b - c * c - d * d, 2.0 * (b * c - a * d), 2.0 * (b * d + a * c)],
                  [2.0 * (b * c + a * d), a * a - b * b + c * c - d * d, 2.0 * (c * d - a * b)],
                  [2.0 * (b * d - a * c), 2.0 * (c * d + a * b), a * a - b * b - c * c + d * d]])
    t = qc - R @ pc
    return dict(R=R, t=t, q=q, sweeps=sweeps, gap=gap, scatter=scatter, degenerate=bool(gap <= GAP_TOL * scatter))


def theta_u(q):
    """Rotation vector of a unit quaternion (w first) with q_w >= 0."""
    nv = np.sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    if nv == 0.0:
        return np.zeros(3)
    return (2.0 * np.arctan2(nv, q[0]) / nv) * q[1:]


def twist(R, t, q, lam):
    return np.concatenate([-lam * (R.T @ t), -lam * theta_u(q)])


def pose_law(P, Q, usable, lam, n_iter=0, sigma_min=0.0, start=None, n_zero=0):
    """The law on given points (the seam vitvs_op_pose_law).  ``usable`` [n]: > 0 a usable row, 0 a padded one, < 0 a hole (a row
    dropped for want of a depth).  -> dict(v [6], status, R, t, info [8], weights [n], sigma, gap, scatter): info = usable rows,
    Jacobi sweeps of the last solve, re-weightings done, usable rows with final weight 0, degenerate flag, holes dropped, 0, 0.
    ``start`` [n]: the weights of the first solve instead of 1 on every usable row, ``n_zero`` the usable rows it leaves at weight 0
    (a consensus start: pose_consensus_ref)."""
    P, Q = np.asarray(P, np.float64).reshape(-1, 3), np.asarray(Q, np.float64).reshape(-1, 3)
    usable = np.asarray(usable).reshape(-1)
    us = usable > 0
    n_us, holes = int(us.sum()), int((usable < 0).sum())
    w = np.where(us, 1.0, 0.0) if start is None else np.array(start, np.float64).reshape(-1)
    status, sweeps, reweighted, degenerate, sigma = OK, 0, 0, 0, 0.0
    R, t, q, gap, scatter = np.eye(3), np.zeros(3), np.array([1.0, 0, 0, 0]), 0.0, 0.0
    gaps, edge = [], np.inf                               # every solve's relative gap; the closest |rho / (c sigma) - 1| of a usable row
    it = 0
    while True:
        if n_us - n_zero < 3:
            status = TOO_FEW
            break
        h = horn(P, Q, w)
        sweeps, gap, scatter = h["sweeps"], h["gap"], h["scatter"]
        gaps.append(gap / scatter if scatter > 0.0 else 0.0)
        if h["degenerate"]:
            degenerate, status = 1, TOO_FEW
            break
        R, t, q = h["R"], h["t"], h["q"]
        if it == n_iter:
            break
        d = Q - (P @ R.T + t)
        rho = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        sigma = max(1.4826 * median_middle(rho[us]), sigma_min)
        tt = rho / (TUKEY_C * sigma)
        u = 1.0 - tt * tt
        edge = min(edge, float(np.abs(tt[us] - 1.0).min()))
        w = np.where(us & (tt < 1.0), u * u, 0.0)
        n_zero = int((us & (w == 0.0)).sum())
        it += 1
        reweighted = it
    if status != OK:
        R, t, v = np.eye(3), np.zeros(3), np.zeros(6)
    else:
        v = twist(R, t, q, lam)
    info = np.array([n_us, sweeps, reweighted, n_zero, degenerate, holes, 0, 0], np.int32)
    return dict(v=v, status=status, R=R, t=t, info=info, weights=w, sigma=sigma, gap=gap, scatter=scatter,
                gaps=gaps, edge=edge)


def points_from_details(selected, s_uv, feat, n_rows, K, table):
    """P, Q and the usable flag of one pair from what the camera's law left: ``selected`` [rows] goal tokens (-1 padded), ``s_uv``
    [rows, 4] (u*, v*, u, v), ``feat`` [rows, 4] (Z, x, y, sim), the first ``n_rows`` rows written; ``K`` = (fx, fy, cx, cy);
    ``table`` [T + 1] uint16 millimetres, the goal depth at every goal token's patch centre."""
    fx, fy, cx, cy = (float(k) for k in K)
    rows = len(selected)
    P, Q, usable = np.zeros((rows, 3)), np.zeros((rows, 3)), np.zeros(rows, np.int32)
    T = len(table) - 1
    for k in range(min(int(n_rows), rows)):
        tok = int(selected[k])
        if tok < 0 or tok >= T:
            continue
        Z, x, y = (float(f) for f in feat[k][:3])
        zs_mm = int(table[tok])
        if not (Z < HOLE_Z) or zs_mm == 0:
            usable[k] = -1
            continue
        Zs = zs_mm / 1000.0
        xs, ys = (float(s_uv[k][0]) - cx) / fx, (float(s_uv[k][1]) - cy) / fy
        P[k] = (Z * x, Z * y, Z)
        Q[k] = (Zs * xs, Zs * ys, Zs)
        usable[k] = 1
    return P, Q, usable


def pose_from_details(det, b, cam_status, K, table, lam, n_iter, pitch_u, pitch_v):
    """The law of pair ``b`` through the handle (vitvs_pose_velocity_dev) from ``Engine.last_details``' dict."""
    rows = det["selected"].shape[1]
    zero = dict(v=np.zeros(6), status=int(cam_status), R=np.eye(3), t=np.zeros(3), info=np.zeros(8, np.int32),
                weights=np.zeros(rows), sigma=0.0, gap=0.0, scatter=0.0, gaps=[], edge=np.inf)
    if int(cam_status) != OK:
        return zero
    if int(det["info"][b, 2]):                           # the same-image shortcut: the camera is at the goal
        return zero
    P, Q, usable = points_from_details(det["selected"][b], det["s_uv"][b], det["feat"][b], det["info"][b, 1], K, table)
    sigma_min = 0.0
    if n_iter > 0 and (usable > 0).any():
        sigma_min = 0.5 * max(pitch_u / float(K[0]), pitch_v / float(K[1])) * median_middle(Q[usable > 0, 2])
    return pose_law(P, Q, usable, lam, n_iter, sigma_min)


def interaction_rows(x, y, Z):
    L = np.zeros((2 * len(x), 6))
    L[0::2] = np.stack([-1.0 / Z, 0 * x, x / Z, x * y, -(1.0 + x * x), y], 1)
    L[1::2] = np.stack([0 * x, -1.0 / Z, y / Z, 1.0 + y * y, -(x * y), -x], 1)
    return L


def ibvs_velocity(P, Q, lam):
    """The plain image-based law on the same points: s = P's normalised image point at its depth, s* = Q's; v = -lambda pinv(L(s, Z))
    (s - s*)."""
    P, Q = np.asarray(P, np.float64), np.asarray(Q, np.float64)
    x, y, Z = P[:, 0] / P[:, 2], P[:, 1] / P[:, 2], P[:, 2]
    e = np.stack([x - Q[:, 0] / Q[:, 2], y - Q[:, 1] / Q[:, 2]], 1).reshape(-1)
    return -lam * (np.linalg.pinv(interaction_rows(x, y, Z)) @ e)


def points_in_camera(X_goal, R, t):
    """Points given in the goal frame as the camera at pose (R, t) sees them: X_cam = R^T (X_goal - t)."""
    return (np.asarray(X_goal) - t) @ R


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def unusable_flags(rows, where, n_off):
    """`n_off` unusable rows first / in the middle / last, alternating padded rows (0) and holes (-1)."""
    u = np.ones(rows, np.int32)
    start = {"first": 0, "middle": (rows - n_off) // 2, "last": rows - n_off}[where]
    u[start:start + n_off] = np.where(np.arange(n_off) % 2 == 0, 0, -1)
    return u
