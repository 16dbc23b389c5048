"""The homography law in fp64 numpy: the statement csrc/homography.hip is tested against.

The matched normalised image points of a planar target, m_k in the current image and m*_k in the goal image, are related by one
3 x 3 homography, m* ~ H m.  In tests/planar_sim.py's convention (the camera at pose (R, t): X_goal = R X_cam + t) that matrix is
H = R + t n_c^T / d_c with (n_c, d_c) the plane in the current camera's frame, scaled to det H = 1.  Benhimane and Malis' law
("Homography-based 2D visual servoing", IJRR 2007) builds a twist from H alone, no depth, no normal, no decomposition:

    e_nu = (H - I) m_c,   e_omega = (H21 - H12, H02 - H20, H10 - H01),   v_h = -lambda (z^ e_nu, e_omega)

a twist in the current camera's own optical frame (planar_sim integrates it as t += R v dt, R = R exp([w]x dt)).  To first order
e_nu = t / Z + theta x m_c - (n . t / 3 d) m_c and e_omega = 2 theta + n x t / d, with (theta, t) the camera's pose: the law moves
the camera against its own pose error, and the depth scale z^ only sets the translational rate.

H is estimated by the normalised DLT: Hartley's similarity on either point set, the 9 x 9 normal matrix M = sum w (r0 r0^T + r1
r1^T), the eigenvector of its smallest eigenvalue.  The sums run in the kernel's order (row r belongs to slice r mod 8, every slice
is added in ascending rows, the slices in ascending order) and the eigen-problem is the same cyclic Jacobi with the same stopping
rule and the same order of arithmetic, so the sweep count can be compared exactly; nothing else of the kernel is shared.
"""
from __future__ import annotations

import numpy as np

OK, NO_CORRESPONDENCE, TOO_FEW, NO_DEPTH = 0, 1, 2, 3
TUKEY_C = 4.6851
DEGENERATE_TOL = 1e-8   # degenerate: ev_2 <= DEGENERATE_TOL trace(M), or |det H| <= DEGENERATE_TOL |H|_F^3
JACOBI_TOL = 1e-40      # sweeps end when the off-diagonal squares are <= JACOBI_TOL of all squares
JACOBI_MAX = 32
SQRT2 = 1.4142135623730951


def rodrigues(w):
    w = np.asarray(w, np.float64)
    th = float(np.linalg.norm(w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + (np.sin(th) / th) * K + ((1.0 - np.cos(th)) / (th * th)) * (K @ K)


def sliced_sum(x: np.ndarray) -> np.ndarray:
    """Column sums of x [n, c] in the kernel's order: eight row slices r mod 8, each added in ascending rows (cumsum is
    sequential), then the slices in ascending order."""
    x = np.asarray(x, np.float64).reshape(len(x), -1)
    tot = np.zeros(x.shape[1])
    for s in range(8):
        part = x[s::8]
        tot = tot + (np.cumsum(part, axis=0)[-1] if len(part) else np.zeros(x.shape[1]))
    return tot


def jacobi(M: np.ndarray):
    """Cyclic Jacobi of a symmetric n x n matrix, rotations in lexicographic (p, q) order -> (diagonal, V with eigenvectors in
    columns, sweeps)."""
    A = np.array(M, np.float64)
    n = len(A)
    V = np.eye(n)
    normsq = 0.0
    for i in range(n):
        for j in range(n):
            normsq += A[i, j] * A[i, j]
    sweeps = 0
    for _ in range(JACOBI_MAX):
        off = 0.0
        for p in range(n):
            for q in range(p + 1, n):
                off += A[p, q] * A[p, q]
        if off <= JACOBI_TOL * normsq:
            break
        sweeps += 1
        for p in range(n):
            for q in range(p + 1, n):
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
                for r in range(n):
                    if r != p and r != q:
                        arp, arq = A[r, p], A[r, q]
                        A[r, p] = A[p, r] = c * arp - s * arq
                        A[r, q] = A[q, r] = s * arp + c * arq
                for r in range(n):
                    vrp, vrq = V[r, p], V[r, q]
                    V[r, p] = c * vrp - s * vrq
                    V[r, q] = s * vrp + c * vrq
    return np.array([A[i, i] for i in range(n)]), V, sweeps


def dlt(m, ms, w):
    """The weighted normalised DLT -> dict(H (det 1, or None), mc [2], sweeps, ratio = ev_2 / trace(M), gap = (ev_2 - ev_1) /
    trace(M): what the eigenvector's accuracy hangs on, degenerate)."""
    m, ms, w = np.asarray(m, np.float64), np.asarray(ms, np.float64), np.asarray(w, np.float64)
    s1 = sliced_sum(np.concatenate([w[:, None], w[:, None] * m, w[:, None] * ms], 1))
    sw = s1[0]
    c, cs = s1[1:3] / sw, s1[3:5] / sw
    d, ds = m - c, ms - cs
    s2 = sliced_sum(np.stack([w * np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]),
                              w * np.sqrt(ds[:, 0] * ds[:, 0] + ds[:, 1] * ds[:, 1])], 1))
    dbar, dbars = s2[0] / sw, s2[1] / sw
    out = dict(H=None, mc=c, sweeps=0, ratio=0.0, gap=0.0, degenerate=True)
    if not dbar > 0.0 or not dbars > 0.0:
        return out
    s, ss = SQRT2 / dbar, SQRT2 / dbars
    x, y, xs, ys = d[:, 0] * s, d[:, 1] * s, ds[:, 0] * ss, ds[:, 1] * ss
    one, zero = np.ones_like(x), np.zeros_like(x)
    r0 = np.stack([-x, -y, -one, zero, zero, zero, xs * x, xs * y, xs], 1)
    r1 = np.stack([zero, zero, zero, -x, -y, -one, ys * x, ys * y, ys], 1)
    iu = [(i, j) for i in range(9) for j in range(i, 9)]
    s3 = sliced_sum(np.stack([w * (r0[:, i] * r0[:, j] + r1[:, i] * r1[:, j]) for i, j in iu], 1))
    M = np.zeros((9, 9))
    for q, (i, j) in enumerate(iu):
        M[i, j] = M[j, i] = s3[q]
    trace = 0.0
    for i in range(9):
        trace += M[i, i]
    ev, V, sweeps = jacobi(M)
    i0 = 0
    for i in range(1, 9):
        if ev[i] < ev[i0]:
            i0 = i
    ev1 = min(ev[i] for i in range(9) if i != i0)
    out.update(sweeps=sweeps, ratio=ev1 / trace if trace > 0.0 else 0.0, gap=(ev1 - ev[i0]) / trace if trace > 0.0 else 0.0)
    degenerate = bool(ev1 <= DEGENERATE_TOL * trace)
    hh = V[:, i0]
    G = np.zeros((3, 3))
    for i in range(3):
        G[i, 0] = hh[3 * i] * s
        G[i, 1] = hh[3 * i + 1] * s
        G[i, 2] = hh[3 * i + 2] - (G[i, 0] * c[0] + G[i, 1] * c[1])
    H = np.zeros((3, 3))
    for j in range(3):
        H[0, j] = G[0, j] / ss + cs[0] * G[2, j]
        H[1, j] = G[1, j] / ss + cs[1] * G[2, j]
        H[2, j] = G[2, j]
    det = (H[0, 0] * (H[1, 1] * H[2, 2] - H[1, 2] * H[2, 1]) - H[0, 1] * (H[1, 0] * H[2, 2] - H[1, 2] * H[2, 0])) \
        + H[0, 2] * (H[1, 0] * H[2, 1] - H[1, 1] * H[2, 0])
    fro2 = 0.0
    for k in H.reshape(-1):
        fro2 += k * k
    fro = np.sqrt(fro2)
    if abs(det) <= DEGENERATE_TOL * (fro * fro * fro):
        degenerate = True
    out["degenerate"] = degenerate
    if not degenerate:
        out["H"] = H / np.cbrt(det)
    return out


def twist(H, mc, lam, depth_scale):
    mx, my = float(mc[0]), float(mc[1])
    en = np.array([((H[0, 0] - 1.0) * mx + H[0, 1] * my) + H[0, 2],
                   (H[1, 0] * mx + (H[1, 1] - 1.0) * my) + H[1, 2],
                   (H[2, 0] * mx + H[2, 1] * my) + (H[2, 2] - 1.0)])
    ew = np.array([H[2, 1] - H[1, 2], H[0, 2] - H[2, 0], H[1, 0] - H[0, 1]])
    return np.concatenate([-lam * (depth_scale * en), -lam * ew])


def transfer_error(H, m, ms):
    """rho = |pi(H m) - m*|; +inf where the third component of H m is <= 0."""
    x, y = m[:, 0], m[:, 1]
    X = (H[0, 0] * x + H[0, 1] * y) + H[0, 2]
    Y = (H[1, 0] * x + H[1, 1] * y) + H[1, 2]
    Z = (H[2, 0] * x + H[2, 1] * y) + H[2, 2]
    front = Z > 0.0
    Zs = np.where(front, Z, 1.0)
    d0, d1 = X / Zs - ms[:, 0], Y / Zs - ms[:, 1]
    return np.where(front, np.sqrt(d0 * d0 + d1 * d1), np.inf)


def median_middle(x):
    """The median as the mean of the two middle values (the same one for an odd count)."""
    s = np.sort(np.asarray(x, np.float64))
    n = len(s)
    return (s[(n - 1) >> 1] + s[n >> 1]) * 0.5


def homography_law(m, ms, usable, lam, depth_scale=1.0, n_iter=0, sigma_min=0.0, start=None, n_zero=0):
    """The law on given points (the seam vitvs_op_homography_law).  ``usable`` [n]: > 0 a usable row.  -> dict(v [6], status, H,
    info [8], weights [n], sigma, ratios, edge): info = usable rows, Jacobi sweeps of the last solve, re-weightings done, usable
    rows with final weight 0, degenerate flag, rows with rho = inf at the last re-weighting, 0, 0; ``ratios`` = every solve's
    ev_2 / trace(M), ``gaps`` = every solve's (ev_2 - ev_1) / trace(M), ``edge`` = the closest |rho / (c sigma) - 1| of a usable row.
    ``start`` [n]: the weights of the first solve instead of 1 on every usable row, ``n_zero`` the usable rows it leaves at weight 0
    (a consensus start: homography_consensus_ref)."""
    m, ms = np.asarray(m, np.float64).reshape(-1, 2), np.asarray(ms, np.float64).reshape(-1, 2)
    us = np.asarray(usable).reshape(-1) > 0
    m, ms = np.where(us[:, None], m, 0.0), np.where(us[:, None], ms, 0.0)
    n_us = int(us.sum())
    w = np.where(us, 1.0, 0.0) if start is None else np.array(start, np.float64).reshape(-1)
    status, sweeps, reweighted, degenerate, n_inf, sigma = OK, 0, 0, 0, 0, 0.0
    H, mc = np.eye(3), np.zeros(2)
    ratios, gaps, edge = [], [], np.inf
    it = 0
    with np.errstate(all="ignore"):
        while True:
            if n_us - n_zero < 4:
                status = TOO_FEW
                break
            h = dlt(m, ms, w)
            sweeps = h["sweeps"]
            ratios.append(h["ratio"])
            gaps.append(h["gap"])
            if h["degenerate"]:
                degenerate, status = 1, TOO_FEW
                break
            H, mc = h["H"], h["mc"]
            if it == n_iter:
                break
            rho = np.where(us, transfer_error(H, m, ms), np.inf)
            n_inf = int((us & np.isinf(rho)).sum())
            sigma = max(1.4826 * median_middle(rho[us]), sigma_min)
            tt = rho / (TUKEY_C * sigma)
            u = 1.0 - tt * tt
            finite = us & np.isfinite(tt)
            if finite.any():
                edge = min(edge, float(np.abs(tt[finite] - 1.0).min()))
            w = np.where(us & (tt < 1.0), u * u, 0.0)
            n_zero = int((us & (w == 0.0)).sum())
            it += 1
            reweighted = it
    if status != OK:
        H, v = np.eye(3), np.zeros(6)
    else:
        v = twist(H, mc, lam, depth_scale)
    info = np.array([n_us, sweeps, reweighted, n_zero, degenerate, n_inf, 0, 0], np.int32)
    return dict(v=v, status=status, H=H, info=info, weights=w, sigma=sigma, ratios=ratios, gaps=gaps, edge=edge)


def points_from_details(selected, s_uv, feat, n_rows, K):
    """m, m* and the usable flag of one pair from what the camera's law left: ``selected`` [rows] goal tokens (-1 padded), ``s_uv``
    [rows, 4] (u*, v*, u, v), ``feat`` [rows, 4] (Z, x, y, sim), the first ``n_rows`` rows written; ``K`` = (fx, fy, cx, cy)."""
    fx, fy, cx, cy = (float(k) for k in K)
    rows = len(selected)
    m, ms, usable = np.zeros((rows, 2)), np.zeros((rows, 2)), np.zeros(rows, np.int32)
    for k in range(min(int(n_rows), rows)):
        if int(selected[k]) < 0:
            continue
        m[k] = (float(feat[k][1]), float(feat[k][2]))
        ms[k] = ((float(s_uv[k][0]) - cx) / fx, (float(s_uv[k][1]) - cy) / fy)
        usable[k] = 1
    return m, ms, usable


def homography_from_details(det, b, cam_status, K, lam, depth_scale, n_iter, pitch_u, pitch_v):
    """The law of pair ``b`` through the handle (vitvs_homography_velocity_dev) from ``Engine.last_details``' dict."""
    rows = det["selected"].shape[1]
    zero = dict(v=np.zeros(6), status=int(cam_status), H=np.eye(3), info=np.zeros(8, np.int32), weights=np.zeros(rows), sigma=0.0,
                ratios=[], gaps=[], edge=np.inf)
    if int(cam_status) in (NO_CORRESPONDENCE, TOO_FEW):
        return zero
    if int(det["info"][b, 2]):                           # the same-image shortcut: the camera is at the goal
        zero["status"] = OK
        return zero
    m, ms, usable = points_from_details(det["selected"][b], det["s_uv"][b], det["feat"][b], det["info"][b, 1], K)
    sigma_min = 0.5 * max(pitch_u / float(K[0]), pitch_v / float(K[1]))
    return homography_law(m, ms, usable, lam, depth_scale, n_iter, sigma_min)


# ------------------------------------------------------------------------------------------ planar_sim's convention
def true_homography(R, t, plane_z=0.61):
    """The homography current -> goal of the plane z = plane_z (goal frame) for a camera at pose (R, t), X_goal = R X_cam + t:
    H = R + t n_c^T / d_c with n_c = R^T e_z and d_c = plane_z - t_z the plane in the camera's frame, scaled to det 1."""
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64)
    n_c = R.T @ np.array([0.0, 0.0, 1.0])
    d_c = plane_z - t[2]
    H = R + np.outer(t, n_c) / d_c
    return H / np.cbrt(np.linalg.det(H))


def project(X_goal, R, t):
    """Normalised image points of goal-frame points in a camera at pose (R, t): X_cam = R^T (X_goal - t)."""
    Xc = (np.asarray(X_goal, np.float64) - t) @ R
    return Xc[:, :2] / Xc[:, 2:3]


def step(R, t, v, dt):
    """tests/planar_sim.py's integration of a body twist."""
    return R @ rodrigues(v[3:] * dt), t + R @ v[:3] * dt


def pose_error(R, t):
    """(|t| in metres, the rotation angle in degrees) of a camera pose against the goal's."""
    ang = np.degrees(np.arccos(np.clip((np.trace(R) - 1.0) * 0.5, -1.0, 1.0)))
    return float(np.linalg.norm(t)), float(ang)
