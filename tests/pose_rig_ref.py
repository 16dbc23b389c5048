"""The pose rig law in fp64 numpy: the statement csrc/pose_rig.hip is tested against.

A rigid rig of cameras, camera i at pose (R_i, t_i) in the rig frame (X_rig = R_i X_cam + t_i).  Every contributing camera's
usable rows give the points of the pose law (tests/pose_ref.py), P_k in the current camera's frame and Q_k in the goal camera's;
carried into the rig frame, P'_k = R_i P_k + t_i and Q'_k = R_i Q_k + t_i, they are points of the current and of the goal RIG, and
ONE alignment over the whole stack, Q' = R P' + t, is the current rig in the goal rig's frame.  The law is the pose law's on it,

    v_rig = -lambda (R^T t, theta u)

a twist in the rig's own frame (integrated as t += R v dt, R = R exp([w]x dt), as tests/test_gpu_rig_loop.py does).

The stack has a fixed layout, row i * ld + k, so the sliced sums of pose_ref.horn run over the same rows in the same order as the
kernel's; rows a camera did not write and rows of cameras that do not contribute carry flag 0, weight 0 and zero points.  Nothing
of the kernel is shared beyond what pose_ref states.  ``per_camera_average`` is the alternative the law is NOT: the pose law per
camera, every twist carried to the rig frame, the mean over the cameras that solved.
"""
from __future__ import annotations

import numpy as np

import pose_ref as pr
from pose_ref import unit  # noqa: F401
from rig_robust_ref import rel_miss  # noqa: F401

OK, TOO_FEW = pr.OK, pr.TOO_FEW


def to_rig(X, R, t):
    """R X + t per row, each coordinate as ((r0 x0 + r1 x1) + r2 x2) + t (the kernel's order, no contraction)."""
    X = np.asarray(X, np.float64).reshape(-1, 3)
    R, t = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    out = np.zeros_like(X)
    for c in range(3):
        out[:, c] = ((R[c, 0] * X[:, 0] + R[c, 1] * X[:, 1]) + R[c, 2] * X[:, 2]) + t[c]
    return out


def rtc_rows(rig):
    """[(R_i, t_i)] -> float64 [n, 12]: R_i row-major, then t_i (the C ABI's rTc)."""
    return np.stack([np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3)]) for R, t in rig])


def moments(Ps, Qs, w):
    """The 18 raw sums of the stack in the kernel's slice order: sum w, sum w P', sum w Q', sum (w P'_a) Q'_b, sum w |P'|^2,
    sum w |Q'|^2."""
    cols = [w] + [w * Ps[:, c] for c in range(3)] + [w * Qs[:, c] for c in range(3)]
    cols += [(w * Ps[:, a]) * Qs[:, b] for a in range(3) for b in range(3)]
    cols.append(w * ((Ps[:, 0] * Ps[:, 0] + Ps[:, 1] * Ps[:, 1]) + Ps[:, 2] * Ps[:, 2]))
    cols.append(w * ((Qs[:, 0] * Qs[:, 0] + Qs[:, 1] * Qs[:, 1]) + Qs[:, 2] * Qs[:, 2]))
    return pr.sliced_sum(np.stack(cols, 1))


def stack_points(P, Q, usable, rig, cam_status=None, same=None):
    """The stack of camera-frame points P, Q [n_cams, ld, 3] and flags usable [n_cams, ld] -> (P' [n_cams * ld, 3], Q', flags,
    contributing [n_cams], worst status)."""
    P, Q = np.asarray(P, np.float64), np.asarray(Q, np.float64)
    usable = np.asarray(usable)
    n_cams, ld = usable.shape
    st = np.zeros(n_cams, np.int64) if cam_status is None else np.asarray(cam_status).reshape(n_cams)
    sm = np.zeros(n_cams, bool) if same is None else np.asarray(same).reshape(n_cams) != 0
    contrib = (st == OK) & ~sm
    Ps, Qs, fl = np.zeros((n_cams * ld, 3)), np.zeros((n_cams * ld, 3)), np.zeros(n_cams * ld, np.int32)
    for i in range(n_cams):
        if not contrib[i]:
            continue
        f = np.sign(usable[i]).astype(np.int32)
        us = f > 0
        rows = slice(i * ld, (i + 1) * ld)
        fl[rows] = f
        Ps[rows][us] = to_rig(P[i][us], *rig[i])
        Qs[rows][us] = to_rig(Q[i][us], *rig[i])
    return Ps, Qs, fl, contrib, int(st.max())


def pose_rig_law(P, Q, usable, rig, cam_status=None, lam=1.0, n_iter=0, sigma_min=0.0, same=None):
    """The law on given camera-frame points (the seam vitvs_op_pose_rig_law).  -> dict(v [6], status, R, t, info [8], weights
    [n_cams, ld], sigma, moments [18], gaps, edge): info = contributing cameras, usable rows, Jacobi sweeps of the last solve,
    re-weightings done, usable rows with final weight 0, degenerate flag, rows dropped for a hole, the largest camera status."""
    usable = np.asarray(usable)
    n_cams, ld = usable.shape
    Ps, Qs, fl, contrib, worst = stack_points(P, Q, usable, rig, cam_status, same)
    if not contrib.any():
        info = np.array([0, 0, 0, 0, 0, 0, 0, worst], np.int32)
        return dict(v=np.zeros(6), status=worst, R=np.eye(3), t=np.zeros(3), info=info, weights=np.zeros((n_cams, ld)), sigma=0.0,
                    moments=np.zeros(18), gaps=[], edge=np.inf)
    out = pr.pose_law(Ps, Qs, fl, lam, n_iter, sigma_min)
    i8 = out["info"]
    info = np.array([int(contrib.sum()), i8[0], i8[1], i8[2], i8[3], i8[4], i8[5], worst], np.int32)
    return dict(v=out["v"], status=out["status"], R=out["R"], t=out["t"], info=info, weights=out["weights"].reshape(n_cams, ld),
                sigma=out["sigma"], moments=moments(Ps, Qs, out["weights"]), gaps=out["gaps"], edge=out["edge"])


def pose_rig_from_details(det, cam_status, rig, K, tables, lam, n_iter, pitch_u, pitch_v):
    """The law through the handle (vitvs_pose_rig_velocity_dev) from ``Engine.last_details``' dict of the n_cams pairs.  ``K``
    [n_cams, 4]; ``tables`` [n_cams, T + 1] or [1, T + 1] (one goal depth for all)."""
    n_cams, ld = det["selected"].shape[:2]
    K = np.broadcast_to(np.asarray(K, np.float64).reshape(-1, 4), (n_cams, 4))
    tables = np.asarray(tables)
    P, Q, usable = np.zeros((n_cams, ld, 3)), np.zeros((n_cams, ld, 3)), np.zeros((n_cams, ld), np.int32)
    for i in range(n_cams):
        tab = tables[i if len(tables) > 1 else 0]
        P[i], Q[i], usable[i] = pr.points_from_details(det["selected"][i], det["s_uv"][i], det["feat"][i], det["info"][i, 1], K[i], tab)
    same = det["info"][:n_cams, 2] != 0
    st = np.asarray(cam_status).reshape(n_cams)
    contrib = (st == OK) & ~same
    sigma_min = 0.0
    us = (usable > 0) & contrib[:, None]
    if n_iter > 0 and us.any():
        pix = max(max(pitch_u / K[i, 0], pitch_v / K[i, 1]) for i in range(n_cams) if contrib[i])
        sigma_min = 0.5 * pix * pr.median_middle(Q[..., 2].reshape(-1)[us.reshape(-1)])
    out = pose_rig_law(P, Q, usable, rig, st, lam, n_iter, sigma_min, same)
    out["sigma_min"] = sigma_min
    return out


def twist_to_rig(v_c, R, t):
    """A camera twist in its own frame as the rig twist that produces it: the inverse of servo.twist_matrix(R, t)."""
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64)
    w = R @ v_c[3:]
    return np.concatenate([R @ v_c[:3] + np.cross(t, w), w])


def per_camera_average(P, Q, usable, rig, lam=1.0, n_iter=0, sigma_min=0.0):
    """NOT the law: the pose law per camera, each twist carried to the rig frame, the mean over the cameras whose law is OK.
    -> (v [6] or None when no camera solved, the cameras' statuses)."""
    vs, sts = [], []
    for i, (R, t) in enumerate(rig):
        out = pr.pose_law(P[i], Q[i], usable[i], lam, n_iter, sigma_min)
        sts.append(out["status"])
        if out["status"] == OK:
            vs.append(twist_to_rig(out["v"], R, t))
    return (np.mean(vs, 0) if vs else None), sts


# ---------------------------------------------------------------------------------------------- seeded rigs


def toe_in_rig(n_cams=3, spacing=0.15, toe_deg=10.0):
    """Cameras in a row along the rig's x axis, ``spacing`` apart, looking along +z, the outer ones turned about y towards the
    middle by ``toe_deg`` per position."""
    rig = []
    for i in range(n_cams):
        o = i - (n_cams - 1) / 2.0
        rig.append((pr.rodrigues(np.array([0.0, -np.radians(toe_deg) * o, 0.0])), np.array([spacing * o, 0.0, 0.0])))
    return rig


def seeded_rig(rng, n_cams):
    """Cameras up to 0.2 m from the rig origin, turned up to 0.5 rad about a random axis."""
    return [(pr.rodrigues(unit(rng.standard_normal(3)) * rng.uniform(0.0, 0.5)), rng.uniform(-0.2, 0.2, 3)) for _ in range(n_cams)]


def seeded_displacement(rng, angle=None, reach=0.1):
    """(R, t): the current rig in the goal rig's frame."""
    angle = rng.uniform(0.02, 0.3) if angle is None else angle
    return pr.rodrigues(unit(rng.standard_normal(3)) * angle), rng.uniform(-reach, reach, 3)


def camera_points(X_goal_rig, rig, R, t):
    """World points given in the goal rig's frame, [n_cams, ld, 3] (camera i sees X[i]) -> (P, Q): the current and the goal
    camera-frame points of every camera, with the current rig at pose (R, t) in the goal rig's frame."""
    X = np.asarray(X_goal_rig, np.float64)
    P, Q = np.zeros_like(X), np.zeros_like(X)
    for i, (Ri, ti) in enumerate(rig):
        Q[i] = (X[i] - ti) @ Ri                           # R_i^T (X - t_i)
        P[i] = (pr.points_in_camera(X[i], R, t) - ti) @ Ri
    return P, Q


def true_twist(R, t, lam):
    """The twist of the displacement itself (what an exact alignment returns)."""
    X = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    q = pr.horn(pr.points_in_camera(X, R, t), X, np.ones(4))["q"]
    return pr.twist(np.asarray(R, np.float64), np.asarray(t, np.float64), q, lam)


def outlier_case(seed, n_cams=3, rows=16, noise=0.002, n_out=6):
    """The "outliers concentrated in one camera" case: n_cams x rows pairs scattered 0.5 .. 1 m in front of a seeded rig, ``noise``
    metres of Gaussian noise on both clouds, ``n_out`` gross outliers of 0.1 .. 0.4 m, all in camera 0's current points.
    -> dict(P, Q, usable, rig, R, t, planted [n_out] rows of camera 0)."""
    rng = np.random.default_rng(7000 + seed)
    rig = seeded_rig(rng, n_cams)
    R, t = seeded_displacement(rng)
    X = np.concatenate([rng.uniform(-0.4, 0.4, (n_cams, rows, 2)), rng.uniform(0.5, 1.0, (n_cams, rows, 1))], 2)
    P, Q = camera_points(X, rig, R, t)
    P = P + noise * rng.standard_normal(P.shape)
    Q = Q + noise * rng.standard_normal(Q.shape)
    planted = rng.permutation(rows)[:n_out]
    for k in planted:
        P[0, k] += unit(rng.standard_normal(3)) * rng.uniform(0.1, 0.4)
    return dict(P=P, Q=Q, usable=np.ones((n_cams, rows), np.int32), rig=rig, R=R, t=t, planted=np.sort(planted))
