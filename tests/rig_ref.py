"""The rig law in fp64 numpy: the statement the kernel of rig.hip is tested against.

Camera i of a rigid rig has pose (R_i, t_i) in the rig frame, X_rig = R_i X_cam + t_i.  A rig twist v_r = (v, w), expressed in the
rig frame, moves camera i with the twist v_ci = W_i v_r in its own optical frame, W_i = [[R_i^T, -R_i^T [t_i]x], [0, R_i^T]].  With
L_i (rows x 6) and e_i what the camera's law built,

    M = stack_i(L_i W_i),  e = stack_i(e_i),  v_r = -lambda pinv(M) e        (numpy.linalg.pinv, rcond = 1e-15)

over the cameras whose status is 0.  ``averaged_law`` is the obvious alternative a user would write on the host — every camera's own
pseudo-inverse twist mapped back to the rig frame, then the mean — which is not the least-squares solution of the stack."""
import numpy as np

from homography_ref import rodrigues  # noqa: F401
from solve_ref import THRESHOLD

STATUS_OK, STATUS_NO_CORRESPONDENCE, STATUS_TOO_FEW, STATUS_NO_DEPTH = 0, 1, 2, 3


def skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def twist_matrix(R, t):
    R = np.asarray(R, np.float64).reshape(3, 3)
    t = np.asarray(t, np.float64).reshape(3)
    W = np.zeros((6, 6))
    W[:3, :3] = R.T
    W[:3, 3:] = -R.T @ skew(t)
    W[3:, 3:] = R.T
    return W


def stacked(Ls, es, Ws, statuses):
    """(M [rows, 6], e [rows]) over the contributing cameras, in camera order; (0 x 6, 0) when none contributes."""
    Ms, ee = [np.zeros((0, 6))], [np.zeros(0)]
    for L, e, W, st in zip(Ls, es, Ws, statuses):
        L = np.asarray(L, np.float64).reshape(-1, 6)
        if int(st) == STATUS_OK and L.shape[0] > 0:
            Ms.append(L @ np.asarray(W, np.float64).reshape(6, 6))
            ee.append(np.asarray(e, np.float64).reshape(-1))
    return np.concatenate(Ms), np.concatenate(ee)


def rig_law(Ls, es, Ws, statuses, lam):
    """dict(v_rig [6], status, M, e, cameras, rows, G, g): status 0 when a camera contributed, else the largest camera status."""
    M, e = stacked(Ls, es, Ws, statuses)
    used = sum(1 for L, st in zip(Ls, statuses) if int(st) == STATUS_OK and np.asarray(L).reshape(-1, 6).shape[0] > 0)
    out = dict(M=M, e=e, cameras=used, rows=M.shape[0], G=M.T @ M, g=M.T @ e)
    if M.shape[0] == 0:
        out.update(v_rig=np.zeros(6), status=max([int(s) for s in statuses] + [0]))
        return out
    out.update(v_rig=-lam * (np.linalg.pinv(M, rcond=1e-15) @ e), status=STATUS_OK)
    return out


def averaged_law(Ls, es, Ws, statuses, lam):
    """The mean over the contributing cameras of inv(W_i) v_ci, v_ci = -lambda pinv(L_i) e_i the camera's own twist."""
    vs = []
    for L, e, W, st in zip(Ls, es, Ws, statuses):
        L = np.asarray(L, np.float64).reshape(-1, 6)
        if int(st) == STATUS_OK and L.shape[0] > 0:
            v_c = -lam * (np.linalg.pinv(L, rcond=1e-15) @ np.asarray(e, np.float64).reshape(-1))
            vs.append(np.linalg.solve(np.asarray(W, np.float64).reshape(6, 6), v_c))
    return np.mean(vs, axis=0) if vs else np.zeros(6)


def normal_packed(M, e):
    """The 28 doubles the kernel reports: G = M^T M upper triangle row-major (21), g = M^T e (6), the rows."""
    G, g = M.T @ M, M.T @ e
    return np.concatenate([G[np.triu_indices(6)], g, [float(M.shape[0])]])


def ldlt_margin(M):
    """The LDL^T pivots of G = M^T M relative to the kernel's test d > THRESHOLD G_jj: min_j d_j / (THRESHOLD G_jj) in fp64 (solve.h
    restated).  > 1: every pivot passes (the LDL^T path); a failing factorisation returns the ratio of its first failing pivot
    (<= 1; 0 for a zero or negative one).  A case is only a fair test of a path when this is >= 100 or <= 0.01."""
    G = M.T @ M
    Lf, dpiv, worst = np.zeros((6, 6)), np.zeros(6), np.inf
    for j in range(6):
        d = G[j, j] - sum(Lf[j, k] ** 2 * dpiv[k] for k in range(j))
        if not G[j, j] > 0:
            return 0.0
        ratio = d / (THRESHOLD * G[j, j])
        if ratio <= 1.0:
            return max(float(ratio), 0.0)
        worst = min(worst, ratio)
        dpiv[j] = d
        for i in range(j + 1, 6):
            Lf[i, j] = (G[i, j] - sum(Lf[i, k] * Lf[j, k] * dpiv[k] for k in range(j))) / d
    return float(worst)


def point_rows(x, y, Z):
    """The two interaction-matrix rows of a normalised image point (x, y) at depth Z (vitvs_v2.py:650-659)."""
    return np.array([[-1.0 / Z, 0.0, x / Z, x * y, -(1.0 + x * x), y],
                     [0.0, -1.0 / Z, y / Z, 1.0 + y * y, -(x * y), -x]])


def random_extrinsic(rng, angle=0.6, baseline=0.3):
    return rodrigues(rng.uniform(-angle, angle, 3)), rng.uniform(-baseline, baseline, 3)


def camera_system(rng, pairs):
    """L (2 pairs x 6) of `pairs` random points in view: x, y in +-0.4, Z in 0.5 .. 1.5 m."""
    return np.concatenate([point_rows(rng.uniform(-0.4, 0.4), rng.uniform(-0.4, 0.4), rng.uniform(0.5, 1.5)) for _ in range(pairs)])


def scenario(seed, n_cams=3, pairs=2):
    """A seeded rig: n_cams cameras with random extrinsics, `pairs` feature pairs each, and the errors e_i = L_i W_i v* of a
    true rig twist v* (so that -lambda pinv(M) e = -lambda v* exactly when M has full column rank)."""
    rng = np.random.default_rng(seed)
    Ws = [twist_matrix(*random_extrinsic(rng)) for _ in range(n_cams)]
    Ls = [camera_system(rng, pairs) for _ in range(n_cams)]
    v_star = rng.standard_normal(6)
    es = [L @ W @ v_star for L, W in zip(Ls, Ws)]
    return Ls, es, Ws, v_star


def statuses(case):
    """What the rig kernels report per camera of a case: 0 with rows, 2 (too few) without."""
    return [0 if L.shape[0] > 0 else 2 for L in case["Ls"]]
