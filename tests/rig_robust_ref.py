"""Test infrastructure: the fp64 numpy statement of the robust rig law, the law the kernel of rig.hip
(rig_robust_kernel) is tested against, and the planted-outlier rigs its tests share.  Built on ``rig_ref.stacked`` and written
like ``robust_ref.robust_velocity``, with a live mask over the stack instead of a live prefix.

A camera contributes when its status is 0, it has rows and a live pair.  M = stack_i(L_i W_i), e = stack_i(e_i) over the
contributing cameras in camera order; pair k of the stack is its rows 2k, 2k + 1; the first ``lives[i]`` pairs of camera i are
live, its other (zero-padded) pairs have weight 0 throughout:

  1. w_k = 1 on live pairs
  2. N times:  x = pinv(sqrt(W) M) sqrt(W) e                                     (np.linalg.pinv, rcond 1e-15)
               rho_k = || e_k - M_k x ||_2
               sigma = max(1.4826 * median(rho over ALL live pairs of ALL contributing cameras), s_min)     (np.median)
               t = rho_k / (4.6851 * sigma);  w_k = (1 - t^2)^2 if t < 1 else 0
  3. x from the last weights; v_rig = -lambda * x"""
import numpy as np

import rig_ref
from robust_ref import MAD_SCALE, TUKEY_C, weighted_solve

STATUS_OK = rig_ref.STATUS_OK


def contributing(Ls, statuses, lives):
    """Per camera: (rows, live pairs) it contributes, (0, 0) when it does not."""
    out = []
    for L, st, lv in zip(Ls, statuses, lives):
        rows = np.asarray(L).reshape(-1, 6).shape[0] & ~1
        lv = rows // 2 if lv is None else min(max(int(lv), 0), rows // 2)
        out.append((rows, lv) if int(st) == STATUS_OK and rows > 0 and lv > 0 else (0, 0))
    return out


def robust_rig_law(Ls, es, Ws, statuses, lives, lam, n_iter, s_min, trace=None):
    """-> (v_rig [6], w [pairs of the stack] final weights, rho last residuals (None when nothing ran), sigma (0.0 when no
    re-weighting ran), n_zero = pairs of the stack whose final weight is 0, padded ones included, margin = min over iterations
    and live pairs of |t - 1|, M, e).  ``lives``: live pairs per camera, None entries (or None) meaning all of them.  A list
    given as ``trace`` receives the sqrt(w)-scaled stack of every solve (for rig_ref.ldlt_margin: which solver each one takes)."""
    lives = [None] * len(Ls) if lives is None else list(lives)
    con = contributing(Ls, statuses, lives)
    use = [STATUS_OK if rows > 0 else 2 for rows, _ in con]
    M, e = rig_ref.stacked([np.asarray(L).reshape(-1, 6)[:rows] for L, (rows, _) in zip(Ls, con)],
                           [np.asarray(x).reshape(-1)[:rows] for x, (rows, _) in zip(es, con)], Ws, use)
    k = M.shape[0] // 2
    live = np.concatenate([np.zeros(0, bool)] + [np.arange(rows // 2) < lv for rows, lv in con if rows > 0])
    if k == 0:
        return np.zeros(6), np.zeros(0), None, 0.0, 0, np.inf, M, e
    w = live.astype(np.float64)
    rho, sigma, margin = None, 0.0, np.inf
    for _ in range(int(n_iter)):
        if trace is not None:
            trace.append(np.sqrt(np.repeat(w, 2))[:, None] * M)
        x = weighted_solve(M, e, w)
        res = (e - M @ x).reshape(k, 2)
        rho = np.sqrt(res[:, 0] ** 2 + res[:, 1] ** 2)
        sigma = max(MAD_SCALE * float(np.median(rho[live])), s_min)
        t = rho / (TUKEY_C * sigma)
        w = np.where(live & (t < 1.0), (1.0 - t * t) ** 2, 0.0)
        margin = min(margin, float(np.min(np.abs(t[live] - 1.0))))
    if trace is not None:
        trace.append(np.sqrt(np.repeat(w, 2))[:, None] * M)
    x = weighted_solve(M, e, w)
    return -lam * x, w, rho, sigma, int(np.count_nonzero(w == 0.0)), margin, M, e


def camera_weights(w, Ls, statuses, lives, stride):
    """The stack's weights as the kernel reports them: [n_cams][stride], 0 outside the pairs of contributing cameras."""
    lives = [None] * len(Ls) if lives is None else list(lives)
    out, o = np.zeros((len(Ls), stride)), 0
    for i, (rows, _) in enumerate(contributing(Ls, statuses, lives)):
        out[i, :rows // 2] = w[o:o + rows // 2]
        o += rows // 2
    return out


def planted(seed, pairs, n_out, smin=0.03, vscale=0.1):
    """A seeded rig of len(pairs) cameras whose errors follow one true rig twist v (the law's answer is -lam * v) up to
    +-0.3 smin of noise, with n_out[i] gross outliers (0.3 .. 0.8 in normalised coordinates) planted in camera i."""
    rng = np.random.default_rng(seed)
    Ws = [rig_ref.twist_matrix(*rig_ref.random_extrinsic(rng)) for _ in pairs]
    Ls = [rig_ref.camera_system(rng, p) for p in pairs]
    v = rng.standard_normal(6) * vscale
    es, outs = [], []
    for L, W, p, no in zip(Ls, Ws, pairs, n_out):
        e = L @ W @ v + rng.uniform(-0.3 * smin, 0.3 * smin, 2 * p)
        o = rng.choice(p, no, replace=False)
        for k in o:
            a = rng.uniform(0, 2 * np.pi); m = rng.uniform(0.3, 0.8)
            e[2 * k] += m * np.cos(a); e[2 * k + 1] += m * np.sin(a)
        es.append(e); outs.append(o)
    return Ls, es, Ws, v, outs          # the true rig twist is -lam * v


def rel_miss(v, v_true):
    return float(np.linalg.norm(np.asarray(v) - v_true) / np.linalg.norm(v_true))
