"""Test infrastructure: the fp64 numpy statement of the outlier-robust control law (option ``robust_law``) and
the planted-outlier scenarios its tests share.  Like tests/registers_ref.py it is a reference, never shipped; it imports the
oracle (oracle/servo_ref.py) and does not edit it.

The algorithm, on the ``L`` (2 rows per feature pair, 6 columns) and ``e`` of ``servo_ref.velocity``; the live rows are the
first ``n_live`` pairs, zero-padded pairs have weight 0:

  1. w_k = 1 for every live pair k
  2. N times:  x = pinv(sqrt(W) L) sqrt(W) e                      (np.linalg.pinv, rcond 1e-15, like the plain law)
               rho_k = || e_k - L_k x ||_2                        (the pair's two rows)
               sigma = max(1.4826 * median(rho over live pairs), sigma_min)      (np.median)
               t = rho_k / (4.6851 * sigma);  w_k = (1 - t^2)^2 if t < 1 else 0  (Tukey's biweight)
  3. x from the last weights; v_c = -lambda * x

sigma_min = 0.5 * max(pitch_u / fx, pitch_v / fy), pitch_u = stride * u_max / S, pitch_v = stride * v_max / S: half a patch
pitch in normalised image coordinates (the features are patch centres, so an inlier's residual is quantisation noise of that
size; the floor also keeps a converged loop, every residual 0, from dividing by zero)."""
from __future__ import annotations

import numpy as np
import torch

from oracle import servo_ref as sr

TUKEY_C = 4.6851
MAD_SCALE = 1.4826


def sigma_min(stride: int, u_max: int, v_max: int, input_size: int, fx: float, fy: float) -> float:
    pitch_u = stride * u_max / input_size
    pitch_v = stride * v_max / input_size
    return 0.5 * max(pitch_u / fx, pitch_v / fy)


def weighted_solve(L: np.ndarray, e: np.ndarray, w: np.ndarray) -> np.ndarray:
    sw = np.sqrt(np.repeat(w, 2))[:, None]
    return (np.linalg.pinv(sw * L) @ (sw * e.reshape(-1, 1))).flatten()


def robust_velocity(L, e, lam: float, n_iter: int, s_min: float, n_live=None) -> dict:
    """``L`` [2K, 6], ``e`` [2K] or [2K, 1] -> dict(v_c [6], w [K] final weights, rho [K] last residuals (None for
    n_iter == 0), sigma, n_zero = pairs whose final weight is 0, padded pairs included, margin)."""
    L = np.asarray(L, np.float64)
    e = np.asarray(e, np.float64).reshape(-1)
    k = L.shape[0] // 2
    n_live = k if n_live is None else int(n_live)
    w = np.zeros(k)
    w[:n_live] = 1.0
    rho, sigma, margin = None, None, np.inf
    for _ in range(int(n_iter)):
        x = weighted_solve(L, e, w)
        res = (e - L @ x).reshape(k, 2)
        rho = np.sqrt(res[:, 0] ** 2 + res[:, 1] ** 2)
        sigma = max(MAD_SCALE * float(np.median(rho[:n_live])), s_min)
        t = rho / (TUKEY_C * sigma)
        w = np.where(t < 1.0, (1.0 - t * t) ** 2, 0.0)
        w[n_live:] = 0.0
        margin = min(margin, float(np.min(np.abs(t[:n_live] - 1.0))))
    x = weighted_solve(L, e, w)
    # margin: the closest any live pair's t came to the rejection point 1 (the count of zero weights is not continuous there)
    return dict(v_c=-lam * x, w=w, rho=rho, sigma=sigma, n_zero=int(np.count_nonzero(w == 0.0)), margin=margin)


# ----------------------------------------------------------------------------- planted-outlier scenarios
def _rodrigues(w):
    th = float(np.linalg.norm(w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    return np.eye(3) + (np.sin(th) / th) * K + ((1.0 - np.cos(th)) / (th * th)) * (K @ K)


def token_pixels(ids, g: int, img: int, u_max: int, v_max: int) -> np.ndarray:
    """Camera pixel (u, v) of the tokens' patch centres, as the law computes them (oracle patch_centres + calculate_uv)."""
    ids = np.asarray(ids, np.int64)
    pts = sr.patch_centres(torch.from_numpy(np.stack([ids // g, ids % g], 1)), img, g)
    uv, _ = sr.calculate_uv(pts, pts, len(ids), u_max, v_max, img)
    return np.asarray(uv)


def planted_scenario(rng, n_pairs: int, outlier_share: float, params, K=None, g: int = 14, plane_z: float = 0.61,
                     holes: bool = False) -> dict:
    """A camera 5 cm and 5 degrees (random directions) away from the goal pose over a plane ``plane_z`` in front of the goal camera.
    Every token of the goal image is matched to the patch of the current image that contains its projection (clipped at
    the image border); ``n_pairs`` distinct goal tokens are drawn at random and ``round(outlier_share * n_pairs)`` of their matches
    replaced by uniformly random tokens.  Returns the arg-max tables the law's entry point takes (``nn_1`` with the planted
    outliers, ``nn_1_clean`` without; ``nn_2`` makes some but not all tokens mutual; ``sim_1`` = 0.5), the drawn ``ids``, the
    current camera's uint16 millimetre depth image (with the 100 m sentinel's holes when ``holes``), ``K`` and ``outliers``
    (positions in ``ids``)."""
    t, img = g * g, 16 * g
    fx, fy, cx, cy = K if K is not None else params.intrinsics()
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    direction = rng.normal(size=3)
    direction /= np.linalg.norm(direction)
    R, tr = _rodrigues(axis * np.deg2rad(5.0)), direction * 0.05            # X_goal = R X_cur + tr
    # goal tokens -> points of the plane -> current camera -> patch
    uv = token_pixels(np.arange(t), g, img, params.u_max, params.v_max).astype(np.float64)
    rays = np.stack([(uv[:, 0] - cx) / fx, (uv[:, 1] - cy) / fy, np.ones(t)], 1)
    X = rays * plane_z
    Xc = (X - tr) @ R                                                       # R^T (X - tr)
    u = fx * Xc[:, 0] / Xc[:, 2] + cx
    v = fy * Xc[:, 1] / Xc[:, 2] + cy
    col = np.clip(np.floor(u * img / params.u_max / 16), 0, g - 1).astype(np.int64)
    row = np.clip(np.floor(v * img / params.v_max / 16), 0, g - 1).astype(np.int64)
    nn1_clean = row * g + col
    ids = rng.choice(t, size=n_pairs, replace=False).astype(np.int32)
    n_out = int(round(outlier_share * n_pairs))
    outliers = rng.choice(n_pairs, size=n_out, replace=False)
    nn1 = nn1_clean.copy()
    nn1[ids[outliers]] = rng.integers(0, t, size=n_out)
    nn2 = np.zeros(t, np.int64)
    nn2[nn1] = np.arange(t)
    n_mutual = int(np.count_nonzero(nn2[nn1] == np.arange(t)))
    assert 0 < n_mutual < t
    # the current camera's depth image: every pixel's ray against the plane
    vv, uu = np.meshgrid(np.arange(params.v_max, dtype=np.float64), np.arange(params.u_max, dtype=np.float64), indexing="ij")
    rw = np.stack([(uu - cx) / fx, (vv - cy) / fy, np.ones_like(uu)], -1) @ R.T
    depth = np.clip(np.round((plane_z - tr[2]) / rw[..., 2] * 1000.0), 0, 65535).astype(np.uint16)
    if holes:
        depth.reshape(-1)[rng.integers(0, depth.size, size=depth.size // 7)] = 0
    return dict(nn_1=nn1, nn_1_clean=nn1_clean, nn_2=nn2, sim_1=np.full(t, 0.5, np.float32), ids=ids, depth=depth,
                K=(float(fx), float(fy), float(cx), float(cy)), outliers=outliers, g=g, img=img)


def oracle_law(sc: dict, params, nn1=None, n_live=None, rows=None) -> tuple:
    """(s_uv*, s_uv, servo_ref.velocity(...)) of a scenario's first ``n_live`` ids in a law of ``rows`` pairs (zero padding)."""
    g, img = sc["g"], sc["img"]
    nn1 = sc["nn_1"] if nn1 is None else nn1
    ids = np.asarray(sc["ids"], np.int64)
    ids = ids if n_live is None else ids[:n_live]
    rows = len(sc["ids"]) if rows is None else rows
    p1 = torch.from_numpy(np.stack([ids // g, ids % g], 1))
    p2 = torch.from_numpy(np.stack([nn1[ids] // g, nn1[ids] % g], 1))
    s_star, s_ = sr.calculate_uv(sr.patch_centres(p1, img, g), sr.patch_centres(p2, img, g), rows, params.u_max, params.v_max, img)
    K = sc["K"]
    return np.asarray(s_star), np.asarray(s_), sr.velocity(s_star, s_, sc["depth"], K[0], K[1], K[2], K[3], params.lambda_)


# The two configurations of the planted-outlier property (pairs, outlier share, first seed) and their scenarios; measured in
# tests/test_robust_host.py
PROPERTY_CONFIGS = [(48, 0.125, 6000), (130, 0.25, 13000)]
N_SCENARIOS = 64


def property_scenarios(n_pairs: int, share: float, seed0: int, params):
    """N_SCENARIOS seeded (scenario, plain law on the un-corrupted matches); seeds whose clean twist is zero are skipped here."""
    out, seed = [], seed0
    while len(out) < N_SCENARIOS:
        sc = planted_scenario(np.random.default_rng(seed), n_pairs, share, params)
        seed += 1
        clean = oracle_law(sc, params, nn1=sc["nn_1_clean"])[2]
        if np.any(clean["v_c"]):
            out.append((sc, clean))
    return out


def rel_l2(a, b) -> float:
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))
