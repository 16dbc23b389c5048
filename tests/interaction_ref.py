"""Test infrastructure: the fp64 numpy statement of the three interaction matrices of the control law (option ``interaction``,
DESIGN.md §5c) and the quarter-turn case its tests share.  Like tests/robust_ref.py it is a reference, never shipped; it is built
on the oracle's pieces (oracle/servo_ref.py ``transform_to_real_world``, ``get_depth``, ``interaction_matrix``) and does not edit
them.

For feature pair k with current pixel (u, v), goal pixel (u*, v*), their normalised points (x, y), (xs, ys), Z = current depth at
(u, v) and Z* = goal depth at (u*, v*), both with get_depth's convention (mm -> m, 0 / out of bounds -> 100 m):

    current   L_k = rows(x, y, Z)                          the reference's law, ``servo_ref.velocity``
    desired   L_k = rows(xs, ys, Z*)                       the current depth is not needed
    mean      L_k = 0.5 * (rows(x, y, Z) + rows(xs, ys, Z*))   element by element

e = s - s* and v_c = -lambda pinv(L) e in every mode; zero-padded rows are pairs at pixel (0, 0) on both sides.  ``robust`` > 0
composes with tests/robust_ref.robust_velocity on the mode's L."""
from __future__ import annotations

import numpy as np

from oracle import servo_ref as sr
import robust_ref as rr

MODES = ("current", "desired", "mean")


def law(s_uv_star, s_uv, depth_mm, goal_depth_mm, K, lam: float, mode: str, robust: int = 0, s_min: float = 0.0, n_live=None) -> dict:
    """dict(L [2K, 6], e [2K, 1], Z [K, 1] or None, Z_goal [K, 1] or None, s_xy, s_star_xy, v_c [6]) plus, with ``robust`` > 0,
    ``rob`` = robust_velocity's result on that L (then v_c is the robust twist)."""
    assert mode in MODES
    fx, fy, cx, cy = K
    s_xy, s_star = sr.transform_to_real_world(s_uv, s_uv_star, fx, fy, cx, cy)
    e = (s_xy - s_star).reshape((len(s_xy) * 2, 1))
    Z = sr.get_depth(depth_mm, s_uv) if mode != "desired" else None
    Zs = sr.get_depth(goal_depth_mm, s_uv_star) if mode != "current" else None
    if mode == "current":
        L = sr.interaction_matrix(s_xy, Z)
    elif mode == "desired":
        L = sr.interaction_matrix(s_star, Zs)
    else:
        L = 0.5 * (sr.interaction_matrix(s_xy, Z) + sr.interaction_matrix(s_star, Zs))
    out = dict(L=L, e=e, Z=Z, Z_goal=Zs, s_xy=s_xy, s_star_xy=s_star)
    if robust:
        out["rob"] = rr.robust_velocity(L, e, lam, robust, s_min, n_live=n_live)
        out["v_c"] = out["rob"]["v_c"]
    else:
        out["v_c"] = (-lam * np.linalg.pinv(L) @ e).flatten()
    return out


# ----------------------------------------------------------------------------- a quarter turn about the optical axis
QUARTER = dict(g=14, n_pairs=24, depth_mm=610, lam=1.0)


def quarter_turn_tables(g: int = 14):
    """nn_1 of a current view turned a quarter turn about the optical axis: goal token (r, c) is seen at (c, g - 1 - r)."""
    idx = np.arange(g * g)
    r, c = idx // g, idx % g
    return (c * g + (g - 1 - r)).astype(np.int64)


def quarter_turn_case(u_max: int = 640, v_max: int = 480, g: int = 14) -> dict:
    """24 goal tokens spread over the 14 x 14 grid, both depths 0.61 m everywhere, fx = 0.9 u_max, fy = 0.9 v_max (the token grid is
    then square in normalised coordinates, so the permutation IS a quarter turn there), principal point at the centre, lambda = 1.
    ``nn_2`` is the inverse permutation except at three unselected tokens, so 0 < n_mutual < T."""
    t, img = g * g, 16 * g
    nn1 = quarter_turn_tables(g)
    ids = np.round(np.linspace(3, t - 4, QUARTER["n_pairs"])).astype(np.int32)
    nn2 = np.empty(t, np.int64)
    nn2[nn1] = np.arange(t)
    spoil = [j for j in (nn1[0], nn1[1], nn1[2])]
    assert not set(np.arange(3)) & set(ids.tolist())
    nn2[spoil] = (np.array([0, 1, 2]) + 50) % t                      # tokens 0, 1, 2 are no longer mutual
    K = (0.9 * u_max, 0.9 * v_max, u_max / 2, v_max / 2)
    depth = np.full((v_max, u_max), QUARTER["depth_mm"], np.uint16)
    s_star = rr.token_pixels(ids, g, img, u_max, v_max)
    s_cur = rr.token_pixels(nn1[ids], g, img, u_max, v_max)
    return dict(g=g, img=img, nn_1=nn1, nn_2=nn2, sim_1=np.full(t, 0.5, np.float32), ids=ids, K=K, depth=depth, goal_depth=depth.copy(),
                s_uv_star=s_star, s_uv=s_cur, lam=QUARTER["lam"])


def quarter_turn_laws(case: dict) -> dict:
    return {m: law(case["s_uv_star"], case["s_uv"], case["depth"], case["goal_depth"], case["K"], case["lam"], m) for m in MODES}


def quarter_turn_properties(vz_current: float, vz_desired: float, vz_mean: float) -> None:
    """What the mean matrix is for: the current and the desired law leave the axis in opposite directions, the mean stays."""
    assert vz_current * vz_desired < 0, (vz_current, vz_desired)
    assert abs(vz_mean) <= 0.05 * abs(vz_current), (vz_mean, vz_current)
