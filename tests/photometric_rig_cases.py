"""Test infrastructure (never shipped): the cases of tests/test_gpu_photometric_rig_op.py, and their fp64 references, kept apart
from it so that tests/test_photometric_rig_host.py can check on the CPU what the device test relies on: that no case has to be
left out.

Inputs: tests/photometric_rig_scene.py's scene and rig with two more cameras, rendered ONCE on the CPU at 640 x 480 with the rig
0.3 cm / 0.4 degrees from its goal (a crop of a few dozen pixels is linear no further), every camera's current frame under a lighting
of its own.  A case crops every one of its cameras' frames at one origin (the principal point moved with it) and plants a block of
4 x 4 random squares over the left third of its first camera's crop.

A run is LEFT OUT of the exact comparisons of the median bin and of the rows of weight 0 when, in any re-weighting of the
reference, a row could land on the other side of a boundary on the device, whose residuals differ from the reference's in the last
digits (its twist is within 2e-10 of the reference's on such crops, the residuals of a few hundred grey levels at the most within
1e-7):
  the median bin   a row's 16 rho lies within EDGE bins of a bin edge (margin_e) AND the half count lies fewer than MARGIN_ROWS rows
                   inside its median bin (margin_m): no row near an edge means the same histogram, hence the same bin, wherever
                   the half count lies;
  the weight 0     a row's t lies within NEAR_T of 1 (margin_t).
The origins were chosen on the CPU, by a search over a grid of them, so that no run of any case is left out."""
import functools

import numpy as np

from vitvs_amd import config, servo, synth
import photometric_rig_ref as rg
import photometric_rig_scene as rs
import closed_loop as cl
from planar_sim import PlanarScene, rodrigues

MU, LAM, SMIN = 0.01, 0.5, 0.01          # sigma_min below the smallest scale a bin can give: sigma tells the median bin
MARGIN_ROWS, EDGE, NEAR_T = 3, 1e-5, 1e-7
PARAMS = config.ServoParams(dino_input_size=224, use_feature_binning=False)
START_CM, START_DEG = 0.3, 0.4
LIGHTS = rs.LIGHTS + ((0.95, 3.0), (1.1, -6.0))


def rig5():
    return rs.rig() + [(rodrigues(np.array([0.0, 0.0, np.deg2rad(35.0)])), np.array([0.1, -0.08, 0.0])),
                       (rodrigues(np.array([0.0, np.deg2rad(2.0), np.deg2rad(-30.0)])), np.array([-0.1, 0.09, 0.01]))]


@functools.lru_cache(maxsize=None)
def scene_frames():
    """(current frames, goal frames, goal depths, current depths) of the five cameras at 640 x 480."""
    sc = PlanarScene(synth.texture(128, 11), rs.SPAN / 128, PARAMS, plane_z=rs.PLANE_Z, device="cpu")
    ext = rig5()
    goal_rgb, goal_depth = rs.goals(sc, ext)
    axis, direction = np.array([0.3, -0.4, 0.85]), np.array([0.6, -0.5, 0.6])
    Rr = rodrigues(axis / np.linalg.norm(axis) * np.deg2rad(START_DEG))
    tr = direction / np.linalg.norm(direction) * START_CM / 100
    cur, depth = [], []
    for i, e in enumerate(ext):
        rgb, z = sc.render(*cl.camera_pose(Rr, tr, e))
        g, b = LIGHTS[i]
        cur.append(np.clip(np.round(g * rgb.astype(np.float64) + b), 0, 255).astype(np.uint8))
        depth.append(z)
    return cur, goal_rgb, goal_depth, depth


# name: (cameras, H, W, level, the crop's first row and column, depth: "z" / "holes" (the second camera all holes) / "scalar",
#        interaction, live or None)
CASES = {
    "2cam-24x32-l0": ((0, 1), 24, 32, 0, 40, 113, "z", 1, None),
    "3cam-41x54-l1": ((0, 1, 2), 41, 54, 1, 40, 325, "z", 1, None),               # 54 = 2 mod 4: byte-wide loads
    "5cam-24x32-l0": ((0, 1, 2, 3, 4), 24, 32, 0, 40, 378, "z", 1, None),         # wave 0 takes cameras 0 and 4
    "2cam-70x24-l0": ((1, 2), 70, 24, 0, 40, 60, "z", 1, None),                  # 70 bands: five chunks of 16, the last ragged
    "3cam-dead": ((0, 1, 2), 24, 32, 0, 40, 325, "z", 1, (1, 0, 1)),
    "3cam-holes": ((2, 0, 1), 24, 32, 0, 40, 272, "holes", 1, None),
    "2cam-scalar": ((1, 0), 24, 32, 0, 151, 537, "scalar", 0, None),
}
RUNS = [(name, illum, N) for name in CASES for illum in (1, 0) for N in (0, 1, 4)]


def block(shape):
    h, w = shape[0], shape[1] // 3
    squares = np.random.default_rng(7).integers(0, 256, (-(-h // 4), -(-w // 4), 3))
    return np.kron(squares, np.ones((4, 4, 1))).astype(np.uint8)[:h, :w]


@functools.lru_cache(maxsize=None)
def fixture(name, origin=None):
    """(cur [n, H, W, 3], des, Z [n, H, W] or None, depth_scale, K [n, 4], cVr [n, 6, 6], live or None) of a case."""
    cams, H, W, level, y0, x0, depth, inter, live = CASES[name]
    if origin is not None:
        y0, x0 = origin
    cur, goal, gdepth, cdepth = scene_frames()
    ext = rig5()
    cut = lambda img: np.ascontiguousarray(img[y0:y0 + H, x0:x0 + W])  # noqa: E731
    fx, fy, cx, cy = PARAMS.intrinsics()
    curs = np.stack([cut(cur[c]) for c in cams])
    curs[0, :, :W // 3] = block((H, W))
    dess = np.stack([cut(goal[c]) for c in cams])
    Z = np.stack([cut((gdepth if inter == 1 else cdepth)[c]) for c in cams])
    if depth == "holes":
        Z[1] = 0
    K = np.array([(fx, fy, cx - x0, cy - y0)] * len(cams))
    W6 = np.stack([servo.twist_matrix(*ext[c]) for c in cams])
    return curs, dess, (None if depth == "scalar" else Z), (0.61 if depth == "scalar" else 0.0), K, W6, live


@functools.lru_cache(maxsize=None)
def reference(name, illum, N, reverse=False, origin=None, smin=SMIN):
    cams, H, W, level, _, _, _, inter, _ = CASES[name]
    cur, des, Z, scalar, K, W6, live = fixture(name, origin)
    return rg.velocity(list(cur), list(des), None if Z is None else list(Z), scalar, K, W6, live, level, inter, MU, LAM, illum, N, smin,
                       reverse=reverse)


def left_out(ref):
    return (ref["margin_e"] < EDGE and ref["margin_m"] < MARGIN_ROWS) or ref["margin_t"] < NEAR_T
