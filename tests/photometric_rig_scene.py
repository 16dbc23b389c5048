"""Test infrastructure (never shipped): the scene of the photometric rig law's closed loops, shared by
tests/test_photometric_rig_host.py (the fp64 reference on the CPU) and tests/test_gpu_photometric_rig_loop.py (the device).

tests/test_photometric_host.py's scene (synth.texture(128, 11) over 1.6 m, the plane 0.61 m away, 640 x 480) seen by a rig of three
cameras: yaw 0 / 20 / -15 degrees about the optical axis, at (-0.12, 0, 0), (0.12, 0.05, 0), (0, -0.1, 0.02) m in the rig frame.
The rig starts 1.5 cm / 2.2 degrees from its goal.  Every current frame of camera i is clip(round(g_i rgb + b_i)) with (g, b) =
(1.15, 8), (0.9, -5), (1.05, 12); then the columns [0, 384) of camera 0's frame (60 % of its view) are overwritten with 8 x 8
squares of random colours."""
import numpy as np

from planar_sim import rodrigues
import closed_loop as cl

PLANE_Z, SPAN, DT = 0.61, 1.6, 0.5
LEVEL, INTER, MU, LAM, UPDATES = 2, 1, 0.01, 0.5, 30
LIGHTS = ((1.15, 8.0), (0.9, -5.0), (1.05, 12.0))
COVERED = 384


def rig():
    yaw = np.deg2rad([0.0, 20.0, -15.0])
    t = ((-0.12, 0.0, 0.0), (0.12, 0.05, 0.0), (0.0, -0.1, 0.02))
    return [(rodrigues(np.array([0.0, 0.0, a])), np.array(p)) for a, p in zip(yaw, t)]


def start():
    axis = np.array([0.3, -0.4, 0.85])
    direction = np.array([0.6, -0.5, 0.6])
    return rodrigues(axis / np.linalg.norm(axis) * np.deg2rad(2.2)), direction / np.linalg.norm(direction) * 0.015


def light(rgb, i):
    g, b = LIGHTS[i]
    return np.clip(np.round(g * rgb.astype(np.float64) + b), 0, 255).astype(np.uint8)


def occluder(covered=COVERED):
    squares = np.random.default_rng(7).integers(0, 256, (60, 48, 3))
    return np.kron(squares, np.ones((8, 8, 1))).astype(np.uint8)[:, :covered]


def disturbed(rgb, i, covered=COVERED):
    """Camera i's current frame as the loops see it."""
    out = light(np.asarray(rgb), i)
    if i == 0 and covered:
        out[:, :covered] = occluder(covered)
    return out


def goals(scene, ext):
    """([goal frames], [goal depths]) of the cameras with the rig at its goal."""
    got = [scene.render(*cl.camera_pose(np.eye(3), np.zeros(3), e)) for e in ext]
    return [np.asarray(g[0]) for g in got], [np.asarray(g[1]) for g in got]


def frames(scene, ext, Rr, tr, covered=COVERED):
    return [disturbed(scene.render(*cl.camera_pose(Rr, tr, e))[0], i, covered) for i, e in enumerate(ext)]


def step(Rr, tr, v):
    """The rig moved by the rig-frame twist v for DT."""
    return Rr @ rodrigues(np.asarray(v[3:]) * DT), tr + Rr @ np.asarray(v[:3]) * DT
