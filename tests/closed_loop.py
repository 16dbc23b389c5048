"""The scaffold of the closed-loop tests (tests/test_gpu_*_loop.py): ``servo.Controller(Engine)`` on ViT-S/16 224² with synthetic
weights driving tests/planar_sim.py's camera over ``synth.texture(px, 11)`` spread over 1.6 m, 0.61 m below the goal pose, from
one fixed start 5 cm and 5 degrees away.  A test names its ``ServoParams``, precision and texture and says what it records."""
import numpy as np
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import config, loop, servo, synth, weights
from planar_sim import CameraSim, PlanarScene, quat_xyzw, rodrigues

KEY = "vits16_224"
DT = 0.5
PLANE_Z = 0.61
SPAN = 1.6                  # metres of plane under the texture, whatever its resolution


class RgbOnlyCameraSim(CameraSim):
    """A plain RGB camera: the rendered depth image is thrown away."""

    def sense(self):
        self.last_rgb, _ = self.scene.render(self.R, self.t)
        self.last_depth = None
        self.ctl.image_callback_rgb(self.last_rgb)
        self.frames += 1


def start_pose():
    axis = np.array([0.3, -0.4, 0.85])
    axis /= np.linalg.norm(axis)
    direction = np.array([0.6, -0.5, 0.6])
    direction /= np.linalg.norm(direction)
    return rodrigues(axis * np.deg2rad(5.0)), direction * 0.05


def sim_pose_error(sim):
    """(position error in cm, orientation error in degrees) against the goal pose (the world frame's origin)."""
    q = quat_xyzw(sim.R)
    return float(np.linalg.norm(sim.t) * 100), float(np.rad2deg(2 * np.arccos(min(1.0, abs(q[3])))))


def set_up(servo_params, precision="fp32", tex_px=128, sim_class=CameraSim, selection="order", give_params=False,
           give_goal_depth=False, generator_seed=None):
    """(eng, params, ctl, sim): the engine for ``ServoParams(**servo_params)``, the scene, a controller on the goal image (given
    the params and the goal's depth image only where asked, and a generator of its own where a seed is named) and the camera at
    the start pose.  The caller closes the engine."""
    from vitvs_amd.engine import Engine
    cfg = config.baseline_config(KEY)
    params = config.ServoParams(dino_input_size=cfg.img_size, use_feature_binning=False, **servo_params)
    eng = Engine(cfg, params, precision=precision, max_pairs=1).load_state_dict(weights.synthetic_state_dict(cfg, 0))
    scene = PlanarScene(synth.texture(tex_px, 11), SPAN / tex_px, params, plane_z=PLANE_Z, device="cuda")
    goal_rgb, goal_depth = scene.render(np.eye(3), np.zeros(3))
    ctl = servo.Controller(eng, goal_image=goal_rgb, params=params if give_params else None, selection=selection,
                           goal_depth=goal_depth if give_goal_depth else None)
    if generator_seed is not None:
        ctl.generator = torch.Generator().manual_seed(generator_seed)
    return eng, params, ctl, sim_class(scene, ctl, *start_pose(), DT)


def record_ibvs(ctl, attrs, also=None):
    """Wraps ``ctl.ibvs``: after every call each named attribute of the controller is appended to a list of its own (returned in
    the order of `attrs`), then `also()` runs."""
    lists = [[] for _ in attrs]
    real_ibvs = ctl.ibvs

    def recording_ibvs():
        real_ibvs()
        for name, seen in zip(attrs, lists):
            seen.append(getattr(ctl, name))
        if also is not None:
            also()
    ctl.ibvs = recording_ibvs
    return lists


def run_servo_loop(ctl, sim, sense=None):
    """``loop.ServoLoop.run()`` towards the goal pose, 360 iterations at the most: (result, the loop, its log records)."""
    logs = []
    sl = loop.ServoLoop(ctl, np.zeros(3), np.array([0.0, 0.0, 0.0, 1.0]), get_pose=sim.get_pose, apply_twist=sim.apply_twist,
                        sense=sense or sim.sense, max_iterations=360, log=logs.append)
    return sl.run(), sl, logs


# ----------------------------------------------------------------------------- the two-camera rig of the rig loops
def toed_in_pair():
    """Two cameras 16 cm apart on the rig's x axis, each toed in by 3 degrees about y (towards the other's side)."""
    toe = np.deg2rad(3.0)
    return [(rodrigues(np.array([0.0, toe, 0.0])), np.array([-0.08, 0.0, 0.0])),
            (rodrigues(np.array([0.0, -toe, 0.0])), np.array([0.08, 0.0, 0.0]))]


def camera_pose(Rr, tr, ext):
    Re, te = ext
    return Rr @ Re, Rr @ te + tr


def rig_pose_error(Rr, tr):
    return 100.0 * float(np.linalg.norm(tr)), float(np.rad2deg(np.arccos(np.clip((np.trace(Rr) - 1.0) / 2.0, -1.0, 1.0))))
