"""Closed loop on the GPU with the homography law (``ServoParams(law="homography")``) and an RGB-only camera.

The set-up of tests/test_gpu_pose_loop.py — ``ServoLoop(servo.Controller(Engine))`` driving a simulated camera over a textured plane
(tests/planar_sim.py), ViT-S/16 224², synthetic weights, ``selection="order"``, fp32, the 5 cm / 5 degree start, at most 360
updates — run with the image-based law and a depth image (for the printed comparison only), the homography law and the homography
law with 4 Tukey re-weightings, ``homography_depth`` = 0.61.  The homography runs use a camera whose ``sense`` feeds RGB only: no
depth image and no goal depth ever reach the controller.  Each run must end through ``is_visual_servoing_done`` without an abort or
a skipped update, every update's camera status must be in {0, 2, 3}, the law must be OK in at least one update, and with N = 4 the
final position and orientation errors must be below their 5 cm / 5 degree start.  No ratio against the image-based run is asserted:
none was measured before this test was written; the final pose errors of all three are printed (DESIGN.md §5h quotes them)."""
import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import config, loop, servo, synth, weights
from planar_sim import CameraSim, PlanarScene, rodrigues

pytestmark = pytest.mark.gpu

KEY = "vits16_224"
DT = 0.5


class RgbOnlyCameraSim(CameraSim):
    """A plain RGB camera: the rendered depth image is thrown away."""

    def sense(self):
        self.last_rgb, _ = self.scene.render(self.R, self.t)
        self.last_depth = None
        self.ctl.image_callback_rgb(self.last_rgb)
        self.frames += 1


def _run_loop(law, n_iter):
    from vitvs_amd.engine import Engine
    cfg = config.baseline_config(KEY)
    params = config.ServoParams(dino_input_size=cfg.img_size, use_feature_binning=False, law=law, homography_robust_iterations=n_iter,
                                homography_depth=0.61)
    eng = Engine(cfg, params, precision="fp32", max_pairs=1).load_state_dict(weights.synthetic_state_dict(cfg, 0))
    scene = PlanarScene(synth.texture(128, 11), 1.6 / 128, params, plane_z=0.61, device="cuda")
    goal_rgb, _ = scene.render(np.eye(3), np.zeros(3))
    ctl = servo.Controller(eng, goal_image=goal_rgb, params=params, selection="order")
    ctl.generator = torch.Generator().manual_seed(121)
    axis = np.array([0.3, -0.4, 0.85])
    axis /= np.linalg.norm(axis)
    direction = np.array([0.6, -0.5, 0.6])
    direction /= np.linalg.norm(direction)
    sim_class = RgbOnlyCameraSim if law == "homography" else CameraSim
    sim = sim_class(scene, ctl, rodrigues(axis * np.deg2rad(5.0)), direction * 0.05, DT)
    status, law_status = [], []
    real_ibvs = ctl.ibvs

    def recording_ibvs():
        real_ibvs()
        status.append(ctl.last_status)
        law_status.append(ctl.last_homography_status)
    ctl.ibvs = recording_ibvs
    logs = []
    sl = loop.ServoLoop(ctl, np.zeros(3), np.array([0.0, 0.0, 0.0, 1.0]), get_pose=sim.get_pose, apply_twist=sim.apply_twist,
                        sense=sim.sense, max_iterations=360, log=logs.append)
    res = sl.run()
    depth_seen = ctl.latest_image_depth is not None or ctl.goal_depth is not None
    eng.close()
    return res, sl, logs, status, law_status, len(ctl.velocity_vector_history), depth_seen


@pytest.mark.parametrize("law,n_iter", [("ibvs", 0), ("homography", 0), ("homography", 4)])
def test_closed_loop_with_the_homography_law(law, n_iter):
    res, sl, logs, status, law_status, n_hist, depth_seen = _run_loop(law, n_iter)
    n = res.iteration_count if res is not None else 0
    assert res is not None and 300 <= n <= 360
    # ended by the convergence monitor (its velocity-window rule or the iteration cap), not by an abort or an exception
    assert ("Maximum iterations reached" in logs) != ("Velocity trend indicates convergence - checking final error" in logs)
    assert not any("Aborting" in m or "Error" in m for m in logs)
    assert all(s in (0, 2, 3) for s in status), sorted(set(status))
    assert n_hist == min(n, 200)                                             # every update moved the camera (none was skipped)
    p0, r0 = sl.initial_error_translation, sl.initial_error_rotation
    ok = sum(1 for s in law_status if s == 0)
    print(f"closed loop fp32, law {law}, N = {n_iter}: {n} updates, ended by '{logs[-1]}'; homography law OK in {ok} of "
          f"{len(law_status)}; pose error {p0:.2f} cm / {r0:.2f} deg -> {res.position_error:.3f} cm / {res.orientation_error:.3f} deg, "
          f"lowest {res.lowest_position_error:.3f} cm / {res.lowest_orientation_error:.3f} deg")
    assert abs(p0 - 5.0) < 1e-9 and abs(r0 - 5.0) < 1e-6
    if law == "homography":
        assert not depth_seen                                               # RGB only: no depth image, no goal depth
        assert all(s is not None for s in law_status)
        assert ok > 0                                                       # the law did drive the camera
    else:
        assert all(s is None for s in law_status)
    if law == "homography" and n_iter == 4:
        assert res.position_error < p0 and res.orientation_error < r0
