"""Closed loop on the GPU with the hand-over of a ``MultiController(rig=...)`` to the photometric rig law.

tests/photometric_rig_scene.py's scene: three cameras on a rig, 1.5 cm / 2.2 degrees from the goal (inside the ViT laws' dead zone),
every camera under a lighting of its own and 60 % of camera 0's view covered.  ViT-S/16 224², synthetic weights, fp32, dt 0.5.
``photometric_handover`` is large enough that the first round (one batched ViT call and the rig law) hands over; the photometric rig
law (lambda 0.5, level 2, mu 0.01, the desired interaction matrix with each camera's goal depth) has the rig for the other 29 of
30 updates.

  * illumination on, 4 re-weightings: the hand-over happens behind update 0 and every photometric status is OK (no fall-back); the
    loop ends below 0.50 cm / 0.40 degrees, ten times the CPU reference's 0.050 / 0.040 (tests/test_photometric_rig_host.py), the
    room tests/test_gpu_photometric_loop.py leaves for the GPU renderer's fp32 sampling and the first, ViT, update; the gains of
    cameras 1 and 2 are within 0.01 of the planted 0.90 / 1.05;
  * illumination off, no re-weighting: the same loop ends above its start.

Measured (MI355X, profiles/photometric_rig.txt): 0.0548 cm / 0.0446 degrees after 30 updates (the CPU reference: 0.0497 / 0.0400; the
first update here is the ViT round's), gains 0.349 / 0.900 / 1.048 (camera 0's is the occluder's), sigma at its floor of 1, camera 0
with 92 % of its weight set aside; without the lighting model and the weights 14.78 cm / 12.06 degrees."""
import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib, config, servo, synth, weights
from planar_sim import PlanarScene
import closed_loop as cl
import photometric_rig_scene as rs

pytestmark = pytest.mark.gpu

KEY = "vits16_224"
HANDOVER = dict(photometric_handover=1e9, photometric_lambda=rs.LAM, photometric_level=rs.LEVEL, photometric_mu=rs.MU,
                photometric_interaction="desired")


def run_loop(illumination, robust_iterations, seed=121):
    """(track [updates + 1, 2] cm / degrees, the update of the hand-over or None, last_photometric of every photometric update)."""
    from vitvs_amd.engine import Engine
    cfg = config.baseline_config(KEY)
    params = config.ServoParams(dino_input_size=cfg.img_size, use_feature_binning=False, photometric_illumination=illumination,
                                photometric_robust_iterations=robust_iterations, **HANDOVER)
    eng = Engine(cfg, params, precision="fp32", max_pairs=3).load_state_dict(weights.synthetic_state_dict(cfg, 0))
    scene = PlanarScene(synth.texture(128, 11), rs.SPAN / 128, params, plane_z=rs.PLANE_Z, device="cuda")
    ext = rs.rig()
    goal_rgb, goal_depth = rs.goals(scene, ext)
    mc = servo.MultiController(eng, goal_rgb, params=params, selection="order", rig=ext, goal_depth=np.stack(goal_depth),
                               generator=torch.Generator().manual_seed(seed))
    Rr, tr = rs.start()
    track, handed, seen = [cl.rig_pose_error(Rr, tr)], None, []
    for it in range(rs.UPDATES):
        for i, e in enumerate(ext):
            rgb, depth = scene.render(*cl.camera_pose(Rr, tr, e))
            mc.image_callback_rgb(i, rs.disturbed(rgb, i))
            mc.image_callback_depth(i, depth)
        was = mc.photometric_active
        mc.ibvs()
        if mc.photometric_active and not was and handed is None:
            handed = it
        if was:
            seen.append(dict(mc.last_photometric))
        if mc.v_rig is not None:
            Rr, tr = rs.step(Rr, tr, mc.v_rig)
        track.append(cl.rig_pose_error(Rr, tr))
    eng.close()
    return np.array(track), handed, seen


def _show(name, track, handed, seen):
    print(f"closed loop fp32, photometric rig hand-over, {name}: pose error (cm / deg) at updates 0, 5, .., {rs.UPDATES}: "
          + "  ".join(f"{p:.4f}/{r:.4f}" for p, r in track[::5]))
    last = seen[-1]
    print(f"    hand-over behind update {handed}; the last update: gains {np.round(last['gain'], 4)}, biases {np.round(last['bias'], 3)}, sigma "
          f"{last['sigma']:.3f}, rejected {np.round(last['rejected'], 4)}, cost {last['cost']:.4f}, n {last['n']}")


def test_the_rig_hand_over_ends_at_the_goal_under_three_lightings_and_a_covered_camera():
    track, handed, seen = run_loop(True, 4)
    _show("illumination, N = 4", track, handed, seen)
    assert abs(track[0, 0] - 1.5) < 1e-9 and abs(track[0, 1] - 2.2) < 1e-6
    assert handed == 0
    assert len(seen) == rs.UPDATES - 1 and all(s["status"] == _lib.STATUS_OK for s in seen)
    assert track[-1, 0] < 0.50 and track[-1, 1] < 0.40
    last = seen[-1]
    assert last["cameras"] == [0, 1, 2] and abs(last["gain"][1] - 0.90) < 0.01 and abs(last["gain"][2] - 1.05) < 0.01


def test_without_the_lighting_model_and_the_weights_the_same_loop_leaves_the_goal():
    track, handed, seen = run_loop(False, 0)
    _show("no illumination, N = 0", track, handed, seen)
    assert handed == 0 and len(seen) > 0
    assert track[-1, 0] > track[0, 0]
