"""Closed loop on the GPU with the pose rig law: tests/test_gpu_rig_loop.py's two-camera rig, start pose and
scene, ``MultiController(law="pose", rig=..., goal_depth=...)`` with one goal depth per camera rendered at the goal; the rig
integrates the ONE twist of the 3-D alignment over both cameras' matches as a body twist (t += R v dt, R = R expm([w]x dt)).

ViT-S/16 224², synthetic weights, fp32, ``selection="order"`` with a seeded generator, at most 200 updates.  Asserted: the rig
status is OK or TOO_FEW throughout and the final rig pose error is below the 5 cm / 5 degree start in both parts.  The image-based
rig law runs on the same seed for the record and both ends are printed; no ratio between the two is asserted: none was
measured before this test was written."""
import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import config, servo, synth, weights
from planar_sim import PlanarScene, rodrigues
import closed_loop as cl

import test_gpu_rig_loop as base

SEED = 121


def _run_pose(seed=SEED):
    from vitvs_amd.engine import Engine
    cfg = config.baseline_config(base.KEY)
    params = config.ServoParams(dino_input_size=cfg.img_size, use_feature_binning=False, law="pose")
    eng = Engine(cfg, params.replace(law="ibvs"), precision="fp32", max_pairs=2).load_state_dict(weights.synthetic_state_dict(cfg, 0))
    scene = PlanarScene(synth.texture(base.TEX_PX, 11), base.MPP, params, plane_z=base.PLANE_Z, device="cuda")
    ext = cl.toed_in_pair()
    at_goal = [scene.render(*cl.camera_pose(np.eye(3), np.zeros(3), e)) for e in ext]
    goals = [g[0] for g in at_goal]
    goal_depth = np.stack([np.asarray(g[1].cpu() if torch.is_tensor(g[1]) else g[1]).astype(np.uint16) for g in at_goal])
    mc = servo.MultiController(eng, goals, params=params, selection="order", rig=ext, goal_depth=goal_depth,
                               generator=torch.Generator().manual_seed(seed))
    Rr, tr = cl.start_pose()
    start_pose = cl.rig_pose_error(Rr, tr)
    statuses = []
    for _ in range(base.UPDATES):
        for i, e in enumerate(ext):
            rgb, depth = scene.render(*cl.camera_pose(Rr, tr, e))
            mc.image_callback_rgb(i, rgb)
            mc.image_callback_depth(i, depth)
        mc.ibvs()
        statuses.append((mc.rig_status, [c.last_status for c in mc.cameras]))
        v = mc.v_rig
        if v is not None:
            tr = tr + Rr @ v[:3] * base.DT
            Rr = Rr @ rodrigues(v[3:] * base.DT)
    eng.close()
    return statuses, start_pose, cl.rig_pose_error(Rr, tr)


@pytest.mark.gpu
def test_closed_loop_two_cameras_one_pose_rig_twist():
    statuses, start_pose, end_pose = _run_pose()
    _, _, _, ibvs_end = base._run("rig", SEED)                       # the image-based rig law on the same seed, for the record
    print(f"closed loop, two cameras on a rig, {base.UPDATES} updates from {start_pose[0]:.2f} cm / {start_pose[1]:.2f} deg: pose rig "
          f"law ends at {end_pose[0]:.3f} cm / {end_pose[1]:.3f} deg; image-based rig law at {ibvs_end[0]:.3f} cm / {ibvs_end[1]:.3f} deg")
    assert all(rs in (0, 2) for rs, _ in statuses), sorted({(rs, tuple(c)) for rs, c in statuses})
    assert abs(start_pose[0] - 5.0) < 1e-9 and abs(start_pose[1] - 5.0) < 1e-6
    assert end_pose[0] < start_pose[0] and end_pose[1] < start_pose[1]
