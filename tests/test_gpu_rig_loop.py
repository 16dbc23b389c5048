"""Closed loop on the GPU with the rig law: two cameras on one rigid rig see the textured plane of
tests/planar_sim.py, each through ``render(R, t)`` at rig pose o extrinsic; ``MultiController(rig=...)`` turns the two cameras'
systems into ONE rig twist per round, and the rig integrates it as a body twist (t += R v dt, R = R expm([w]x dt)).

ViT-S/16 224², synthetic weights, fp32, ``selection="order"`` with a seeded generator, the 5 cm / 5 degree start of the existing
loop tests applied to the rig, a 16 cm baseline with 3 degrees of toe-in per camera.  At most 200 updates.  Asserted: the existing
loop tests' bar, feature error down >= 90 % for BOTH cameras, and a final rig pose error below the start.  Driving the rig from
camera 0's twist alone, mapped back to the rig frame (``_run("camera0")``), is what a user without the law would do; it is run for
the record (DESIGN.md §5d quotes it) and no ratio between the two is asserted: none was measured before this test was written."""
import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import config, servo, synth, weights
from planar_sim import PlanarScene, rodrigues
import closed_loop as cl

KEY = "vits16_224"
DT = 1.0
UPDATES = 200
PLANE_Z, TEX_PX, MPP = 0.61, 128, 1.6 / 128


def _footprint(params, R, t):
    """Where the four image corners' rays meet the plane, in texture pixels."""
    out = []
    for u, v in ((0, 0), (params.u_max - 1, 0), (0, params.v_max - 1), (params.u_max - 1, params.v_max - 1)):
        ray = R @ np.array([(u - params.c_x) / params.f_x, (v - params.c_y) / params.f_y, 1.0])
        s = (PLANE_Z - t[2]) / ray[2]
        X = t + s * ray
        out.append((X[0] / MPP + (TEX_PX - 1) / 2.0, X[1] / MPP + (TEX_PX - 1) / 2.0))
    return np.array(out)


def test_both_views_stay_on_the_texture_at_the_start_and_goal_poses():
    params = config.ServoParams(dino_input_size=224, use_feature_binning=False)
    for Rr, tr in ((np.eye(3), np.zeros(3)), cl.start_pose()):
        for ext in cl.toed_in_pair():
            fp = _footprint(params, *cl.camera_pose(Rr, tr, ext))
            assert (fp >= 0).all() and (fp <= TEX_PX - 1).all(), fp


def _run(mode="rig", seed=121):
    """mode "rig": the rig integrates MultiController.v_rig; "camera0": camera 0's smoothed twist mapped back, inv(W_0) v_c0."""
    from vitvs_amd.engine import Engine
    cfg = config.baseline_config(KEY)
    params = config.ServoParams(dino_input_size=cfg.img_size, use_feature_binning=False)
    eng = Engine(cfg, params, precision="fp32", max_pairs=2).load_state_dict(weights.synthetic_state_dict(cfg, 0))
    scene = PlanarScene(synth.texture(TEX_PX, 11), MPP, params, plane_z=PLANE_Z, device="cuda")
    ext = cl.toed_in_pair()
    goals = [scene.render(*cl.camera_pose(np.eye(3), np.zeros(3), e))[0] for e in ext]
    mc = servo.MultiController(eng, goals, selection="order", rig=ext, generator=torch.Generator().manual_seed(seed))
    W0 = servo.twist_matrix(*ext[0])
    Rr, tr = cl.start_pose()
    start_pose = cl.rig_pose_error(Rr, tr)
    feat_err, statuses = [], []
    for _ in range(UPDATES):
        for i, e in enumerate(ext):
            rgb, depth = scene.render(*cl.camera_pose(Rr, tr, e))
            mc.image_callback_rgb(i, rgb)
            mc.image_callback_depth(i, depth)
        mc.ibvs()
        L = eng.last_details(2)["L"]
        feat_err.append([float(np.linalg.norm(L[i, 6, :2 * params.num_pairs])) for i in range(2)])
        statuses.append((mc.rig_status, [c.last_status for c in mc.cameras]))
        v = mc.v_rig if mode == "rig" else (None if mc.cameras[0].v_c is None else np.linalg.solve(W0, mc.cameras[0].v_c))
        if v is not None:
            tr = tr + Rr @ v[:3] * DT
            Rr = Rr @ rodrigues(v[3:] * DT)
    eng.close()
    return np.array(feat_err), statuses, start_pose, cl.rig_pose_error(Rr, tr)


@pytest.mark.gpu
def test_closed_loop_two_cameras_one_rig_twist():
    feat_err, statuses, start_pose, end_pose = _run("rig")
    assert all(rs == 0 and all(s in (0, 2) for s in cams) for rs, cams in statuses), sorted({(rs, tuple(c)) for rs, c in statuses})
    start, end = feat_err[:5].mean(axis=0), feat_err[-60:].mean(axis=0)
    print(f"closed loop, two cameras on a rig, rig law: {UPDATES} updates; feature error camera 0 {start[0]:.4f} -> {end[0]:.4f}, "
          f"camera 1 {start[1]:.4f} -> {end[1]:.4f}; rig pose error {start_pose[0]:.2f} cm / {start_pose[1]:.2f} deg -> "
          f"{end_pose[0]:.3f} cm / {end_pose[1]:.3f} deg")
    assert abs(start_pose[0] - 5.0) < 1e-9 and abs(start_pose[1] - 5.0) < 1e-6
    assert (end <= 0.1 * start).all()                                  # >= 90 % of the feature error gone, for both cameras
    assert end_pose[0] < start_pose[0] and end_pose[1] < start_pose[1]
