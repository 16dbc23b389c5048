"""Closed loop on the GPU with the robust rig law: the two-camera rig of tests/test_gpu_rig_loop.py (poses
and extrinsics: tests/closed_loop.py) over the FINE texture of tests/test_gpu_robust_loop.py (synth.texture at 512 px over 1.6 m),
whose nearest-neighbour matches under untrained weights contain gross outliers.  ViT-S/16 224², synthetic weights, fp32,
``selection="order"`` with a seeded generator (both laws see the same draws), the 5 cm / 5 degree start, 120 updates.
``MultiController(rig=...)`` drives the rig once with the plain rig law and once with ``rig_robust_iterations=4``.

Asserted: the robust run ends below its start error in position and in orientation, and no worse than the plain run in either.
Measured when this test was written: the plain rig law diverges, 44.38 cm / 11.54 degrees after 120 updates; the
robust rig law ends at 2.25 cm / 1.91 degrees, 0.051 / 0.165 of that.  The ratio bars are the geometric means of 1 and those
ratios (the margin the refine loop took over its measured ratio): position <= 0.226 x, orientation <= 0.407 x the plain run's."""
import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import config, servo, synth, weights
from planar_sim import PlanarScene, rodrigues
import closed_loop as cl

KEY = "vits16_224"
DT = 1.0
UPDATES = 120
PLANE_Z, TEX_PX, MPP = 0.61, 512, 1.6 / 512


def _run(robust_iterations, seed=121):
    from vitvs_amd.engine import Engine
    cfg = config.baseline_config(KEY)
    params = config.ServoParams(dino_input_size=cfg.img_size, use_feature_binning=False, rig_robust_iterations=robust_iterations)
    eng = Engine(cfg, params, precision="fp32", max_pairs=2).load_state_dict(weights.synthetic_state_dict(cfg, 0))
    scene = PlanarScene(synth.texture(TEX_PX, 11), MPP, params, plane_z=PLANE_Z, device="cuda")
    ext = cl.toed_in_pair()
    goals = [scene.render(*cl.camera_pose(np.eye(3), np.zeros(3), e))[0] for e in ext]
    mc = servo.MultiController(eng, goals, params=params, selection="order", rig=ext, generator=torch.Generator().manual_seed(seed))
    Rr, tr = cl.start_pose()
    track, zero_weights, reweighted = [cl.rig_pose_error(Rr, tr)], [], []
    for _ in range(UPDATES):
        for i, e in enumerate(ext):
            rgb, depth = scene.render(*cl.camera_pose(Rr, tr, e))
            mc.image_callback_rgb(i, rgb)
            mc.image_callback_depth(i, depth)
        mc.ibvs()
        if mc.rig_status == 0:
            reweighted.append(mc.rig_info.get("reweighted", 0))
            zero_weights.append(mc.rig_info.get("zero_weights", 0))
        if mc.v_rig is not None:
            tr = tr + Rr @ mc.v_rig[:3] * DT
            Rr = Rr @ rodrigues(mc.v_rig[3:] * DT)
        track.append(cl.rig_pose_error(Rr, tr))
    eng.close()
    return np.array(track), np.array(reweighted), np.array(zero_weights)


@pytest.mark.gpu
def test_fine_texture_rig_loop_under_the_robust_rig_law():
    plain, plain_n, _ = _run(0)
    robust, robust_n, zeros = _run(4)
    for name, tr in (("plain rig law ", plain), ("robust rig law", robust)):
        print(f"closed loop, two cameras on a rig, fine texture, {name}: pose error (cm / deg) at updates 0, 10, .., {UPDATES}: "
              + "  ".join(f"{p:.2f}/{r:.2f}" for p, r in tr[::10]) + f"; highest position error {tr[:, 0].max():.2f} cm")
    print(f"  robust / plain final error: position {robust[-1, 0] / plain[-1, 0]:.3f}, orientation {robust[-1, 1] / plain[-1, 1]:.3f}; "
          f"pairs of the rig with final weight 0 per update: mean {zeros.mean():.2f}, max {zeros.max()}")
    p0, r0 = robust[0]
    assert abs(p0 - 5.0) < 1e-9 and abs(r0 - 5.0) < 1e-6
    assert len(robust_n) > UPDATES // 2 and np.all(robust_n == 4) and np.all(plain_n == 0)
    assert robust[-1, 0] < p0 and robust[-1, 1] < r0
    assert robust[-1, 0] <= plain[-1, 0] and robust[-1, 1] <= plain[-1, 1]
    assert robust[-1, 0] <= 0.226 * plain[-1, 0] and robust[-1, 1] <= 0.407 * plain[-1, 1]
