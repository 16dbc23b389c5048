"""Closed loop on the GPU with the outlier-robust control law, on the scene the plain law cannot servo.

The set-up of tests/test_gpu_loop.py (tests/closed_loop.py): ``servo.Controller(Engine)`` on ViT-S/16 224² with synthetic weights
driving a simulated camera (tests/planar_sim.py) from a 5 cm / 5 degree offset, ``selection="order"``, dt = 0.5 s — but over the FINE
texture (synth.texture at 512 px over 1.6 m) that test avoids: with untrained weights the nearest-neighbour matches of fine
texture contain gross outliers, and the least-squares law has no defence against them (the CPU oracle's plain law diverges to
20 cm on this scene, the robust law with 4 re-weightings ends at 2.5 cm / 1.9 degrees).  120 updates are driven directly with
``ServoParams(robust_iterations=4)``, fp32 and bf16:

  * the position error never exceeds 2 x the initial 5 cm (the reference's divergence abort, vitvs_v2.py:345-421);
  * after 120 updates position and orientation errors are <= 0.8 x their initial values (the bar of tests/test_gpu_loop.py);
  * the law did reject rows: the mean number of pairs per update with a final weight below 0.05 (``vitvs_last_weights``) is
    > 0 and < num_pairs / 2.

The same loop under the plain law (``robust_iterations=0``) runs beside it; its trajectory is printed (and recorded in
profiles/robust_law.txt), nothing is asserted on it."""
import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
import closed_loop as cl

pytestmark = pytest.mark.gpu

UPDATES = 120


def _run_loop(precision, robust_iterations):
    eng, params, ctl, sim = cl.set_up(dict(robust_iterations=robust_iterations), precision, tex_px=512)
    torch.manual_seed(121)          # the visiting orders come from torch's global RNG: both laws see the same draws (vitvs_v2.py:1397)
    track, rejected, info6 = [cl.sim_pose_error(sim)], [], []
    for _ in range(UPDATES):
        sim.sense()
        ctl.ibvs()
        if ctl.last_status == 0:
            w = eng.last_weights(1)[0, :params.num_pairs]
            rejected.append(int(np.count_nonzero(w < 0.05)))
            info6.append(int(eng.last_features(1)["info"][0, 6]))
        lin, ang = ctl.publish_twist()
        sim.apply_twist(lin, ang)
        track.append(cl.sim_pose_error(sim))
    eng.close()
    return np.array(track), np.array(rejected), np.array(info6), params


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_fine_texture_loop_holds_under_the_robust_law(precision):
    plain, _, plain6, _ = _run_loop(precision, 0)
    track, rejected, info6, params = _run_loop(precision, 4)
    for name, tr in (("plain ", plain), ("robust", track)):
        print(f"closed loop {precision}, fine texture, {name} law: pose error (cm / deg) at updates 0, 10, .., {UPDATES}: "
              + "  ".join(f"{p:.2f}/{r:.2f}" for p, r in tr[::10]) + f"; highest position error {tr[:, 0].max():.2f} cm")
    print(f"closed loop {precision}: pairs with weight < 0.05 per update: mean {rejected.mean():.2f}, max {rejected.max()} of "
          f"{params.num_pairs} ({len(rejected)} of {UPDATES} updates evaluated the law)")
    p0, r0 = track[0]
    assert abs(p0 - 5.0) < 1e-9 and abs(r0 - 5.0) < 1e-6
    assert np.all(info6 == 4) and np.all(plain6 == 0) and len(rejected) > UPDATES // 2
    assert track[:, 0].max() <= 2 * p0                                   # never at the divergence abort
    assert track[-1, 0] <= 0.8 * p0 and track[-1, 1] <= 0.8 * r0
    assert 0 < rejected.mean() < params.num_pairs / 2
