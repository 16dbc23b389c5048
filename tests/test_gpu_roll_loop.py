"""Closed loop on the GPU from a 95 degree roll, with and without the roll search (``ServoParams(roll_search=True)``).

The scene of tests/closed_loop.py (ViT-S/16 224², synthetic weights, ``synth.texture(px, 11)`` over 1.6 m, 0.61 m below the goal
pose) seen by a SQUARE camera (``u_max = v_max = 480``), the pose law with 4 Tukey re-weightings, ``selection="best"``, fp32.  The
start is ``closed_loop.start_pose()`` composed with a 95 degree roll about the optical axis.

Asserted (128-px texture, the search on) is only what exact geometry predicts: the first update's winner is k* = 3, and after 30
updates the orientation error is at most 0.75 of its start — the pose law removes lambda dt = 1.5 % of the rotation per update,
0.985^30 = 0.64, and the margin covers the lag of the EMA on the twist.  That keeps the asserted stretch above the 45 degree zone,
where two candidates tie.  Everything else is PRINTED, not asserted: the same start without the search, the errors after 360
updates of both, on the 128- and the 512-px texture (profiles/roll_search.txt and the README record them).  Whether the loop crosses
45 degrees cleanly on these weights was not known when this test was written."""
import numpy as np
import pytest

import vitvs_amd  # noqa: F401
from vitvs_amd import config, servo, synth, weights
from vitvs_amd.engine import Engine
import closed_loop as cl
from planar_sim import CameraSim, PlanarScene, rodrigues

pytestmark = pytest.mark.gpu

ROLL_DEG = 95.0
UPDATES_ASSERTED, UPDATES = 30, 360


def _set_up(roll_search, tex_px):
    cfg = config.baseline_config(cl.KEY)
    params = config.ServoParams(dino_input_size=cfg.img_size, use_feature_binning=False, u_max=480, v_max=480, law="pose",
                                pose_robust_iterations=4, roll_search=roll_search)
    eng = Engine(cfg, params, precision="fp32", max_pairs=4 if roll_search else 1)
    eng.load_state_dict(weights.synthetic_state_dict(cfg, 0))
    scene = PlanarScene(synth.texture(tex_px, 11), cl.SPAN / tex_px, params, plane_z=cl.PLANE_Z, device="cuda")
    goal_rgb, goal_depth = scene.render(np.eye(3), np.zeros(3))
    ctl = servo.Controller(eng, goal_image=goal_rgb, params=params, selection="best", goal_depth=goal_depth)
    R0, t0 = cl.start_pose()
    sim = CameraSim(scene, ctl, R0 @ rodrigues(np.array([0.0, 0.0, np.deg2rad(ROLL_DEG)])), t0, cl.DT)
    return eng, ctl, sim


@pytest.mark.parametrize("tex_px", [128, 512])
@pytest.mark.parametrize("roll_search", [True, False])
def test_closed_loop_from_a_95_degree_roll(roll_search, tex_px):
    eng, ctl, sim = _set_up(roll_search, tex_px)
    p0, r0 = cl.sim_pose_error(sim)
    assert abs(p0 - 5.0) < 1e-9 and 90.0 < r0 < 100.0, (p0, r0)
    rolls, at_30, ended = [], None, "ran all updates"
    for i in range(UPDATES):
        sim.sense()
        try:
            ctl.ibvs()
        except RuntimeError as exc:
            ended = f"stopped at update {i}: {exc}"
            break
        rolls.append(ctl.last_roll)
        if ctl.v_c is not None:
            sim.apply_twist(*ctl.publish_twist())
        if i + 1 == UPDATES_ASSERTED:
            at_30 = cl.sim_pose_error(sim)
    end = cl.sim_pose_error(sim)
    eng.close()
    at_30 = at_30 or (float("nan"), float("nan"))
    counts = {k: rolls.count(k) for k in sorted(set(rolls), key=str)}
    print(f"closed loop fp32, square camera, pose law N = 4, selection best, {tex_px}-px texture, roll search "
          f"{'on' if roll_search else 'off'}: start {p0:.2f} cm / {r0:.2f} deg; after {UPDATES_ASSERTED} updates "
          f"{at_30[0]:.3f} cm / {at_30[1]:.3f} deg; after {len(rolls)} updates {end[0]:.3f} cm / {end[1]:.3f} deg ({ended}); "
          f"winners {counts}")
    if roll_search:
        assert all(k is not None for k in rolls)
    else:
        assert all(k is None for k in rolls)
    if roll_search and tex_px == 128:
        assert rolls[0] == 3, rolls[:5]
        assert at_30[1] <= 0.75 * r0, (at_30, r0)
