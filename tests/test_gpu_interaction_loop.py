"""Closed loop on the GPU with the three interaction matrices of the control law (option ``interaction``).

The set-up of tests/test_gpu_loop.py — ``ServoLoop(servo.Controller(Engine))`` driving a simulated camera over a textured plane
(tests/planar_sim.py), ViT-S/16 224², synthetic weights, ``selection="order"``, fp32, the 5 cm / 5 degree start — run three times:
the current law L(s, Z), the desired law L(s*, Z*) with the run-time depth image WITHHELD from the controller on every update (one
depth image rendered at the goal pose serves the whole run), and the mean of the two.  Each run must end through
``is_visual_servoing_done`` without an abort and take >= 90 % of the feature error away, the bar of the existing loop test.  No
pose-error ratio between the laws is asserted: none was measured before this test was written; the final pose errors are printed
(DESIGN.md §5c and profiles/interaction.txt quote them)."""
import numpy as np
import pytest

import vitvs_amd  # noqa: F401
import closed_loop as cl

pytestmark = pytest.mark.gpu


def _run_loop(interaction, withhold_depth):
    eng, params, ctl, sim = cl.set_up(dict(interaction=interaction), give_goal_depth=interaction != "current", generator_seed=121)

    def sense():
        sim.sense()
        if withhold_depth:
            ctl.latest_image_depth = None                 # no depth camera at run time
    feat_err = []
    status, = cl.record_ibvs(ctl, ["last_status"], also=lambda: feat_err.append(
        float(np.linalg.norm(eng.last_details(1)["L"][0, 6, :2 * params.num_pairs]))))
    res, sl, logs = cl.run_servo_loop(ctl, sim, sense)
    eng.close()
    return res, sl, logs, status, feat_err, len(ctl.velocity_vector_history)


@pytest.mark.parametrize("interaction,withhold_depth", [("current", False), ("desired", True), ("mean", False)])
def test_closed_loop_with_each_interaction_matrix(interaction, withhold_depth):
    res, sl, logs, status, feat_err, n_hist = _run_loop(interaction, withhold_depth)
    n = res.iteration_count if res is not None else 0
    assert res is not None and 300 <= n <= 360
    # ended by the convergence monitor (its velocity-window rule or the iteration cap), not by an abort or an exception
    assert ("Maximum iterations reached" in logs) != ("Velocity trend indicates convergence - checking final error" in logs)
    assert not any("Aborting" in m or "Error" in m for m in logs)
    assert all(s in (0, 2) for s in status), sorted(set(status))             # never NO_DEPTH: the desired law reads none
    assert n_hist == min(n, 200)                                             # every update moved the camera (none was skipped)
    start, end = float(np.mean(feat_err[:5])), float(np.mean(feat_err[-60:]))
    p0, r0 = sl.initial_error_translation, sl.initial_error_rotation
    print(f"closed loop fp32, interaction {interaction}{' (no run-time depth)' if withhold_depth else ''}: {n} updates, ended by "
          f"'{logs[-1]}'; feature error {start:.4f} -> {end:.4f} ({100 * (1 - end / start):.1f} % down), pose error {p0:.2f} cm / "
          f"{r0:.2f} deg -> {res.position_error:.3f} cm / {res.orientation_error:.3f} deg, lowest {res.lowest_position_error:.3f} cm / "
          f"{res.lowest_orientation_error:.3f} deg")
    assert abs(p0 - 5.0) < 1e-9 and abs(r0 - 5.0) < 1e-6
    assert end <= 0.1 * start                                               # >= 90 % of the feature error gone
