"""Closed loop on the GPU with the homography law (``ServoParams(law="homography")``) and an RGB-only camera.

The set-up of tests/test_gpu_pose_loop.py — ``ServoLoop(servo.Controller(Engine))`` driving a simulated camera over a textured plane
(tests/planar_sim.py), ViT-S/16 224², synthetic weights, ``selection="order"``, fp32, the 5 cm / 5 degree start, at most 360
updates — run with the image-based law and a depth image (for the printed comparison only), the homography law and the homography
law with 4 Tukey re-weightings, ``homography_depth`` = 0.61.  The homography runs use a camera whose ``sense`` feeds RGB only: no
depth image and no goal depth ever reach the controller.  Each run must end through ``is_visual_servoing_done`` without an abort or
a skipped update, every update's camera status must be in {0, 2, 3}, the law must be OK in at least one update, and with N = 4 the
final position and orientation errors must be below their 5 cm / 5 degree start.  No ratio against the image-based run is asserted:
none was measured before this test was written; the final pose errors of all three are printed (DESIGN.md §5h quotes them)."""
import pytest

import vitvs_amd  # noqa: F401
from planar_sim import CameraSim
import closed_loop as cl

pytestmark = pytest.mark.gpu


def _run_loop(law, n_iter):
    eng, _, ctl, sim = cl.set_up(dict(law=law, homography_robust_iterations=n_iter, homography_depth=0.61),
                                 sim_class=cl.RgbOnlyCameraSim if law == "homography" else CameraSim, give_params=True,
                                 generator_seed=121)
    status, law_status = cl.record_ibvs(ctl, ["last_status", "last_homography_status"])
    res, sl, logs = cl.run_servo_loop(ctl, sim)
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
