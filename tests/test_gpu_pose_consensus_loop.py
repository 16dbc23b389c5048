"""Closed loop on the GPU with the pose law's consensus start (``ServoParams(law="pose", pose_consensus=256)``).

The scene and settings of tests/test_gpu_pose_loop.py — ``ServoLoop(servo.Controller(Engine))`` over a textured plane, ViT-S/16 224²,
synthetic weights, ``selection="order"``, fp32, generator seed 121, the 5 cm / 5 degree start, one depth image rendered at the goal
pose as the goal depth — run three times: 4 Tukey re-weightings alone, the consensus start (256 hypotheses) with no re-weighting, and
the consensus start with 4.

Asserted for the two runs with the start: the law is OK in every update, and the run ends no farther from the goal than it began.
No ratio between the runs is asserted: nobody had measured these loops before this test was written.  The three final errors and the
mean number of rows starting at weight 1 are printed (DESIGN.md §5f quotes them)."""
import numpy as np
import pytest

import vitvs_amd  # noqa: F401
import closed_loop as cl

pytestmark = pytest.mark.gpu

RUNS = {"N = 4 alone": (4, 0), "consensus 256, N = 0": (0, 256), "consensus 256, N = 4": (4, 256)}


def _run_loop(n_iter, consensus):
    eng, _, ctl, sim = cl.set_up(dict(law="pose", pose_robust_iterations=n_iter, pose_consensus=consensus), give_params=True,
                                 give_goal_depth=True, generator_seed=121)
    start_weights, usable = [], []
    law = eng.pose_velocity_host

    def recording_law(*args):
        v, info = law(*args)
        start_weights.append(int(info["start_weights"][0]))
        usable.append(int(info["usable"][0]))
        return v, info
    eng.pose_velocity_host = recording_law
    status, pose_status = cl.record_ibvs(ctl, ["last_status", "last_pose_status"])
    res, sl, logs = cl.run_servo_loop(ctl, sim)
    eng.close()
    return res, sl, logs, status, pose_status, np.array(start_weights), np.array(usable)


@pytest.mark.parametrize("run", sorted(RUNS))
def test_closed_loop_with_the_consensus_start(run):
    n_iter, consensus = RUNS[run]
    res, sl, logs, status, pose_status, start_weights, usable = _run_loop(n_iter, consensus)
    n = res.iteration_count if res is not None else 0
    ok = sum(1 for s in pose_status if s == 0)
    p0, r0 = sl.initial_error_translation, sl.initial_error_rotation
    print(f"closed loop fp32, pose law, {run}: {n} updates, ended by '{logs[-1]}'; pose law OK in {ok} of {len(pose_status)}; pose error "
          f"{p0:.2f} cm / {r0:.2f} deg -> {res.position_error:.3f} cm / {res.orientation_error:.3f} deg, lowest "
          f"{res.lowest_position_error:.3f} cm / {res.lowest_orientation_error:.3f} deg; usable rows per update: mean "
          f"{usable.mean() if len(usable) else 0:.2f}; rows starting at weight 1: mean {start_weights.mean() if len(start_weights) else 0:.2f}")
    assert res is not None and not any("Aborting" in m or "Error" in m for m in logs)
    assert abs(p0 - 5.0) < 1e-9 and abs(r0 - 5.0) < 1e-6
    assert all(s is not None for s in pose_status) and ok > 0            # the law did drive the camera
    assert (start_weights > 0).any() == (consensus > 0)                  # the counter is 0 without a consensus start
    if consensus:
        assert ok == len(pose_status), [s for s in pose_status if s != 0]
        assert res.position_error <= p0 and res.orientation_error <= r0
