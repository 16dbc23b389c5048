"""Closed loop on the GPU with the homography law's consensus start (``ServoParams(homography_consensus=256)``) over
fine texture, where a third of the matches of untrained-like tokens can be wrong.

The set-up of tests/test_gpu_homography_loop.py (ViT-S/16 224², synthetic weights, fp32, an RGB-only camera, ``selection="order"``,
generator seed 121, the 5 cm / 5 degree start, ``homography_depth`` = 0.61) over the scene of tests/test_gpu_robust_loop.py
(``synth.texture(512, 11)`` at 1.6 / 512 m per texel), 120 updates driven directly as that test drives them.  Three runs: 4 Tukey
re-weightings alone, the consensus start (256 hypotheses) with no re-weighting, and the consensus start with 4.

Asserted: no update aborts (``Controller.ibvs`` never raises), every camera status is in {0, 2, 3}, the law is OK in at least one
update, and the run with the consensus start and N = 4 ends below its 5 cm / 5 degree start.  No ratio between the runs is asserted:
nobody had measured these loops before this test was written.  The three end errors, the share of updates in which the law was OK
and the mean number of start weights at 1 are printed (DESIGN.md §5h quotes them)."""
import numpy as np
import pytest

import vitvs_amd  # noqa: F401
import closed_loop as cl

pytestmark = pytest.mark.gpu

UPDATES = 120
RUNS = {"N = 4 alone": (4, 0), "consensus 256, N = 0": (0, 256), "consensus 256, N = 4": (4, 256)}


def _run_loop(n_iter, consensus):
    eng, params, ctl, sim = cl.set_up(dict(law="homography", homography_depth=0.61, homography_robust_iterations=n_iter,
                                           homography_consensus=consensus), tex_px=512, sim_class=cl.RgbOnlyCameraSim,
                                      give_params=True, generator_seed=121)
    start_weights, usable = [], []
    law = eng.homography_velocity_host

    def recording_law(*args):
        v, info = law(*args)
        start_weights.append(int(info["start_weights"][0]))
        usable.append(int(info["usable"][0]))
        return v, info
    eng.homography_velocity_host = recording_law
    track, status, law_status, aborted = [cl.sim_pose_error(sim)], [], [], None
    for _ in range(UPDATES):
        sim.sense()
        try:
            ctl.ibvs()
        except RuntimeError as exc:                             # what loop.ServoLoop aborts an episode on
            aborted = str(exc)
            break
        status.append(ctl.last_status)
        law_status.append(ctl.last_homography_status)
        lin, ang = ctl.publish_twist()
        sim.apply_twist(lin, ang)
        track.append(cl.sim_pose_error(sim))
    depth_seen = ctl.latest_image_depth is not None or ctl.goal_depth is not None
    eng.close()
    return np.array(track), status, law_status, np.array(start_weights), np.array(usable), aborted, depth_seen


@pytest.mark.parametrize("run", sorted(RUNS))
def test_fine_texture_loop_with_the_consensus_start(run):
    n_iter, consensus = RUNS[run]
    track, status, law_status, start_weights, usable, aborted, depth_seen = _run_loop(n_iter, consensus)
    ok = sum(1 for s in law_status if s == 0)
    p0, r0 = track[0]
    print(f"closed loop fp32, fine texture, homography law, {run}: pose error (cm / deg) at updates 0, 10, .., {UPDATES}: "
          + "  ".join(f"{p:.2f}/{r:.2f}" for p, r in track[::10]) + f"; end {track[-1, 0]:.3f} cm / {track[-1, 1]:.3f} deg, highest "
          f"position error {track[:, 0].max():.2f} cm; law OK in {ok} of {len(law_status)} updates; usable rows per update: mean "
          f"{usable.mean() if len(usable) else 0:.2f}; start weights at 1: mean {start_weights.mean() if len(start_weights) else 0:.2f}")
    assert aborted is None, aborted
    assert len(status) == UPDATES and all(s in (0, 2, 3) for s in status), sorted(set(status))
    assert abs(p0 - 5.0) < 1e-9 and abs(r0 - 5.0) < 1e-6
    assert not depth_seen                                               # RGB only: no depth image, no goal depth
    assert all(s is not None for s in law_status) and ok > 0            # the law did drive the camera
    assert (start_weights > 0).any() == (consensus > 0)                 # the counter is 0 without a consensus start
    if run == "consensus 256, N = 4":
        assert track[-1, 0] < p0 and track[-1, 1] < r0
