"""Closed loop on the GPU with the hand-over to the TILE photometric law (``photometric_tiles``) under a cast shadow,
and the hand-back rule (``photometric_handback_rejected``).

The set-up of tests/test_gpu_photometric_robust_loop.py (ViT-S/16 224², fp32, the goal's depth image, dt 0.5, the start 1.5 cm / 2.2
degrees, ``photometric_handover`` large enough that the first ViT update hands over; level 2, mu 0.01, lambda 0.5, the desired
interaction matrix, illumination, 4 re-weightings) with a camera whose every frame is under "shadow"
(tests/photometric_tile_cases.py: 0.6 where column + 0.5 row < 380, about 45 % of the view), 40 updates.

  * ``photometric_tiles=(4, 4)``: every photometric status is OK, the loop ends below 0.32 cm / 0.26 degrees (ten times the CPU
    reference's 0.0316 / 0.0256), and the two regimes show in ``tile_gain``: tiles wholly inside the shadow are within 0.05 of 0.6,
    tiles wholly outside within 0.05 of 1.0;
  * ``photometric_tiles=(1, 1)``, the robust law: the same loop leaves twice its start error with every status OK;
  * with ``photometric_handback_rejected`` below that run's rejected share (half of its last update's) the controller hands back
    instead: the first step whose share is above it returns False with its status OK and the ViT update runs for that call.  Under
    this disturbance that is late: the robust law rejects no row for its first 30 updates (the test's docstring has the figures);
  * the rule where rows are rejected at once, the (4, 4) run: with the share below its first update's 7.95 % the first photometric
    step hands back; with the share above, nothing changes.

Measured (MI355X): see DESIGN.md 5n."""
import functools

import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib
import closed_loop as cl
import photometric_tile_cases as tc
from planar_sim import CameraSim, rodrigues

pytestmark = pytest.mark.gpu

UPDATES = 40
ROBUST = dict(photometric_handover=1e9, photometric_lambda=0.5, photometric_level=2, photometric_mu=0.01,
              photometric_interaction="desired", photometric_illumination=True, photometric_robust_iterations=4)


class ShadowedCameraSim(CameraSim):
    """A camera with a shadow cast over its view after the goal was taken."""

    def sense(self):
        rgb, self.last_depth = self.scene.render(self.R, self.t)
        self.last_rgb = tc.shadow(np.asarray(rgb))
        self.ctl.image_callback_rgb(self.last_rgb)
        self.ctl.image_callback_depth(self.last_depth)
        self.frames += 1


def run_loop(updates=UPDATES, stop_at=None, on_update=None, stop_on_handback=False, **more):
    """(track [.., 2] cm / degrees, the update of the hand-over or None, last_photometric of every photometric update, the tile
    law's ``tile_gain`` / ``tile_live`` of its calls, what every photometric step returned)."""
    eng, params, ctl, sim = cl.set_up({**ROBUST, **more}, "fp32", give_goal_depth=True, sim_class=ShadowedCameraSim)
    axis, direction = np.array([0.3, -0.4, 0.85]), np.array([0.6, -0.5, 0.6])
    sim.R = rodrigues(axis / np.linalg.norm(axis) * np.deg2rad(2.2))
    sim.t = direction / np.linalg.norm(direction) * 0.015
    torch.manual_seed(121)
    tiles, steps = [], []
    real_law, real_step = eng.photometric_tile_velocity, ctl._photometric_step

    def law(*a, **k):
        v, info = real_law(*a, **k)
        tiles.append((info["tile_gain"][0].copy(), info["tile_live"][0].copy()))
        return v, info

    def step():
        steps.append(real_step())
        return steps[-1]
    eng.photometric_tile_velocity, ctl._photometric_step = law, step
    forwards = []
    real_detect = ctl.detect_features

    def detect(*a, **k):                                        # the ViT update's first step in Controller.ibvs
        forwards.append(1)
        return real_detect(*a, **k)
    ctl.detect_features = detect
    track, handed, seen = [cl.sim_pose_error(sim)], None, []
    for it in range(updates):
        sim.sense()
        was = ctl.photometric_active
        before = len(forwards)
        ctl.ibvs()
        if on_update is not None:
            on_update(len(forwards) > before)                    # the ViT update ran in this call
        if ctl.photometric_active and not was and handed is None:
            handed = it
        if was:
            seen.append(dict(ctl.last_photometric))
        lin, ang = ctl.publish_twist()
        sim.apply_twist(lin, ang)
        track.append(cl.sim_pose_error(sim))
        if stop_at is not None and track[-1][0] > stop_at:
            break
        if stop_on_handback and steps and steps[-1] is False:
            break
    eng.close()
    return np.array(track), handed, seen, tiles, steps


@functools.lru_cache(maxsize=None)
def _tile_run():
    return run_loop(photometric_tiles=(4, 4))


def test_the_tile_hand_over_ends_at_the_goal_under_a_shadow():
    track, handed, seen, tiles, steps = _tile_run()
    print(f"closed loop fp32, tile photometric hand-over (4 x 4) under a shadow: pose error (cm / deg) at updates 0, 10, .., {UPDATES}: "
          + "  ".join(f"{p:.4f}/{r:.4f}" for p, r in track[::10]))
    last, (gains, live) = seen[-1], tiles[-1]
    print(f"hand-over behind update {handed}; the last update: sigma {last['sigma']:.3f}, rejected {last['rejected']:.4f}, dead tiles "
          f"{last['dead_tiles']}, gains {last['gain_min']:.4f} .. {last['gain_max']:.4f}, cost {last['cost']:.4f}, n {last['n']}\n{np.round(gains, 4)}")
    assert abs(track[0, 0] - 1.5) < 1e-9 and abs(track[0, 1] - 2.2) < 1e-6
    assert handed == 0 and steps == [True] * (UPDATES - 1)
    assert len(seen) == UPDATES - 1 and all(s["status"] == _lib.STATUS_OK for s in seen) and len(tiles) == UPDATES - 1
    assert track[-1, 0] < 0.32 and track[-1, 1] < 0.26
    inside = outside = 0
    for ty in range(4):                                          # tile (ty, tx): pixel rows [120 ty, 120 ty + 120), columns [160 tx, 160 tx + 160)
        for tx in range(4):
            if 160 * tx + 159 + 0.5 * (120 * ty + 119) < 380:
                assert live[ty, tx] and abs(gains[ty, tx] - 0.6) < 0.05, (ty, tx, gains[ty, tx])
                inside += 1
            elif 160 * tx + 0.5 * 120 * ty >= 380:
                assert live[ty, tx] and abs(gains[ty, tx] - 1.0) < 0.05, (ty, tx, gains[ty, tx])
                outside += 1
    assert inside >= 4 and outside >= 6


@functools.lru_cache(maxsize=None)
def _one_tile_run():
    return run_loop(photometric_tiles=(1, 1))


def test_one_tile_leaves_under_the_shadow():
    """The need: the same loop with ``photometric_tiles=(1, 1)``, the robust law, leaves twice its start error with every status
    OK: it is past 3 cm behind its first photometric update and goes on outward for all 40 updates."""
    track, handed, seen, tiles, steps = _one_tile_run()
    print("closed loop fp32, the robust law (1 x 1) under a shadow: pose error (cm / deg) at updates 0, 1, 2, 10, 20, 30, 40: "
          + "  ".join(f"{p:.4f}/{r:.4f}" for p, r in track[[0, 1, 2, 10, 20, 30, 40]]) + "; rejected per photometric update: "
          + " ".join(f"{s['rejected']:.4f}" for s in seen))
    assert handed == 0 and not tiles and len(seen) == UPDATES - 1 and all(s["status"] == _lib.STATUS_OK for s in seen) and all(steps)
    assert track[2, 0] > 2 * track[0, 0] and track[-1, 0] > 2 * track[0, 0]


def test_the_hand_back_rule_hands_the_one_tile_run_back():
    """With ``photometric_handback_rejected`` set below the (1, 1) run's rejected share (its last update's), the controller hands
    back instead: the first photometric step whose share is above it returns False with its status OK, and the ViT update runs for
    that call.  The share is half of the run's last one.

    It does so LATE, and that is the limit of the rule under this disturbance, not a fault of it: the two lighting regimes widen
    the median (sigma 27.6 grey levels at the first update, Tukey's cut at 129), so the robust law rejects NO row while it reads
    the shadow as motion.  On the CPU reference the share is 0.0000 for the first 30 updates (4.3 .. 42 cm away) and reaches 3.6 %
    at update 40 (46 cm); the rule catches what the weights see."""
    track, handed, seen, tiles, steps = _one_tile_run()
    shares = [s["rejected"] for s in seen]
    print("the (1, 1) run's rejected share per photometric update: " + " ".join(f"{r:.4f}" for r in shares))
    assert shares[-1] > 0
    share = 0.5 * shares[-1]
    at = next(i for i, r in enumerate(shares) if r > share)      # the first photometric update the rule objects to
    ran = []
    track2, handed2, seen2, _, steps2 = run_loop(photometric_tiles=(1, 1), photometric_handback_rejected=share, on_update=ran.append,
                                                 stop_on_handback=True)
    print(f"with photometric_handback_rejected {share:.4f} (half of the last share {shares[-1]:.4f}): handed back at photometric update "
          f"{at} of {len(shares)}, {track2[-1, 0]:.2f} cm / {track2[-1, 1]:.2f} degrees away")
    assert handed2 == 0 and steps2 == [True] * at + [False]
    assert seen2[at]["status"] == _lib.STATUS_OK and seen2[at]["rejected"] == shares[at] > share
    assert ran == [True] + [False] * at + [True]                 # update 0; the photometric updates; the ViT update behind the hand-back


def test_the_hand_back_rule_hands_back_where_rows_are_rejected():
    """The rule on the device: the (4, 4) run's first photometric update rejects 7.95 % of its rows; with the share at half of
    that, the same update's step returns False with its status OK, the hand-over is cleared and the ViT update runs for that call;
    with the share at twice that, the loop goes on as without the rule."""
    _, _, seen, _, _ = _tile_run()
    first = seen[0]["rejected"]
    assert 0.01 < first < 0.5
    ctl_calls = []
    _, handed, seen2, tiles2, steps2 = run_loop(updates=2, photometric_tiles=(4, 4), photometric_handback_rejected=0.5 * first,
                                                on_update=ctl_calls.append)
    print(f"the (4, 4) run's first rejected share {first:.4f}; with photometric_handback_rejected {0.5 * first:.4f} the photometric steps "
          f"returned {steps2}, the ViT updates ran {ctl_calls}")
    assert handed == 0 and steps2 == [False] and len(tiles2) == 1
    assert seen2[0]["status"] == _lib.STATUS_OK and seen2[0]["rejected"] == first
    assert ctl_calls == [True, True]                             # update 0, and update 1 behind the hand-back
    _, _, seen3, _, steps3 = run_loop(updates=3, photometric_tiles=(4, 4), photometric_handback_rejected=min(1.0, 2.0 * first))
    assert steps3 == [True, True] and [s["rejected"] for s in seen3] == [s["rejected"] for s in seen[:2]]
