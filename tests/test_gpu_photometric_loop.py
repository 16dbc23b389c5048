"""Closed loop on the GPU with the hand-over to the photometric law (``photometric_handover``).

The set-up of tests/closed_loop.py with ``subpatch`` on, fp32 and the goal's depth image: ``servo.Controller(Engine)`` on ViT-S/16
224² with synthetic weights driving tests/planar_sim.py's camera over synth.texture(128, 11) from 5 cm / 5 degrees, selection
"order", dt 0.5, torch seed 121.  At most 120 updates, twice: as it is (the yardstick: the loop ends in the dead zone of one patch
pitch), and with ``photometric_handover`` = THRESHOLD, ``photometric_lambda`` 0.5, level 2, mu 0.01 and the desired interaction
matrix (the settings of the CPU prototype; the ViT law keeps the reference's gain 0.03).

  * the hand-over happens, behind update HANDED = 37 (asserted), and the photometric law keeps the robot from there on (its status stays
    OK: no fall-back);
  * up to the hand-over the two runs are the same run;
  * the run with the hand-over ends at less than ONE TENTH of the position AND of the orientation error of the run without it.
    The CPU reference (tests/test_photometric_host.py) predicts a factor above 100; ten leaves room for the GPU renderer's fp32
    sampling.

THRESHOLD: max |raw v_c| / lambda_ is the ViT law's own estimate of what is left, in metres / radians; with a random visiting
order per update it jitters between 0.03 and 0.1 on the way in, and is exactly 0 under the same-image shortcut.  0.03 (3 cm / 1.7
degrees left) is first met behind update 37; 0.04 hands over at the same update, 0.06 at update 19 (3.33 cm / 3.99 degrees, and the
loop still ends at 0.0003 cm), 0.02 only at update 107, when the shortcut's zero arrives, which leaves the law 12 updates.

Measured (MI355X, profiles/photometric.txt): hand-over behind update 37 at 2.5528 cm / 3.1341 degrees; after 120 updates 1.5348 cm /
2.2335 degrees without it, 0.00080 cm / 0.00073 degrees with it (x 0.0005 / x 0.0003)."""
import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib
import closed_loop as cl

pytestmark = pytest.mark.gpu

UPDATES = 120
THRESHOLD = 0.03
HANDED = 37              # the update behind which the hand-over comes (measured; the run is deterministic: seed 121)
PHOTOMETRIC = dict(photometric_lambda=0.5, photometric_level=2, photometric_mu=0.01, photometric_interaction="desired")


def run_loop(threshold, updates=UPDATES, **more):
    """(track [updates + 1, 2] cm / degrees, left [updates] = max |raw v_c| / lambda_ of every update, the update of the hand-over
    or None, the photometric statuses seen)."""
    servo_params = dict(subpatch=True)
    if threshold > 0:
        servo_params.update(photometric_handover=threshold, **{**PHOTOMETRIC, **more})
    eng, params, ctl, sim = cl.set_up(servo_params, "fp32", give_goal_depth=True)
    torch.manual_seed(121)
    track, left, handed, statuses = [cl.sim_pose_error(sim)], [], None, []
    for it in range(updates):
        sim.sense()
        was = ctl.photometric_active
        ctl.ibvs()
        if ctl.photometric_active and not was and handed is None:
            handed = it                                          # this update's twist made the criterion: the next one is photometric
        if was:
            statuses.append(ctl.last_photometric["status"])
        gain = params.lambda_ if not (was and ctl.photometric_active) else PHOTOMETRIC["photometric_lambda"]
        left.append(float(np.max(np.abs(ctl._raw_v))) / gain)
        lin, ang = ctl.publish_twist()
        sim.apply_twist(lin, ang)
        track.append(cl.sim_pose_error(sim))
    eng.close()
    return np.array(track), np.array(left), handed, statuses


def test_the_hand_over_ends_ten_times_closer_than_the_vit_law_alone():
    plain, left_plain, handed_plain, _ = run_loop(0.0)
    fine, left_fine, handed, statuses = run_loop(THRESHOLD)
    for name, tr in (("hand-over off", plain), ("hand-over on ", fine)):
        print(f"closed loop fp32, subpatch, {name}: pose error (cm / deg) at updates 0, 10, .., {UPDATES}: "
              + "  ".join(f"{p:.4f}/{r:.4f}" for p, r in tr[::10]))
    print(f"max |raw v_c| / lambda_ of the plain run at updates 0, 10, ..: " + "  ".join(f"{x:.4f}" for x in left_plain[::10]))
    assert handed_plain is None
    assert handed is not None, "the hand-over never happened"
    print(f"hand-over behind update {handed} at {fine[handed + 1, 0]:.4f} cm / {fine[handed + 1, 1]:.4f} deg; final {plain[-1, 0]:.4f} cm / "
          f"{plain[-1, 1]:.4f} deg without it, {fine[-1, 0]:.4f} cm / {fine[-1, 1]:.4f} deg with it "
          f"(x {fine[-1, 0] / plain[-1, 0]:.4f} / x {fine[-1, 1] / plain[-1, 1]:.4f})")
    assert 0 < handed < UPDATES - 20, "a hand-over this late leaves the photometric law no updates to show anything"
    assert handed == HANDED, "the hand-over moved: the figures of the docstring, the README and profiles/photometric.txt are stale"
    assert np.array_equal(plain[:handed + 2], fine[:handed + 2])          # the same run up to the first photometric update
    assert len(statuses) == UPDATES - 1 - handed and all(s == _lib.STATUS_OK for s in statuses)    # no fall-back
    assert fine[:, 0].max() <= 2 * plain[0, 0]                             # never near the divergence abort
    assert fine[-1, 0] < 0.1 * plain[-1, 0] and fine[-1, 1] < 0.1 * plain[-1, 1]
