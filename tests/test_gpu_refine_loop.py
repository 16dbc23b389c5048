"""Closed loop on the GPU with the sub-patch refinement of matches (option ``subpatch``).

The set-up of tests/test_gpu_loop.py (tests/closed_loop.py): ``servo.Controller(Engine)`` on ViT-S/16 224² with synthetic weights
driving a simulated camera (tests/planar_sim.py) over the smooth texture (synth.texture at 128 px over 1.6 m, 0.61 m away) from a
5 cm / 5 degree offset, ``selection="order"``, dt = 0.5 s, torch seed 121.  That loop ends in the patch-quantisation dead zone: the
features are patch centres, so once every match is the identity the error is 0 wherever within a patch pitch the camera stands.
Here it runs twice, 360 updates each, fp32 and bf16: with the option off (the yardstick: the plain law, bit for bit) and on.

  * neither run comes near the divergence abort (position error <= 2 x the initial 5 cm throughout);
  * the refined run's final position and orientation errors are below the unrefined run's, by the ratios below.

Measured (final pose error after 360 updates, cm / degrees; profiles/subpatch.txt has the trajectories):
    fp32   subpatch off 3.547 / 2.782   on 1.535 / 2.233   ratio 0.433 / 0.803
    bf16   subpatch off 3.567 / 2.805   on 1.551 / 2.245   ratio 0.435 / 0.800
The asserted ratios are half-way between the measured ratio and 1."""
import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
import closed_loop as cl

pytestmark = pytest.mark.gpu

UPDATES = 360
# (position, orientation): refined final error <= ratio x unrefined final error
RATIO = {"fp32": (0.72, 0.90), "bf16": (0.72, 0.90)}


def _run_loop(precision, subpatch):
    eng, _, ctl, sim = cl.set_up(dict(subpatch=subpatch), precision)
    torch.manual_seed(121)          # the visiting orders come from torch's global RNG: both runs see the same draws (vitvs_v2.py:1397)
    track, statuses, moved, same = [cl.sim_pose_error(sim)], [], 0, []
    for it in range(UPDATES):
        sim.sense()
        ctl.ibvs()
        statuses.append(ctl.last_status)
        same.append(int(eng.last_features(1)["info"][0, 2]))
        if it % 30 == 0 and ctl.last_status == 0:
            moved += int(np.any(eng.last_offsets(1)))
        lin, ang = ctl.publish_twist()
        sim.apply_twist(lin, ang)
        track.append(cl.sim_pose_error(sim))
    eng.close()
    return np.array(track), statuses, moved, np.array(same)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_refined_loop_ends_closer_than_the_unrefined_loop(precision):
    plain, st_plain, moved_plain, same_plain = _run_loop(precision, False)
    fine, st_fine, moved_fine, same_fine = _run_loop(precision, True)
    for name, tr in (("subpatch off", plain), ("subpatch on ", fine)):
        print(f"closed loop {precision}, {name}: pose error (cm / deg) at updates 0, 30, .., {UPDATES}: "
              + "  ".join(f"{p:.2f}/{r:.2f}" for p, r in tr[::30]) + f"; highest position error {tr[:, 0].max():.2f} cm; "
              f"mean of the last 60: {tr[-60:, 0].mean():.3f} cm / {tr[-60:, 1].mean():.3f} deg")
    print(f"closed loop {precision}: final {plain[-1, 0]:.3f} cm / {plain[-1, 1]:.3f} deg -> {fine[-1, 0]:.3f} cm / {fine[-1, 1]:.3f} deg "
          f"(x {fine[-1, 0] / plain[-1, 0]:.3f} / x {fine[-1, 1] / plain[-1, 1]:.3f})")
    for name, same in (("subpatch off", same_plain), ("subpatch on ", same_fine)):
        first = int(np.argmax(same)) if same.any() else -1
        print(f"closed loop {precision}, {name}: {int(same.sum())} of {UPDATES} updates took the same-image shortcut (mean similarity "
              f"> 0.99: v_c = 0), the first at update {first}")
    p0, r0 = plain[0]
    assert abs(p0 - 5.0) < 1e-9 and abs(r0 - 5.0) < 1e-6 and np.array_equal(plain[0], fine[0])
    assert all(s in (0, 2) for s in st_plain + st_fine)
    assert moved_plain == 0 and moved_fine > 0                           # the option, and only the option, moves matches
    assert plain[:, 0].max() <= 2 * p0 and fine[:, 0].max() <= 2 * p0    # never at the divergence abort
    rp, rr_ = RATIO[precision]
    assert fine[-1, 0] < plain[-1, 0] and fine[-1, 1] < plain[-1, 1]
    assert fine[-1, 0] <= rp * plain[-1, 0] and fine[-1, 1] <= rr_ * plain[-1, 1]
