"""The three interaction matrices of the control law (option ``interaction``) on the CPU: the fp64 reference
(tests/interaction_ref.py) alone, and the host-side parameter plumbing."""
import numpy as np
import pytest

import vitvs_amd  # noqa: F401
from vitvs_amd import config
import interaction_ref as ir
import robust_ref as rr


def test_equal_features_and_depths_give_equal_laws():
    """s = s* and Z = Z*: the three matrices are one matrix, element for element."""
    rng = np.random.default_rng(1)
    params = config.ServoParams(dino_input_size=224)
    ids = rng.choice(196, size=24, replace=False)
    s = rr.token_pixels(ids, 14, 224, params.u_max, params.v_max)
    depth = rng.integers(1, 3000, size=(params.v_max, params.u_max)).astype(np.uint16)
    depth[s[0, 1], s[0, 0]] = 0                                        # a hole under the first feature: the 100 m sentinel
    laws = {m: ir.law(s, s, depth, depth, params.intrinsics(), params.lambda_, m) for m in ir.MODES}
    assert np.array_equal(laws["current"]["L"], laws["desired"]["L"]) and np.array_equal(laws["current"]["L"], laws["mean"]["L"])
    assert np.array_equal(laws["mean"]["Z"], laws["mean"]["Z_goal"]) and np.any(laws["mean"]["Z"] == 100.0)
    for m in ir.MODES:
        assert not laws[m]["e"].any() and not laws[m]["v_c"].any()
    # and with an error that is not zero (the same matrix on another e): shift the goal side, keep L's inputs by construction
    e = rng.normal(size=(48, 1)) * 1e-2
    v = [(-params.lambda_ * np.linalg.pinv(laws[m]["L"]) @ e).flatten() for m in ir.MODES]
    assert np.array_equal(v[0], v[1]) and np.array_equal(v[0], v[2])


def test_current_mode_is_the_oracle_law():
    from oracle import servo_ref as sr
    params = config.ServoParams(dino_input_size=224)
    sc = rr.planted_scenario(np.random.default_rng(2), 24, 0.125, params, holes=True)
    s_star, s_, ref = rr.oracle_law(sc, params)
    mine = ir.law(s_star, s_, sc["depth"], sc["depth"], sc["K"], params.lambda_, "current")
    assert np.array_equal(mine["L"], ref["L"]) and np.array_equal(mine["e"], ref["e"]) and np.array_equal(mine["v_c"], ref["v_c"])
    assert sr.get_depth(sc["depth"], s_).tolist() == mine["Z"].tolist()


def test_quarter_turn_about_the_optical_axis():
    """A quarter turn of the 14 x 14 token grid, 24 pairs, both depths 0.61 m, lambda = 1: the current law retreats along the
    optical axis, the desired law advances, the mean matrix gives (nearly) the pure rotation.  Not at 180 degrees: the mean matrix
    is rank deficient there."""
    case = ir.quarter_turn_case()
    laws = ir.quarter_turn_laws(case)
    v = {m: laws[m]["v_c"] for m in ir.MODES}
    for m in ir.MODES:
        print(f"quarter turn, {m:8s}: v_z = {v[m][2]:+.4f}  w_z = {v[m][5]:+.4f}  |other four| = {np.linalg.norm(v[m][[0, 1, 3, 4]]):.2e}")
        assert np.linalg.matrix_rank(laws[m]["L"]) == 6
    ir.quarter_turn_properties(v["current"][2], v["desired"][2], v["mean"][2])
    assert v["current"][2] < 0 < v["desired"][2]
    # the rotation itself: every law turns the same way, the mean about twice as fast as either (the chord against the arc)
    assert v["current"][5] * v["desired"][5] > 0 and v["mean"][5] * v["current"][5] > 0
    assert abs(v["mean"][5]) > 1.5 * abs(v["current"][5])


def test_params_and_the_reference_config_mapping():
    assert config.ServoParams().interaction == "current"
    for name in ir.MODES:
        assert config.ServoParams(interaction=name).interaction == name
    assert tuple(config.INTERACTIONS) == ir.MODES                      # option values 0 / 1 / 2 in this order
    with pytest.raises(ValueError):
        config.ServoParams(interaction="average")
    with pytest.raises(ValueError):
        config.ServoParams().replace(interaction="Current")
    m = {k: 1 for k in config._REQUIRED_KEYS}
    m["image_path"] = "goal.png"
    rc = config.load_reference_config(m)
    assert rc.servo.interaction == "current"
    m["interaction"] = "mean"
    rc = config.load_reference_config(m)
    assert rc.servo.interaction == "mean" and "interaction" not in rc.extras
