"""The robust photometric law away from the GPU: the configuration, the YAML keys, the refusals and argument checks of
the Python layer, the new symbols, and tests/photometric_robust_ref.py itself, the fp64 reference the device tests compare with.

The closed loops are test_photometric_host.py's (640 x 480, level 2, the desired interaction matrix with the goal's depth image, mu
0.01, lambda 0.5, dt 0.5, from 1.5 cm / 2.2 degrees, 60 updates) with the current frame disturbed before the law sees it:
  "gain+bias"  clip(round(1.15 rgb + 8)): an exposure change that saturates 5.7 % of the goal's pixels;
  "block"      pixels [120:240, 160:320] replaced by a random 6 x 8 checker of 20-pixel squares: 6.25 % of the frame.
The prototype's end points (cm / degrees): the plain law diverges under "gain+bias" (51 cm at update 42); the robust law
(illumination, 4 re-weightings) ends at 0.030 / 0.020 under "gain+bias", 0.0054 / 0.0046 under "block", 0.048 / 0.031 under both and
0.0061 / 0.0053 undisturbed.  The bars are ten times those (the convention of test_photometric_host.py) and its 0.05 / 0.05
undisturbed: the tests assert the reference's behaviour, not a tolerance of the device."""
import os
import types

import numpy as np
import pytest

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib, config, synth
import photometric_ref as pr
import photometric_robust_ref as rr
from planar_sim import PlanarScene, quat_xyzw, rodrigues

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- (a) configuration and refusals
def test_servo_params_validation():
    p = config.ServoParams()
    assert p.photometric_illumination is False and p.photometric_robust_iterations == 0 and p.photometric_sigma_min == 1.0
    q = config.ServoParams(photometric_illumination=True, photometric_robust_iterations=4, photometric_sigma_min=0.25)
    assert (q.photometric_illumination, q.photometric_robust_iterations, q.photometric_sigma_min) == (True, 4, 0.25)
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="photometric_illumination"):
            config.ServoParams(photometric_illumination=bad)
    for bad in (-1, 5, 1.5, True, "2"):
        with pytest.raises(ValueError, match="photometric_robust_iterations"):
            config.ServoParams(photometric_robust_iterations=bad)
    for bad in (0.0, -1.0, float("inf"), float("nan"), "1", True):
        with pytest.raises(ValueError, match="photometric_sigma_min"):
            config.ServoParams(photometric_sigma_min=bad)
    with pytest.raises(ValueError, match="roll_search"):                         # the hand-over's own refusals are unchanged
        config.ServoParams(photometric_handover=0.02, roll_search=True, photometric_illumination=True)


def test_yaml_keys():
    cfg = {k: 1 for k in config._REQUIRED_KEYS}
    cfg["image_path"] = "goal.png"
    got = config.load_reference_config(cfg).servo
    assert got == config.ServoParams(**{f.name: getattr(got, f.name) for f in config.dataclasses.fields(got)
                                        if not f.name.startswith("photometric_")})      # everything off: nothing changes
    assert (got.photometric_illumination, got.photometric_robust_iterations, got.photometric_sigma_min) == (False, 0, 1.0)
    cfg.update(photometric_illumination=True, photometric_robust_iterations=3, photometric_sigma_min=0.5)
    ref = config.load_reference_config(cfg)
    got = ref.servo
    assert (got.photometric_illumination, got.photometric_robust_iterations, got.photometric_sigma_min) == (True, 3, 0.5)
    assert not {k for k in ref.extras if k.startswith("photometric")}
    for key, bad in (("photometric_robust_iterations", 7), ("photometric_robust_iterations", 1.5), ("photometric_sigma_min", 0),
                     ("photometric_illumination", 2)):
        with pytest.raises(ValueError, match=key):
            config.load_reference_config(dict(cfg, **{key: bad}))


def _fake_engine(params, calls):
    def plain(*a):
        calls.append(("plain", a))
        return _FakeTwist(), dict(status=np.array([0]), cost=np.array([2.0]), n=np.array([7]))

    def robust(*a):
        calls.append(("robust", a))
        return _FakeTwist(), dict(status=np.array([0]), cost=np.array([2.0]), n=np.array([7]), gain=np.array([1.15]), bias=np.array([8.0]),
                                  sigma=np.array([1.5]), rejected=np.array([0.0625]))
    return types.SimpleNamespace(params=params, cfg=types.SimpleNamespace(img_size=224), apply_law_params=lambda p: None, max_pairs=4,
                                 set_goal_depth=lambda z: None, device="cpu", photometric_velocity=plain,
                                 photometric_robust_velocity=robust)


class _FakeTwist:
    def __getitem__(self, i):
        return self

    def cpu(self):
        return self

    def numpy(self):
        return np.zeros(6)


@pytest.mark.parametrize("extra,which", [({}, "plain"), (dict(photometric_illumination=True), "robust"),
                                         (dict(photometric_robust_iterations=2), "robust"),
                                         (dict(photometric_illumination=True, photometric_robust_iterations=4,
                                               photometric_sigma_min=0.5), "robust")])
def test_the_controller_calls_the_robust_law_when_either_option_is_on(extra, which):
    from vitvs_amd import servo
    p = config.ServoParams(photometric_handover=0.02, lambda_=0.03, u_max=32, v_max=24, homography_depth=0.6, **extra)
    calls = []
    ctl = servo.Controller(_fake_engine(p, calls), goal_image=np.zeros((24, 32, 3), np.uint8), params=p)
    ctl.image_callback_rgb(np.zeros((24, 32, 3), np.uint8))
    ctl.photometric_active = True
    assert ctl._photometric_step() is True
    assert [c[0] for c in calls] == [which]
    args = calls[0][1]
    assert args[4:8] == (2, "desired", 0.01, 0.03)
    if which == "robust":
        assert args[9:] == (p.photometric_illumination, p.photometric_robust_iterations, p.photometric_sigma_min)
        assert ctl.last_photometric == dict(status=0, cost=2.0, n=7, gain=1.15, bias=8.0, sigma=1.5, rejected=0.0625)
    else:
        assert len(args) == 9 and ctl.last_photometric == dict(status=0, cost=2.0, n=7)


def test_the_hand_overs_refusals_are_unchanged():
    from vitvs_amd import pipeline, servo
    on = config.ServoParams(photometric_handover=0.02, photometric_illumination=True, photometric_robust_iterations=4)
    eng = _fake_engine(on, [])
    with pytest.raises(ValueError, match="photometric_handover"):
        servo.MultiController(eng, [None, None], params=on)
    with pytest.raises(ValueError, match="photometric_handover"):
        pipeline.UpdatePipeline(config.baseline_config("vits16_224"), on, {})
    rolled = config.ServoParams(roll_search=True, photometric_illumination=True)
    object.__setattr__(rolled, "photometric_handover", 0.02)
    with pytest.raises(ValueError, match="roll_search"):
        servo.Controller(_fake_engine(rolled, []), goal_image=None, params=rolled)


def test_engine_checks_its_arguments_before_the_device():
    from vitvs_amd.engine import Engine, VitvsError
    eng = Engine.__new__(Engine)                               # no handle, no device: the checks come first
    f = np.zeros((24, 32, 3), np.uint8)
    K = (30.0, 30.0, 16.0, 12.0)
    with pytest.raises(VitvsError, match="uint8"):
        eng.photometric_robust_velocity_host(f.astype(np.float32), f, None, K, depth_scale=1.0)
    with pytest.raises(VitvsError, match="one shape"):
        eng.photometric_robust_velocity_host(f, f[:, :30], None, K, depth_scale=1.0)
    with pytest.raises(VitvsError, match="uint16"):
        eng.photometric_robust_velocity_host(f, f, np.zeros((24, 32), np.int32), K)
    with pytest.raises(VitvsError, match="per pair"):
        eng.photometric_robust_velocity_host(f, f, None, np.zeros((2, 4)), depth_scale=1.0)
    for bad in (2, -1, "on", None):
        with pytest.raises(VitvsError, match="illumination"):
            eng.photometric_robust_velocity_host(f, f, None, K, depth_scale=1.0, illumination=bad)
    for bad in (-1, 5, 2.5, True):
        with pytest.raises(VitvsError, match="robust_iterations"):
            eng.photometric_robust_velocity_host(f, f, None, K, depth_scale=1.0, robust_iterations=bad)
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(VitvsError, match="sigma_min"):
            eng.photometric_robust_velocity_host(f, f, None, K, depth_scale=1.0, sigma_min=bad)
    with pytest.raises(VitvsError, match="interaction"):
        eng.photometric_robust_velocity_host(f, f, None, K, interaction="mean", depth_scale=1.0)


# ---------------------------------------------------------------------------------------------- (b) symbols
def test_the_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "vitvs.h")).read()
    lib = _lib.load()
    for name, count in (("vitvs_photometric_robust_velocity_dev", 22), ("vitvs_photometric_robust_velocity", 21)):
        assert f"VITVS_API int {name}(" in header, name
        assert name in _lib.PROTOTYPES and getattr(lib, name) is not None, name
        assert len(_lib.PROTOTYPES[name][1]) == count
        declared = header.split(f"VITVS_API int {name}(")[1].split(");")[0]
        assert declared.count(",") + 1 == count, name
    assert len(_lib.PROTOTYPES["vitvs_photometric_velocity_dev"][1]) == 18        # the plain law's prototypes stand
    assert len(_lib.PROTOTYPES["vitvs_photometric_velocity"][1]) == 17
    assert _lib.ABI_VERSION == 2 and lib.vitvs_abi_version() == 2
    from vitvs_amd.engine import Engine
    assert callable(Engine.photometric_robust_velocity) and callable(Engine.photometric_robust_velocity_host)


# ---------------------------------------------------------------------------------------------- (c) the reference itself
PARAMS = config.ServoParams(dino_input_size=224, use_feature_binning=False)
PLANE_Z, SPAN, DT = 0.61, 1.6, 0.5
LEVEL, INTER, MU, LAM, UPDATES = 2, 1, 0.01, 0.5, 60


def gain_bias(rgb, gain=1.15, bias=8.0):
    return np.clip(np.round(gain * rgb.astype(np.float64) + bias), 0, 255).astype(np.uint8)


def block(rgb):
    out = rgb.copy()
    out[120:240, 160:320] = np.kron(np.random.default_rng(5).integers(0, 256, (6, 8, 3)), np.ones((20, 20, 1))).astype(np.uint8)
    return out


DISTURBANCES = {"none": lambda rgb: rgb, "gain+bias": gain_bias, "block": block, "gain+bias and block": lambda rgb: block(gain_bias(rgb))}


@pytest.fixture(scope="module")
def scene():
    sc = PlanarScene(synth.texture(128, 11), SPAN / 128, PARAMS, plane_z=PLANE_Z, device="cpu")
    goal_rgb, goal_depth = sc.render(np.eye(3), np.zeros(3))
    return sc, goal_rgb, goal_depth


def _pose_error(R, t):
    q = quat_xyzw(R)
    return float(np.linalg.norm(t) * 100), float(np.rad2deg(2 * np.arccos(min(1.0, abs(q[3])))))


def _start():
    axis = np.array([0.3, -0.4, 0.85])
    direction = np.array([0.6, -0.5, 0.6])
    return rodrigues(axis / np.linalg.norm(axis) * np.deg2rad(2.2)), direction / np.linalg.norm(direction) * 0.015


def _loop(scene, disturb, law, stop_at=None):
    """(track of (cm, deg), the last law output)."""
    sc, goal_rgb, goal_depth = scene
    R, t = _start()
    track, out = [_pose_error(R, t)], None
    for _ in range(UPDATES):
        rgb, _ = sc.render(R, t)
        out = law(DISTURBANCES[disturb](rgb), goal_rgb, goal_depth)
        assert out["status"] == pr.OK
        v, w = out["v"][:3], out["v"][3:]
        t = t + R @ v * DT
        R = R @ rodrigues(w * DT)
        track.append(_pose_error(R, t))
        if stop_at is not None and track[-1][0] > stop_at:
            break
    print(f"closed loop, {disturb}: pose error (cm / deg) at updates 0, 10, ..: " + "  ".join(f"{p:.4f}/{r:.4f}" for p, r in track[::10])
          + f"; the last {track[-1][0]:.4f}/{track[-1][1]:.4f}")
    return track, out


def _plain(cur, goal, depth):
    return pr.velocity(cur, goal, depth, 0.0, PARAMS.intrinsics(), LEVEL, INTER, MU, LAM)


def _robust(cur, goal, depth):
    return rr.velocity(cur, goal, depth, 0.0, PARAMS.intrinsics(), LEVEL, INTER, MU, LAM, 1, 4, 1.0)


def test_both_options_off_is_the_plain_reference_bit_for_bit(scene):
    sc, goal_rgb, goal_depth = scene
    R, t = _start()
    rgb, depth = sc.render(R, t)
    for cur, z, scalar, inter in ((rgb, goal_depth, 0.0, 1), (block(gain_bias(rgb)), depth, 0.0, 0), (rgb, None, 0.61, 1)):
        for reverse in (False, True):
            want = pr.velocity(cur, goal_rgb, z, scalar, PARAMS.intrinsics(), LEVEL, inter, MU, LAM, reverse=reverse)
            got = rr.velocity(cur, goal_rgb, z, scalar, PARAMS.intrinsics(), LEVEL, inter, MU, LAM, 0, 0, 1.0, reverse=reverse)
            assert got["status"] == want["status"] == pr.OK
            assert np.array_equal(got["v"].view(np.uint64), want["v"].view(np.uint64))
            assert np.array_equal(got["normal"][:28].view(np.uint64), want["normal"].view(np.uint64))
            assert np.array_equal(got["info"][:6], want["info"][:6]) and list(got["info"][6:]) == [0, 0]
            assert np.array_equal(got["robust"], [0.0, 0.0, 0.0, float(want["info"][0])])


def test_the_plain_law_diverges_under_an_exposure_change(scene):
    """The need: under "gain+bias" the plain law leaves twice its start error, with status OK."""
    track, _ = _loop(scene, "gain+bias", _plain, stop_at=3.0)
    assert track[-1][0] > 2 * track[0][0]


@pytest.mark.parametrize("disturb,bar", [("gain+bias", (0.30, 0.20)), ("block", (0.054, 0.046)), ("gain+bias and block", (0.48, 0.31)),
                                         ("none", (0.05, 0.05))])
def test_the_robust_reference_loop_ends_at_the_goal(scene, disturb, bar):
    track, out = _loop(scene, disturb, _robust)
    assert track[-1][0] < bar[0] and track[-1][1] < bar[1]
    assert max(p for p, _ in track) <= 2 * track[0][0]
    gamma, beta = out["robust"][:2]
    print(f"{disturb}: gamma {gamma:.4f}, beta {beta:.3f}, sigma {out['robust'][2]:.3f}, rows of weight 0: {out['info'][6]} of {out['info'][0]}")
    if disturb == "gain+bias":
        assert abs(gamma - 0.15) < 0.02 and abs(beta - 8.0) < 2.0     # the prototype: 0.147 / 8.31; the distance is the clipping


def test_reference_statuses(scene):
    _, goal_rgb, goal_depth = scene
    K = PARAMS.intrinsics()
    same = rr.velocity(goal_rgb, goal_rgb, goal_depth, 0.0, K, 2, 1, MU, LAM, 1, 4, 1.0)
    assert same["status"] == pr.OK and np.array_equal(same["v"], np.zeros(6)) and same["info"][0] == 118 * 158
    assert np.array_equal(same["robust"][:2], np.zeros(2)) and same["robust"][2] == 1.0 and same["robust"][3] == 118 * 158
    assert list(same["info"][6:]) == [0, 4]
    flat = np.full_like(goal_rgb, 90)
    out = rr.velocity(flat, flat, goal_depth, 0.0, K, 2, 1, MU, LAM, 1, 4, 1.0)      # D is constant: the 2 x 2 pivot fails
    assert out["status"] == pr.TOO_FEW and list(out["info"][5:]) == [1, 0, 0] and np.array_equal(out["v"], np.zeros(6))
    l, d0, d1, good = rr._c_factor(out["normal"][40:43])
    assert not good and d0 > 0 and not d1 > 1e-4 * out["normal"][42]
    out = rr.velocity(goal_rgb, goal_rgb, None, 0.0, K, 2, 1, MU, LAM, 1, 4, 1.0)
    assert out["status"] == pr.NO_DEPTH and np.array_equal(out["v"], np.zeros(6))
    out = rr.velocity(goal_rgb, goal_rgb, np.zeros_like(goal_depth), 0.0, K, 2, 1, MU, LAM, 1, 4, 1.0)
    assert out["status"] == pr.TOO_FEW and list(out["info"][[0, 4, 5]]) == [0, 118 * 158, 0]


def test_fewer_than_six_rows_with_a_weight_is_too_few():
    cur, des, K = rr.few_weights_pair()
    out = rr.velocity(cur, des, None, 0.6, K, 0, 1, MU, LAM, 0, 4, 1e-3)
    assert out["info"][0] == 10 and out["status"] == pr.TOO_FEW and out["info"][5] == 0
    assert out["info"][7] == 1 and out["margin_t"] > 0.2 and out["info"][0] - out["info"][6] < 6 and np.array_equal(out["v"], np.zeros(6))
