"""The photometric law away from the GPU: the configuration and the refusals of the Python layer, the new symbols
and ``vitvs_op_photometric_plan`` against a restatement of its arithmetic, and tests/photometric_ref.py itself, the fp64 reference
the device tests compare with: its signs, and a closed loop on tests/planar_sim.py on the CPU.

The closed loop is the set-up of tests/closed_loop.py (640 x 480, f = 502.3 px, the plane 0.61 m away, synth.texture(128, 11) over
1.6 m, dt 0.5) from 1.5 cm / 2.2 degrees, where the loop with ``subpatch`` stalls: level 2, the desired interaction matrix with the
goal's depth image, mu 0.01, lambda 0.5, 60 updates.  The prototype ended at 0.0044 cm / 0.0038 degrees; the bar, 0.05 cm / 0.05
degrees, is ten times that: the test asserts the reference's behaviour, not a tolerance of the device."""
import ctypes as C
import os
import types

import numpy as np
import pytest

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib, config, synth
import photometric_ref as pr
from planar_sim import PlanarScene, quat_xyzw, rodrigues

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- (a) configuration and refusals
def test_servo_params_validation():
    p = config.ServoParams()
    assert p.photometric_handover == 0.0 and p.photometric_level == 2 and p.photometric_mu == 0.01
    assert p.photometric_lambda is None and p.photometric_interaction == "desired"
    q = config.ServoParams(photometric_handover=0.02, photometric_level=3, photometric_mu=0.0, photometric_lambda=0.5,
                           photometric_interaction="current")
    assert (q.photometric_handover, q.photometric_level, q.photometric_mu, q.photometric_lambda) == (0.02, 3, 0.0, 0.5)
    for bad in (-0.01, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="photometric_handover"):
            config.ServoParams(photometric_handover=bad)
    for bad in (-1, 4, 1.5):
        with pytest.raises(ValueError, match="photometric_level"):
            config.ServoParams(photometric_level=bad)
    for bad in (-1e-3, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="photometric_mu"):
            config.ServoParams(photometric_mu=bad)
    for bad in (float("inf"), float("nan")):
        with pytest.raises(ValueError, match="photometric_lambda"):
            config.ServoParams(photometric_lambda=bad)
    for bad in ("mean", "", 1):
        with pytest.raises(ValueError, match="photometric_interaction"):
            config.ServoParams(photometric_interaction=bad)
    with pytest.raises(ValueError, match="roll_search"):
        config.ServoParams(photometric_handover=0.02, roll_search=True)
    assert config.ServoParams(roll_search=True).photometric_handover == 0.0      # off: nothing to refuse


def test_yaml_keys():
    cfg = {k: 1 for k in config._REQUIRED_KEYS}
    cfg["image_path"] = "goal.png"
    got = config.load_reference_config(cfg).servo
    assert got.photometric_handover == 0.0 and got.photometric_level == 2 and got.photometric_mu == 0.01
    assert got.photometric_lambda is None and got.photometric_interaction == "desired"
    cfg.update(photometric_handover=0.03, photometric_level=1, photometric_mu=0.1, photometric_lambda=0.25,
               photometric_interaction="current")
    ref = config.load_reference_config(cfg)
    got = ref.servo
    assert (got.photometric_handover, got.photometric_level, got.photometric_mu, got.photometric_lambda,
            got.photometric_interaction) == (0.03, 1, 0.1, 0.25, "current")
    assert not {k for k in ref.extras if k.startswith("photometric")}
    for bad in (7, 1.5):                                                         # (1.5 is not truncated to 1 on the way in)
        cfg.update(photometric_level=bad)
        with pytest.raises(ValueError, match="photometric_level"):
            config.load_reference_config(cfg)


def _fake_engine(params):
    return types.SimpleNamespace(params=params, cfg=types.SimpleNamespace(img_size=224), apply_law_params=lambda p: None,
                                 max_pairs=4, set_goal_depth=lambda z: None)


def test_the_controllers_and_the_hand_over():
    from vitvs_amd import pipeline, servo
    on = config.ServoParams(photometric_handover=0.02)
    eng = _fake_engine(on)
    ctl = servo.Controller(eng, goal_image=None, params=on)
    assert ctl.photometric_active is False and ctl.last_photometric is None
    with pytest.raises(ValueError, match="photometric_handover"):
        servo.MultiController(eng, [None, None], params=on)
    with pytest.raises(ValueError, match="photometric_handover"):
        pipeline.UpdatePipeline(config.baseline_config("vits16_224"), on, {})
    rolled = config.ServoParams(roll_search=True)
    object.__setattr__(rolled, "photometric_handover", 0.02)                     # (past ServoParams' own refusal)
    with pytest.raises(ValueError, match="roll_search"):
        servo.Controller(_fake_engine(rolled), goal_image=None, params=rolled)


def test_the_hand_over_criterion():
    """max |raw v_c| / lambda_ against the threshold, behind an update with status OK only; the same-image shortcut's exact zero is
    below any threshold; a goal image that is not at the camera's resolution is refused at construction."""
    from vitvs_amd import servo
    p = config.ServoParams(photometric_handover=0.02, lambda_=0.03, u_max=32, v_max=24)
    eng = _fake_engine(p)
    eng.device = "cpu"
    goal = np.zeros((24, 32, 3), np.uint8)

    def after(raw, status, goal_image=goal):
        ctl = servo.Controller(eng, goal_image=goal_image, params=p)
        ctl.image_callback_rgb(np.zeros((24, 32, 3), np.uint8))
        ctl._raw_v, ctl.last_status = np.asarray(raw, np.float64), status
        ctl._watch_handover()
        return ctl.photometric_active

    assert after([0, 0, 0, 0, 0, 0.03 * 0.0199], _lib.STATUS_OK)
    assert not after([0, 0, 0, 0, 0, 0.03 * 0.0201], _lib.STATUS_OK)
    assert not after([0, -0.03 * 0.0201, 0, 0, 0, 0], _lib.STATUS_OK)
    assert after(np.zeros(6), _lib.STATUS_OK)
    assert not after(np.zeros(6), _lib.STATUS_TOO_FEW)
    with pytest.raises(ValueError, match="v_max x u_max"):                       # a goal the law could never be handed
        after(np.zeros(6), _lib.STATUS_OK, goal_image=np.zeros((48, 64, 3), np.uint8))
    late = servo.Controller(eng, goal_image=goal, params=p)                      # a goal replaced later by one of another size, or a
    late.goal_image = np.zeros((48, 64, 3), np.uint8)                            # frame of another size: no hand-over
    late.image_callback_rgb(np.zeros((24, 32, 3), np.uint8))
    late._raw_v, late.last_status = np.zeros(6), _lib.STATUS_OK
    late._watch_handover()
    assert late.photometric_active is False
    off = servo.Controller(_fake_engine(config.ServoParams()), goal_image=goal)
    off._raw_v, off.last_status = np.zeros(6), _lib.STATUS_OK
    off._watch_handover()
    assert off.photometric_active is False


def test_engine_photometric_velocity_checks_its_arguments_before_the_device():
    from vitvs_amd.engine import Engine, VitvsError
    eng = Engine.__new__(Engine)                               # no handle, no device: the checks come first
    f = np.zeros((24, 32, 3), np.uint8)
    K = (30.0, 30.0, 16.0, 12.0)
    with pytest.raises(VitvsError, match="uint8"):
        eng.photometric_velocity_host(f.astype(np.float32), f, None, K, depth_scale=1.0)
    with pytest.raises(VitvsError, match="one shape"):
        eng.photometric_velocity_host(f, f[:, :30], None, K, depth_scale=1.0)
    with pytest.raises(VitvsError, match="uint16"):
        eng.photometric_velocity_host(f, f, np.zeros((24, 32), np.int32), K)
    with pytest.raises(VitvsError, match="uint16"):
        eng.photometric_velocity_host(f, f, np.zeros((24, 30), np.uint16), K)
    with pytest.raises(VitvsError, match="per pair"):
        eng.photometric_velocity_host(f, f, None, np.zeros((2, 4)), depth_scale=1.0)


# ---------------------------------------------------------------------------------------------- (b) symbols and the plan
NEW_SYMBOLS = ("vitvs_photometric_velocity_dev", "vitvs_photometric_velocity", "vitvs_op_photometric_plan")


def test_the_new_symbols_are_declared_bound_and_exported():
    headers = "".join(open(os.path.join(ROOT, "include", n)).read() for n in ("vitvs.h", "vitvs_ops.h"))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert f"VITVS_API int {name}(" in headers, name
        assert name in _lib.PROTOTYPES and getattr(lib, name) is not None, name
    assert len(_lib.PROTOTYPES["vitvs_photometric_velocity_dev"][1]) == 18
    assert len(_lib.PROTOTYPES["vitvs_photometric_velocity"][1]) == 17
    assert _lib.ABI_VERSION == 2 and lib.vitvs_abi_version() == 2


def _plan(height, width, level):
    """The launch plan restated: pooled size, pooled rows per band (at most 2048 >> level pooled pixels, and one row until the image
    has more than 256 of them: a band per CU first; at least one row), bands, LDS = four waves' 32 doubles + the two luminance
    bands with their halo rows + the depth band, int32 each, the opt-in past 64 KiB, 256 bytes of partial per band."""
    h, w = height >> level, width >> level
    rows = max(1, min((2048 >> level) // w, h // 256))
    bands = -(-h // rows)
    lds = 4 * 32 * 8 + 4 * ((rows + 2) * 2 * w + rows * w)
    return (h, w, rows, bands, lds, 256 * bands, int(lds > 64 * 1024), 0)


def _call(height, width, level):
    out = (C.c_int32 * 8)(*([-1] * 8))
    return _lib.load().vitvs_op_photometric_plan(height, width, level, out), tuple(out)


# (513, 32, 0) and (1538, 64, 1): pooled rows = a whole number of bands + 1 (513 = 256 x 2 + 1; 769 = 256 x 3 + 1)
PLAN_SHAPES = [(24, 32, 0), (29, 37, 1), (48, 64, 2), (88, 96, 3), (224, 224, 0), (480, 640, 0), (480, 640, 3), (513, 32, 0),
               (1538, 64, 1), (4096, 4096, 0), (4096, 4096, 3), (4096, 64, 0), (3, 3, 0), (24, 24, 3)]


@pytest.mark.parametrize("shape", PLAN_SHAPES)
def test_plan_equals_its_formula(shape):
    rc, out = _call(*shape)
    assert rc == 0 and out == _plan(*shape), (shape, rc, out)
    assert out[:6] == pr.plan(*shape), "tests/photometric_ref.py restates the same plan"
    h, w, rows, bands = out[:4]
    assert (bands - 1) * rows < h <= bands * rows and out[4] <= 160 * 1024


def test_plan_one_row_past_a_whole_number_of_bands():
    for shape in ((513, 32, 0), (1538, 64, 1)):
        h, w, rows, bands = _call(*shape)[1][:4]
        assert bands > 1 and rows > 1 and h == (bands - 1) * rows + 1, (shape, h, rows, bands)


def test_plan_refusals():
    lib = _lib.load()
    assert lib.vitvs_op_photometric_plan(24, 32, 0, None) == -1
    for bad in ((24, 32, -1), (24, 32, 4), (0, 32, 0), (24, 0, 0), (-24, 32, 0), (4097, 32, 0), (24, 4097, 0), (2, 32, 0), (24, 2, 0),
                (23, 32, 3), (24, 23, 3), (5, 64, 1)):
        rc, out = _call(*bad)
        assert rc == -2, bad


# ---------------------------------------------------------------------------------------------- (c), (d) the reference itself
PARAMS = config.ServoParams(dino_input_size=224, use_feature_binning=False)
PLANE_Z, SPAN, DT = 0.61, 1.6, 0.5


@pytest.fixture(scope="module")
def scene():
    sc = PlanarScene(synth.texture(128, 11), SPAN / 128, PARAMS, plane_z=PLANE_Z, device="cpu")
    goal_rgb, goal_depth = sc.render(np.eye(3), np.zeros(3))
    return sc, goal_rgb, goal_depth


def _pose_error(R, t):
    q = quat_xyzw(R)
    return float(np.linalg.norm(t) * 100), float(np.rad2deg(2 * np.arccos(min(1.0, abs(q[3])))))


def test_reference_closed_loop_ends_past_the_dead_zone(scene):
    sc, goal_rgb, goal_depth = scene
    axis = np.array([0.3, -0.4, 0.85])
    direction = np.array([0.6, -0.5, 0.6])
    R = rodrigues(axis / np.linalg.norm(axis) * np.deg2rad(2.2))
    t = direction / np.linalg.norm(direction) * 0.015
    p0, r0 = _pose_error(R, t)
    assert abs(p0 - 1.5) < 1e-9 and abs(r0 - 2.2) < 1e-6
    track = [(p0, r0)]
    for _ in range(60):
        rgb, _ = sc.render(R, t)
        out = pr.velocity(rgb, goal_rgb, goal_depth, 0.0, PARAMS.intrinsics(), 2, 1, 0.01, 0.5)
        assert out["status"] == pr.OK
        v, w = out["v"][:3], out["v"][3:]
        t = t + R @ v * DT                                     # planar_sim's integration of a camera-frame twist
        R = R @ rodrigues(w * DT)
        track.append(_pose_error(R, t))
    print("photometric reference, closed loop from 1.5 cm / 2.2 deg, level 2: pose error (cm / deg) at updates 0, 10, .., 60: "
          + "  ".join(f"{p:.4f}/{r:.4f}" for p, r in track[::10]))
    assert track[-1][0] < 0.05 and track[-1][1] < 0.05
    assert max(p for p, _ in track) <= 2 * p0


@pytest.mark.parametrize("axis", range(6))
def test_reference_signs(scene, axis):
    """A camera a little way along (or turned a little about) one axis of the goal frame is sent back along that axis."""
    sc, goal_rgb, goal_depth = scene
    R, t = np.eye(3), np.zeros(3)
    if axis < 3:
        t[axis] = 0.004
    else:
        w = np.zeros(3)
        w[axis - 3] = np.deg2rad(0.4)
        R = rodrigues(w)
    rgb, depth = sc.render(R, t)
    for interaction, z in ((1, goal_depth), (0, depth)):
        out = pr.velocity(rgb, goal_rgb, z, 0.0, PARAMS.intrinsics(), 2, interaction, 0.01, 0.5)
        assert out["status"] == pr.OK and out["v"][axis] < 0.0, (axis, interaction, out["v"])
        assert abs(out["v"][axis]) == np.abs(out["v"][:3] if axis < 3 else out["v"][3:]).max(), (axis, interaction, out["v"])


def test_reference_statuses(scene):
    _, goal_rgb, goal_depth = scene
    K = PARAMS.intrinsics()
    same = pr.velocity(goal_rgb, goal_rgb, goal_depth, 0.0, K, 2, 1, 0.01, 0.5)
    assert same["status"] == pr.OK and np.array_equal(same["v"], np.zeros(6)) and same["info"][0] == 118 * 158
    flat = np.full_like(goal_rgb, 90)
    out = pr.velocity(flat, flat, goal_depth, 0.0, K, 2, 1, 0.01, 0.5)
    assert out["status"] == pr.TOO_FEW and out["info"][5] == 1 and np.array_equal(out["v"], np.zeros(6))
    out = pr.velocity(goal_rgb, goal_rgb, np.zeros_like(goal_depth), 0.0, K, 2, 1, 0.01, 0.5)
    assert out["status"] == pr.TOO_FEW and list(out["info"][[0, 4, 5]]) == [0, 118 * 158, 0]
    out = pr.velocity(goal_rgb, goal_rgb, None, 0.0, K, 2, 1, 0.01, 0.5)
    assert out["status"] == pr.NO_DEPTH and np.array_equal(out["v"], np.zeros(6))
    assert pr.velocity(goal_rgb, goal_rgb, None, 0.61, K, 2, 1, 0.01, 0.5)["status"] == pr.OK
