"""The tile photometric law away from the GPU: the configuration, the YAML keys, the refusals, the hand-back rule on
fake engines, the new symbols, the plan against its restatement, and tests/photometric_tile_ref.py itself, the fp64 reference the
device tests compare with.

The closed loops are test_photometric_robust_host.py's (640 x 480, level 2, the desired interaction matrix with the goal's depth
image, mu 0.01, lambda 0.5, dt 0.5, from 1.5 cm / 2.2 degrees; illumination on, N = 4, sigma_min 1) over 40 updates, every current
frame under "shadow" (photometric_tile_cases.shadow: 0.6 behind a slanted edge, about 45 % of the view).  The prototype's end points
(cm / degrees): the robust law is at 6.93 / 4.28 after two updates and gone; 4 x 4 tiles end at 0.0316 / 0.0256, 2 x 2 at 0.1435 /
0.1254, 4 x 4 undisturbed at 0.0180.  The bars are ten times those (the convention of test_photometric_host.py): the tests assert the
reference's behaviour, not a tolerance of the device.  The loop tests' docstrings have what this reference measures."""
import ctypes as C
import os
import types

import numpy as np
import pytest

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib, config, servo, synth
import photometric_ref as pr
import photometric_robust_ref as rr
import photometric_tile_ref as tr
import photometric_tile_cases as tc
from planar_sim import PlanarScene, quat_xyzw, rodrigues

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ON = dict(photometric_illumination=True, photometric_robust_iterations=4)


# ---------------------------------------------------------------------------------------------- (a) configuration and refusals
def test_servo_params_validation():
    p = config.ServoParams()
    assert p.photometric_tiles == (1, 1) and p.photometric_handback_rejected == 0.0
    q = config.ServoParams(photometric_tiles=(4, 8), photometric_handback_rejected=0.25, **ON)
    assert q.photometric_tiles == (4, 8) and q.photometric_handback_rejected == 0.25
    assert config.ServoParams(photometric_tiles=[2, 3], **ON).photometric_tiles == (2, 3)          # a YAML sequence
    assert config.ServoParams(photometric_tiles=(1, 1)).photometric_tiles == (1, 1)                # off needs nothing
    for bad in ((0, 4), (4, 9), (4,), (2, 2, 2), 4, "4x4", (2.0, 2), (True, 2), None):
        with pytest.raises(ValueError, match="photometric_tiles"):
            config.ServoParams(photometric_tiles=bad, **ON)
    with pytest.raises(ValueError, match="photometric_illumination"):
        config.ServoParams(photometric_tiles=(4, 4))
    with pytest.raises(ValueError, match="photometric_illumination"):
        config.ServoParams(photometric_tiles=(1, 2), photometric_robust_iterations=4)
    for bad in (-0.1, 1.5, float("nan"), float("inf"), "0.2", True, None):
        with pytest.raises(ValueError, match="photometric_handback_rejected"):
            config.ServoParams(photometric_handback_rejected=bad, **ON)
    with pytest.raises(ValueError, match="photometric_robust_iterations"):
        config.ServoParams(photometric_handback_rejected=0.3, photometric_illumination=True)
    assert config.ServoParams(photometric_handback_rejected=1.0, photometric_robust_iterations=1).photometric_handback_rejected == 1.0


def test_yaml_keys():
    cfg = {k: 1 for k in config._REQUIRED_KEYS}
    cfg["image_path"] = "goal.png"
    got = config.load_reference_config(cfg).servo
    assert got.photometric_tiles == (1, 1) and got.photometric_handback_rejected == 0.0
    cfg.update(photometric_illumination=True, photometric_robust_iterations=3, photometric_tiles=[4, 2], photometric_handback_rejected=0.4)
    ref = config.load_reference_config(cfg)
    assert ref.servo.photometric_tiles == (4, 2) and ref.servo.photometric_handback_rejected == 0.4
    assert not {k for k in ref.extras if k.startswith("photometric")}
    for key, bad in (("photometric_tiles", [4, 16]), ("photometric_tiles", 4), ("photometric_handback_rejected", 2),
                     ("photometric_illumination", False), ("photometric_robust_iterations", 0)):
        with pytest.raises(ValueError, match=key):
            config.load_reference_config(dict(cfg, **{key: bad}))


class _FakeTwist:
    def __getitem__(self, i):
        return self

    def cpu(self):
        return self

    def numpy(self):
        return np.zeros(6)


def _fake_engine(params, calls, rejected=0.0625, status=0):
    base = dict(status=np.array([status]), cost=np.array([2.0]), n=np.array([7]))

    def plain(*a):
        calls.append(("plain", a))
        return _FakeTwist(), dict(base)

    def robust(*a):
        calls.append(("robust", a))
        return _FakeTwist(), dict(base, gain=np.array([1.15]), bias=np.array([8.0]), sigma=np.array([1.5]), rejected=np.array([rejected]))

    def tile(*a):
        calls.append(("tile", a))
        gy, gx = a[9]
        gain = np.linspace(0.6, 1.0, gy * gx).reshape(1, gy, gx)
        live = np.ones((1, gy, gx), bool)
        live[0, 0, 0] = False                                    # the dead tile's gain of 1 is not in the range
        return _FakeTwist(), dict(base, sigma=np.array([1.5]), rejected=np.array([rejected]), tile_gain=np.where(live, gain, 1.0),
                                  tile_live=live, dead_tiles=np.array([1]))
    return types.SimpleNamespace(params=params, cfg=types.SimpleNamespace(img_size=224), apply_law_params=lambda p: None, max_pairs=4,
                                 set_goal_depth=lambda z: None, device="cpu", photometric_velocity=plain,
                                 photometric_robust_velocity=robust, photometric_tile_velocity=tile)


def _controller(calls, rejected=0.0625, status=0, **extra):
    p = config.ServoParams(photometric_handover=0.02, lambda_=0.03, u_max=32, v_max=24, homography_depth=0.6, **extra)
    ctl = servo.Controller(_fake_engine(p, calls, rejected, status), goal_image=np.zeros((24, 32, 3), np.uint8), params=p)
    ctl.image_callback_rgb(np.zeros((24, 32, 3), np.uint8))
    ctl.photometric_active = True
    return ctl, p


@pytest.mark.parametrize("extra,which", [({}, "plain"), (dict(photometric_illumination=True), "robust"), (dict(ON), "robust"),
                                         (dict(ON, photometric_tiles=(1, 1)), "robust"), (dict(ON, photometric_tiles=(4, 4)), "tile"),
                                         (dict(photometric_illumination=True, photometric_tiles=(1, 2)), "tile"),
                                         (dict(ON, photometric_tiles=(8, 3), photometric_sigma_min=0.5), "tile")])
def test_the_controller_calls_the_tile_law_exactly_when_tiles_are_set(extra, which):
    calls = []
    ctl, p = _controller(calls, **extra)
    assert ctl._photometric_step() is True and ctl.photometric_active
    assert [c[0] for c in calls] == [which]
    args = calls[0][1]
    assert args[4:8] == (2, "desired", 0.01, 0.03)
    if which == "tile":
        assert args[9:] == (p.photometric_tiles, p.photometric_robust_iterations, p.photometric_sigma_min) and len(args) == 12
        T = p.photometric_tiles[0] * p.photometric_tiles[1]
        lo = 0.6 + 0.4 / (T - 1)                                 # the second tile's: the first is dead
        assert ctl.last_photometric == dict(status=0, cost=2.0, n=7, sigma=1.5, rejected=0.0625, dead_tiles=1,
                                            gain_min=pytest.approx(lo), gain_max=1.0)
    elif which == "robust":
        assert args[9:] == (p.photometric_illumination, p.photometric_robust_iterations, p.photometric_sigma_min)
        assert ctl.last_photometric == dict(status=0, cost=2.0, n=7, gain=1.15, bias=8.0, sigma=1.5, rejected=0.0625)
    else:
        assert len(args) == 9 and ctl.last_photometric == dict(status=0, cost=2.0, n=7)


@pytest.mark.parametrize("tiles", [(1, 1), (4, 4)])
def test_the_hand_back_rule_of_the_controller(tiles):
    """``rejected`` above the share clears the hand-over; at the share, or with the rule off, it does not."""
    for share, rejected, kept in ((0.25, 0.2501, False), (0.25, 0.25, True), (0.25, 0.1, True), (0.0, 0.99, True), (1.0, 1.0, True)):
        calls = []
        ctl, _ = _controller(calls, rejected=rejected, photometric_tiles=tiles, photometric_handback_rejected=share, **ON)
        assert ctl._photometric_step() is kept and ctl.photometric_active is kept, (share, rejected)
        assert len(calls) == 1 and ctl.last_photometric["rejected"] == rejected
    calls = []                                                   # a status that is not OK hands back as before
    ctl, _ = _controller(calls, status=_lib.STATUS_TOO_FEW, photometric_tiles=tiles, photometric_handback_rejected=0.25, **ON)
    assert ctl._photometric_step() is False and ctl.photometric_active is False


RIG2 = [(np.eye(3), np.array([-0.1, 0.0, 0.0])), (np.eye(3), np.array([0.1, 0.0, 0.0]))]


def _fake_rig_engine(params, calls, zero_weight):
    def rig_law(*a):
        calls.append(a)
        n = len(a[0])
        return (types.SimpleNamespace(cpu=lambda: types.SimpleNamespace(numpy=lambda: np.zeros(6))),
                dict(status=0, cost=2.0, n=100 * n, zero_weight=zero_weight, gain=np.full(n, 1.1), bias=np.full(n, 3.0),
                     sigma=np.full(n, 1.5), weight=np.full(n, 35.0)))
    return types.SimpleNamespace(params=params, cfg=types.SimpleNamespace(img_size=224), apply_law_params=lambda p: None, max_pairs=4,
                                 set_goal_depth=lambda z: None, device="cpu", photometric_rig_velocity=rig_law)


def test_the_hand_back_rule_of_the_multi_controller_and_its_refusal_of_tiles():
    goal = np.zeros((24, 32, 3), np.uint8)
    small = dict(photometric_handover=0.02, lambda_=0.03, u_max=32, v_max=24, homography_depth=0.6)
    for share, zero_weight, kept in ((0.25, 51, False), (0.25, 50, True), (0.0, 199, True)):
        p = config.ServoParams(photometric_handback_rejected=share, **small, **ON)
        calls = []
        mc = servo.MultiController(_fake_rig_engine(p, calls, zero_weight), [goal, goal], params=p, rig=RIG2)
        for i in range(2):
            mc.image_callback_rgb(i, goal)
        mc.photometric_active = True
        assert mc._photometric_round([0, 1]) is kept and mc.photometric_active is kept and len(calls) == 1, (share, zero_weight)
        if share > 0:
            assert mc.last_photometric["rejected_share"] == zero_weight / 200
        else:
            assert "rejected_share" not in mc.last_photometric   # the rule off: the dict of before
    tiled = config.ServoParams(photometric_tiles=(2, 2), **small, **ON)
    with pytest.raises(ValueError, match="photometric_tiles"):
        servo.MultiController(_fake_rig_engine(tiled, [], 0), [goal, goal], params=tiled, rig=RIG2)
    with pytest.raises(ValueError, match="photometric_tiles"):   # with the hand-over off too: the field means nothing there
        servo.MultiController(_fake_rig_engine(tiled, [], 0), [goal, goal],
                              params=config.ServoParams(photometric_tiles=(2, 2), u_max=32, v_max=24, **ON))


def test_engine_checks_its_arguments_before_the_device():
    from vitvs_amd.engine import Engine, VitvsError
    eng = Engine.__new__(Engine)                               # no handle, no device: the checks come first
    f = np.zeros((24, 32, 3), np.uint8)
    K = (30.0, 30.0, 16.0, 12.0)
    with pytest.raises(VitvsError, match="uint8"):
        eng.photometric_tile_velocity_host(f.astype(np.float32), f, None, K, depth_scale=1.0)
    with pytest.raises(VitvsError, match="one shape"):
        eng.photometric_tile_velocity_host(f, f[:, :30], None, K, depth_scale=1.0)
    for bad in ((0, 2), (2, 9), (2,), 4, (2.5, 2), (True, 2), None, "22"):
        with pytest.raises(VitvsError, match="tiles"):
            eng.photometric_tile_velocity_host(f, f, None, K, depth_scale=1.0, tiles=bad)
    for bad in (-1, 5, 2.5, True):
        with pytest.raises(VitvsError, match="robust_iterations"):
            eng.photometric_tile_velocity_host(f, f, None, K, depth_scale=1.0, robust_iterations=bad)
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(VitvsError, match="sigma_min"):
            eng.photometric_tile_velocity_host(f, f, None, K, depth_scale=1.0, sigma_min=bad)
    with pytest.raises(VitvsError, match="interaction"):
        eng.photometric_tile_velocity_host(f, f, None, K, interaction="mean", depth_scale=1.0)


# ---------------------------------------------------------------------------------------------- (b) symbols and the plan
def test_the_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "vitvs.h")).read()
    lib = _lib.load()
    for name, count in (("vitvs_photometric_tile_velocity_dev", 24), ("vitvs_photometric_tile_velocity", 23),
                        ("vitvs_op_photometric_tile_plan", 6)):
        assert f"VITVS_API int {name}(" in header, name
        assert name in _lib.PROTOTYPES and getattr(lib, name) is not None, name
        assert len(_lib.PROTOTYPES[name][1]) == count
        declared = header.split(f"VITVS_API int {name}(")[1].split(");")[0]
        assert declared.count(",") + 1 == count, name
    assert len(_lib.PROTOTYPES["vitvs_photometric_robust_velocity_dev"][1]) == 22     # the robust law's prototypes stand
    assert len(_lib.PROTOTYPES["vitvs_photometric_robust_velocity"][1]) == 21
    assert _lib.ABI_VERSION == 2 and lib.vitvs_abi_version() == 2
    from vitvs_amd.engine import Engine
    assert callable(Engine.photometric_tile_velocity) and callable(Engine.photometric_tile_velocity_host)
    io = open(os.path.join(ROOT, "vit-vs_amd", "csrc", "io_layout.h")).read()
    check = open(os.path.join(ROOT, "tools", "io_layout_check.cpp")).read()
    assert "struct PhotometricTileIo" in io and "photometric_tile_io(" in check


def _plan(H, W, level, gy, gx):
    out = np.full(8, -7, np.int32)
    rc = _lib.load().vitvs_op_photometric_tile_plan(H, W, level, gy, gx, out.ctypes.data_as(C.c_void_p))
    return rc, tuple(int(x) for x in out)


def test_the_plan_equals_its_restatement():
    shapes = [(480, 640, 2, 4, 4), (480, 640, 0, 8, 8), (224, 224, 0, 2, 2), (24, 32, 0, 3, 5), (23, 29, 0, 4, 4), (70, 32, 0, 8, 2),
              (1042, 16, 1, 3, 1), (1042, 16, 1, 4, 1), (521, 16, 0, 1, 1), (4096, 4096, 0, 8, 8), (4096, 8, 0, 8, 8), (2048, 64, 1, 5, 7), (24, 8, 0, 2, 8),
              (4096, 4096, 3, 8, 8), (3, 3, 0, 3, 3)]
    for H, W, level, gy, gx in shapes:
        rc, out = _plan(H, W, level, gy, gx)
        assert rc == 0 and out == tr.plan(H, W, level, gy, gx), (H, W, level, gy, gx, out)
        h, w, rows, bands, slots = out[:5]
        assert bands * slots <= 4096 and slots == (2 if rows > 1 else 1)
        # a band touches at most two tile rows, and the second slot is the next tile row
        first = np.arange(bands) * rows
        last = np.minimum(first + rows, h) - 1
        assert np.all(last * gy // h - first * gy // h <= slots - 1)
    assert tr.plan(1042, 16, 1, 3, 1)[2:5] == (2, 261, 2) and tr.plan(480, 640, 2, 4, 4)[2:5] == (1, 120, 1)
    # 521 pooled rows in two-row bands (band b = rows 2 b, 2 b + 1).  Three tile rows begin at the even rows 174 and 348, where
    # bands begin too: no band is cut.  Four begin at 131, 261 and 391: bands 65, 130 and 195 lie across a tile-row edge.
    first = np.arange(261) * 2
    last = np.minimum(first + 2, 521) - 1
    assert [tr.plan(1042, 16, 1, g, 1)[2:5] for g in (3, 4)] == [(2, 261, 2)] * 2
    assert np.array_equal(np.nonzero(first * 3 // 521 != last * 3 // 521)[0], [])
    assert np.array_equal(np.nonzero(first * 4 // 521 != last * 4 // 521)[0], [65, 130, 195])
    assert (130 * 4 // 521, 131 * 4 // 521, 260 * 4 // 521, 261 * 4 // 521, 390 * 4 // 521, 391 * 4 // 521) == (0, 1, 1, 2, 2, 3)
    for bad in ((480, 640, 2, 0, 4), (480, 640, 2, 4, 9), (24, 32, 2, 7, 2), (24, 28, 2, 2, 8), (20, 32, 2, 6, 8), (4097, 32, 0, 2, 2),
                (24, 32, 4, 1, 1), (8, 8, 2, 1, 1)):
        rc, out = _plan(*bad)
        assert rc == -2 and out == (0,) * 8, bad
    assert _lib.load().vitvs_op_photometric_tile_plan(480, 640, 2, 4, 4, None) == -1


# ---------------------------------------------------------------------------------------------- (c) the reference itself
PARAMS = config.ServoParams(dino_input_size=224, use_feature_binning=False)
PLANE_Z, SPAN, DT = 0.61, 1.6, 0.5
LEVEL, INTER, MU, LAM, UPDATES = 2, 1, 0.01, 0.5, 40


def gain_bias(rgb, gain=1.15, bias=8.0):
    return np.clip(np.round(gain * rgb.astype(np.float64) + bias), 0, 255).astype(np.uint8)


def block(rgb):
    out = rgb.copy()
    out[120:240, 160:320] = np.kron(np.random.default_rng(5).integers(0, 256, (6, 8, 3)), np.ones((20, 20, 1))).astype(np.uint8)
    return out


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
        out = law(disturb(rgb), goal_rgb, goal_depth)
        assert out["status"] == pr.OK
        v, w = out["v"][:3], out["v"][3:]
        t = t + R @ v * DT
        R = R @ rodrigues(w * DT)
        track.append(_pose_error(R, t))
        if stop_at is not None and track[-1][0] > stop_at:
            break
    print("closed loop: pose error (cm / deg) at updates 0, 10, ..: " + "  ".join(f"{p:.4f}/{r:.4f}" for p, r in track[::10])
          + f"; the last ({len(track) - 1}) {track[-1][0]:.4f}/{track[-1][1]:.4f}")
    return track, out


def _robust(cur, goal, depth):
    return rr.velocity(cur, goal, depth, 0.0, PARAMS.intrinsics(), LEVEL, INTER, MU, LAM, 1, 4, 1.0)


def _tiles(gy, gx):
    return lambda cur, goal, depth: tr.velocity(cur, goal, depth, 0.0, PARAMS.intrinsics(), LEVEL, INTER, MU, LAM, gy, gx, 4, 1.0)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_one_tile_is_the_robust_reference_bit_for_bit(scene):
    sc, goal_rgb, goal_depth = scene
    R, t = _start()
    rgb, depth = sc.render(R, t)
    for cur, z, scalar, inter in ((rgb, goal_depth, 0.0, 1), (block(gain_bias(rgb)), depth, 0.0, 0), (rgb, None, 0.61, 1)):
        for N in (0, 4):
            for reverse in (False, True):
                want = rr.velocity(cur, goal_rgb, z, scalar, PARAMS.intrinsics(), LEVEL, inter, MU, LAM, 1, N, 1.0, reverse=reverse)
                got = tr.velocity(cur, goal_rgb, z, scalar, PARAMS.intrinsics(), LEVEL, inter, MU, LAM, 1, 1, N, 1.0, reverse=reverse)
                assert got["status"] == want["status"] == pr.OK
                assert np.array_equal(_bits(got["v"]), _bits(want["v"]))
                assert got["normal"].shape == (1, 45) and np.array_equal(_bits(got["normal"][0]), _bits(want["normal"]))
                assert np.array_equal(got["info"], want["info"])
                assert np.array_equal(_bits(got["tiles"][0, :2]), _bits(want["robust"][:2]))
                assert np.array_equal(_bits(got["robust"][2:]), _bits(want["robust"][2:])) and list(got["robust"][:2]) == [1.0, 0.0]
                assert got["tiles"][0, 2] == want["robust"][3] and got["tiles"][0, 3] == 1.0
                assert np.array_equal(_bits(got["weights"]), _bits(want["weights"]))


def test_the_tile_of_a_row():
    """k = floor(r gy / h) gx + floor(c gx / w) over the rows photometric_ref.rows keeps, holes left out."""
    Z = np.full((24, 32), 600, np.uint16)
    Z[5, 7] = 0
    k = tr.tile_of_rows((24, 32), Z, 0, 3, 5)
    assert k.shape[0] == 22 * 30 - 1
    grid = np.full((24, 32), -1)
    r, c = np.mgrid[1:23, 1:31]
    keep = ~((r == 5) & (c == 7))
    grid[r[keep], c[keep]] = k
    assert grid[1, 1] == 0 and grid[22, 30] == 14 and grid[7, 6] == 0 and grid[8, 6] == 5 and grid[8, 7] == 6 and grid[5, 7] == -1
    assert grid[15, 12] == 6 and grid[16, 13] == 12 and grid[16, 12] == 11
    assert np.array_equal(np.bincount(tr.tile_of_rows((24, 8), None, 0, 2, 8), minlength=16), [0] + [11] * 6 + [0, 0] + [11] * 6 + [0])


def test_the_robust_law_leaves_under_a_shadow(scene):
    """The need: under "shadow" the robust reference leaves twice its start error, with status OK (the prototype: 6.93 cm / 4.28
    degrees after two updates)."""
    track, _ = _loop(scene, tc.shadow, _robust, stop_at=3.0)
    assert track[-1][0] > 2 * track[0][0] and len(track) - 1 <= 2


@pytest.mark.parametrize("grid,disturb,bar", [((4, 4), "shadow", (0.32, 0.26)), ((2, 2), "shadow", (1.5, 1.3)), ((4, 4), "none", (0.18, 0.16))])
def test_the_tile_reference_loop_ends_at_the_goal(scene, grid, disturb, bar):
    """The remedy: 40 updates end below ten times the prototype's end points and no track point lies above the start.  Measured
    with this reference (cm / degrees): 4 x 4 under "shadow" 0.0316 / 0.0256, 2 x 2 under "shadow" 0.1435 / 0.1254, 4 x 4 undisturbed
    0.0180 / 0.0155."""
    track, out = _loop(scene, tc.shadow if disturb == "shadow" else (lambda rgb: rgb), _tiles(*grid))
    assert track[-1][0] < bar[0] and track[-1][1] < bar[1]
    assert max(p for p, _ in track) <= track[0][0] and max(r for _, r in track) <= track[0][1]
    gains = 1.0 + out["tiles"][:, 0].reshape(grid)
    print(f"{grid} {disturb}: live {int(out['robust'][0])}, dead {int(out['robust'][1])}, sigma {out['robust'][2]:.3f}, rows of weight 0: "
          f"{out['info'][6]} of {out['info'][0]}; gains\n{np.round(gains, 3)}")
    if disturb == "shadow" and grid == (4, 4):
        # tile (ty, tx) covers pixel rows [120 ty, 120 ty + 120) and columns [160 tx, 160 tx + 160): wholly inside the shadow where
        # its far corner is (x + 0.5 y < 380), wholly outside where its near corner is not
        for ty in range(4):
            for tx in range(4):
                if 160 * tx + 159 + 0.5 * (120 * ty + 119) < 380:
                    assert abs(gains[ty, tx] - 0.6) < 0.05, (ty, tx)
                elif 160 * tx + 0.5 * 120 * ty >= 380:
                    assert abs(gains[ty, tx] - 1.0) < 0.05, (ty, tx)


def test_a_flat_region_gives_dead_tiles(scene):
    """Goal and current frame flat over the pixel block of tiles (1, 1) and (1, 2) of a 4 x 4 grid: two dead tiles, status OK,
    gamma = beta = 0 there, and the twist is the one of the other fourteen tiles' sums alone."""
    sc, goal_rgb, goal_depth = scene
    R, t = _start()
    rgb, _ = sc.render(R, t)
    cur, goal = tc.shadow(rgb), goal_rgb.copy()
    cur[120:240, 160:480] = 90
    goal[120:240, 160:480] = 90
    for N in (0, 4):
        out = tr.velocity(cur, goal, goal_depth, 0.0, PARAMS.intrinsics(), LEVEL, INTER, MU, LAM, 4, 4, N, 1.0)
        assert out["status"] == pr.OK and list(out["robust"][:2]) == [14.0, 2.0]
        live = out["tiles"][:, 3].astype(bool)
        assert np.array_equal(np.nonzero(~live)[0], [5, 6]) and np.array_equal(out["tiles"][~live, :2], np.zeros((2, 2)))
        assert np.all(out["tile_n"][[5, 6]] == 30 * 40) and np.all(out["normal"][[5, 6], 42] > 0)       # the rows are there
        without = out["normal"].copy()
        without[[5, 6]] = 0.0
        v, _, gb, live2, solved = tr.solve_tiles(without, MU, LAM)
        assert solved and np.array_equal(live2, live) and np.array_equal(_bits(v), _bits(out["v"]))
        assert np.array_equal(_bits(gb), _bits(out["tiles"][:, :2]))
        assert out["robust"][3] == sum(out["normal"][k, 42] for k in range(16) if live[k])


def test_every_tile_flat_is_too_few(scene):
    _, goal_rgb, goal_depth = scene
    flat = np.full_like(goal_rgb, 90)
    out = tr.velocity(flat, flat, goal_depth, 0.0, PARAMS.intrinsics(), LEVEL, INTER, MU, LAM, 4, 4, 4, 1.0)
    assert out["status"] == pr.TOO_FEW and list(out["info"][5:]) == [1, 0, 0] and np.array_equal(out["v"], np.zeros(6))
    assert np.array_equal(out["robust"], np.zeros(4)) and np.array_equal(out["tiles"], np.zeros((16, 4)))
    out = tr.velocity(goal_rgb, goal_rgb, None, 0.0, PARAMS.intrinsics(), LEVEL, INTER, MU, LAM, 4, 4, 4, 1.0)
    assert out["status"] == pr.NO_DEPTH
    same = tr.velocity(goal_rgb, goal_rgb, goal_depth, 0.0, PARAMS.intrinsics(), LEVEL, INTER, MU, LAM, 4, 4, 4, 1.0)
    assert same["status"] == pr.OK and np.array_equal(same["v"], np.zeros(6)) and list(same["info"][6:]) == [0, 4]
    assert list(same["robust"]) == [16.0, 0.0, 1.0, 118.0 * 158.0]


def test_the_device_tests_cases_reach_the_paths_they_name():
    """No device result: the crops' references have status OK, the half count lies at least 3 rows inside the median bin in at
    least three quarters of the runs, and the special cases are what their names say."""
    plans = {name: tr.plan(c[0], c[1], c[2], *c[3]) for name, c in tc.CASES.items()}
    assert plans["1042x16-l1-3x1"][:5] == (521, 8, 2, 261, 2) and plans["70x32-l0-8x2"][:5] == (70, 32, 1, 70, 1)
    # a band across a tile-row edge: only bands of more than one row can lie so, and of the cases only 1042 x 16 with 4 x 1 does
    cut = {}
    for name, c in tc.CASES.items():
        h, _, rows, bands = plans[name][:4]
        first = np.arange(bands) * rows
        last = np.minimum(first + rows, h) - 1
        cut[name] = [int(b) for b in np.nonzero(first * c[3][0] // h != last * c[3][0] // h)[0]]
    assert cut["1042x16-l1-4x1"] == [65, 130, 195] and plans["1042x16-l1-4x1"][:5] == (521, 8, 2, 261, 2)
    assert all(not b for name, b in cut.items() if name != "1042x16-l1-4x1")
    edge4 = tc.reference("1042x16-l1-4x1", 4)
    assert edge4["robust"][0] == 4.0 and np.all(edge4["tile_n"] > 0)        # the rows on both sides of each cut band count
    assert plans["24x8-l0-2x8"][1] == 8 and plans["48x64-l2-8x8"][:2] == (12, 16)
    runs = [(name, N) for name in tc.CASES for N in (1, 2, 3, 4)]
    margins = []
    for name, N in runs:
        ref = tc.reference(name, N)
        assert ref["status"] == pr.OK, (name, N)
        margins.append(ref["margin_m"])
    print("margin_m per run: " + ", ".join(f"{n}/{N} {m}" for (n, N), m in zip(runs, margins)))
    assert sum(m >= 3 for m in margins) * 4 >= 3 * len(margins)
    flat = tc.reference("48x64-l2-4x4-flat", 4)
    assert flat["tiles"][5, 3] == 0.0 and flat["tile_n"][5] == 12
    edge = tc.reference("24x8-l0-2x8", 4)
    assert np.all(edge["tile_n"][[0, 7, 8, 15]] == 0) and np.all(edge["tiles"][[0, 7, 8, 15], 3] == 0) and edge["robust"][1] >= 4
    holes = tc.reference("48x64-l2-4x4-holes", 0)
    assert holes["info"][4] == 9 and holes["info"][0] == 140 - 9
