"""The pose law's fp64 statement (tests/pose_ref.py) on the CPU, and the law's host side: what the law computes
on exact points, what it buys over the image-based law at large rotations about the optical axis and with wrong matches, its
status rules, the Python arguments refused before any device call, the new symbols and the launch plan.  No GPU call.

Every bar below is the issue's; figures measured with the generators as committed are printed by the tests and quoted in §5f."""
import ctypes as C
import types

import numpy as np
import pytest

import pose_ref as pr
import vitvs_amd  # noqa: F401
from vitvs_amd import _lib, config

LDS_CAP = 160 * 1024
ANGLES = (0.1, 1.0, 3.0, 3.1415)


def _seeded_pose(rng, angle):
    return pr.rodrigues(pr.unit(rng.standard_normal(3)) * angle), rng.uniform(-0.1, 0.1, 3)


def test_exact_recovery_on_coplanar_points():
    """64 seeded poses at each of four rotation angles, 8 coplanar points at 0.61 m: R and t to 1e-12."""
    worst, gap = 0.0, np.inf
    for angle in ANGLES:
        for seed in range(64):
            rng = np.random.default_rng(1000 + seed)
            R, t = _seeded_pose(rng, angle)
            Q = np.concatenate([rng.uniform(-0.25, 0.25, (8, 2)), np.full((8, 1), 0.61)], 1)
            P = pr.points_in_camera(Q, R, t)
            h = pr.horn(P, Q, np.ones(8))
            worst = max(worst, np.abs(h["R"] - R).max(), np.abs(h["t"] - t).max())
            gap = min(gap, h["gap"] / h["scatter"])
            assert not h["degenerate"] and abs(np.linalg.det(h["R"]) - 1.0) < 1e-12
            out = pr.pose_law(P, Q, np.ones(8), 0.7, 0)
            assert out["status"] == pr.OK and out["info"][0] == 8
            th = angle * pr.unit(pr.theta_u(h["q"]))
            assert np.allclose(out["v"], -0.7 * np.concatenate([R.T @ t, th]), atol=1e-12)
    print(f"exact recovery: worst |R|, |t| miss {worst:.2e}; smallest relative eigen-gap {gap:.3f}")
    assert worst <= 1e-12 and gap > 1e-6


def test_collinear_points_have_no_gap():
    line = np.outer(np.linspace(-0.3, 0.3, 8), pr.unit([1.0, 2.0, 0.5])) + np.array([0.0, 0.0, 0.61])
    R, t = _seeded_pose(np.random.default_rng(5), 1.0)
    h = pr.horn(pr.points_in_camera(line, R, t), line, np.ones(8))
    assert h["gap"] / h["scatter"] < 1e-12 and h["degenerate"]


GRID = np.array([[x, y, 0.61] for y in np.linspace(-0.2, 0.2, 5) for x in np.linspace(-0.2, 0.2, 5)])
T0 = np.array([0.04, -0.03, 0.03])                         # 5.8 cm from the goal, t_z = 0.03


def _start(turn_deg):
    Rz = pr.rodrigues(np.array([0.0, 0.0, np.deg2rad(turn_deg)]))
    return Rz @ pr.rodrigues(pr.unit([1.0, 0.5, 0.0]) * np.deg2rad(3.0)), T0.copy()


def _closed_loop(law, turn_deg, steps=400, lam=1.0, dt=0.05):
    R, t = _start(turn_deg)
    tz, ts, ths = [t[2]], [np.linalg.norm(t)], []
    for _ in range(steps):
        P = pr.points_in_camera(GRID, R, t)
        if law == "pose":
            out = pr.pose_law(P, GRID, np.ones(len(GRID)), lam, 0)
            assert out["status"] == pr.OK
            v = out["v"]
            ths.append(np.linalg.norm(v[3:]) / lam)
        else:
            v = pr.ibvs_velocity(P, GRID, lam)
        R, t = pr.step(R, t, v, dt)
        if not np.isfinite(t).all() or np.linalg.norm(t) > 1e3:
            break
        tz.append(t[2])
        ts.append(np.linalg.norm(t))
    return dict(t=t, R=R, tz=np.array(tz), ts=np.array(ts), ths=np.array(ths))


def test_translation_and_angle_decay_geometrically():
    """|t_k| = (1 - lambda dt)^k |t_0| and the same for theta: a straight line and a turn about a fixed axis."""
    for turn in (5.0, 90.0, 170.0):
        run = _closed_loop("pose", turn, steps=11)
        k = np.arange(11)
        assert np.abs(run["ts"][:11] - 0.95 ** k * run["ts"][0]).max() <= 1e-9
        assert np.abs(run["ths"][:11] - 0.95 ** k * run["ths"][0]).max() <= 1e-9


@pytest.mark.parametrize("turn", [5.0, 90.0, 170.0, 179.9])
def test_closed_loop_ends_without_a_retreat(turn):
    run = _closed_loop("pose", turn)
    end = float(np.linalg.norm(run["t"]))
    print(f"pose law, {turn} deg about the optical axis: ends at {end:.2e} m, t_z within [{run['tz'].min():.4f}, {run['tz'].max():.4f}]")
    assert end < 1e-6 and run["tz"].min() >= -1e-9


def test_the_image_based_law_retreats_at_170_degrees():
    lows = {turn: float(_closed_loop("ibvs", turn)["tz"].min()) for turn in (90.0, 170.0)}
    print(f"image-based law, lowest t_z: 90 deg {lows[90.0]:.2f} m, 170 deg {lows[170.0]:.2f} m")
    assert lows[170.0] < -1.0


def test_half_turn_of_a_symmetric_grid():
    lam = 0.7
    P = pr.points_in_camera(GRID, pr.rodrigues(np.array([0.0, 0.0, np.pi])), np.zeros(3))
    out = pr.pose_law(P, GRID, np.ones(len(GRID)), lam, 0)
    assert out["status"] == pr.OK
    assert abs(abs(out["v"][5]) - np.pi * lam) <= 1e-9 and np.abs(out["v"][:3]).max() <= 1e-9 and np.abs(out["v"][3:5]).max() <= 1e-9
    # the image-based law sees e = s - s* through the centre: no rotation at all
    assert np.abs(pr.ibvs_velocity(P, GRID, lam)[3:]).max() <= 1e-9


# sigma_min of the default configuration (ViT-S/14 at 308, 640 x 480, f = 502.3): half a patch pitch at the median goal depth
_PARAMS = config.ServoParams()
PITCH_U, PITCH_V = 14 * _PARAMS.u_max / 308, 14 * _PARAMS.v_max / 308


def _outlier_case(seed):
    rng = np.random.default_rng(7000 + seed)
    R, t = pr.rodrigues(pr.unit(rng.standard_normal(3)) * rng.uniform(0.05, 0.6)), rng.uniform(-0.08, 0.08, 3)
    Z = rng.uniform(0.5, 0.8, 24)
    Q = np.stack([rng.uniform(-0.4, 0.4, 24) * Z, rng.uniform(-0.3, 0.3, 24) * Z, Z], 1)
    P = pr.points_in_camera(Q, R, t) + rng.standard_normal((24, 3)) * 0.002
    bad = rng.choice(24, 6, replace=False)
    P[bad] += np.stack([pr.unit(d) for d in rng.standard_normal((6, 3))]) * rng.uniform(0.1, 0.4, (6, 1))
    smin = 0.5 * max(PITCH_U / _PARAMS.f_x, PITCH_V / _PARAMS.f_y) * pr.median_middle(Q[:, 2])
    return P, Q, bad, R, t, smin


def _angle(Ra, Rb):
    return float(np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1.0) / 2.0, -1.0, 1.0))))


def test_wrong_matches_are_rejected():
    """64 seeded cases of 24 pairs, 2 mm noise, 6 gross outliers of 0.1 - 0.4 m, 4 re-weightings."""
    plain, robust, rot_plain, rot_robust = [], [], [], []
    for seed in range(64):
        P, Q, bad, R, t, smin = _outlier_case(seed)
        a, b = pr.pose_law(P, Q, np.ones(24), 1.0, 0, smin), pr.pose_law(P, Q, np.ones(24), 1.0, 4, smin)
        assert a["status"] == b["status"] == pr.OK and b["info"][2] == 4
        plain.append(np.linalg.norm(a["t"] - t))
        robust.append(np.linalg.norm(b["t"] - t))
        rot_plain.append(_angle(a["R"], R))
        rot_robust.append(_angle(b["R"], R))
        good = np.setdiff1d(np.arange(24), bad)
        assert (b["weights"][bad] == 0.0).all(), (seed, b["weights"][bad])
        assert (b["weights"][good] > 0.0).all(), (seed, b["weights"][good].min())
        assert b["info"][3] == 6
    ratio = np.array(robust) / np.array(plain)
    for name, m in (("plain", plain), ("4 re-weightings", robust)):
        print(f"translation miss, {name}: min {min(m):.4f} median {np.median(m):.4f} max {max(m):.4f} m")
    print(f"rotation miss, median: plain {np.median(rot_plain):.2f} deg, robust {np.median(rot_robust):.2f} deg; "
          f"robust / plain translation miss: largest {ratio.max():.3f}")
    assert (ratio < 0.5).sum() == 64, ratio.max()


def _cloud(seed, n=12):
    rng = np.random.default_rng(seed)
    R, t = _seeded_pose(rng, 0.8)
    Q = np.stack([rng.uniform(-0.3, 0.3, n), rng.uniform(-0.2, 0.2, n), rng.uniform(0.5, 0.8, n)], 1)
    return pr.points_in_camera(Q, R, t), Q, R, t


def test_status_holes_are_dropped():
    P, Q, R, t = _cloud(11)
    usable = np.ones(12, np.int32)
    usable[[2, 7]] = -1
    usable[11] = 0
    P[[2, 7, 11]] = 1e6                                     # whatever an unusable row holds cannot reach the pose
    out = pr.pose_law(P, Q, usable, 1.0, 0)
    keep = usable > 0
    same = pr.pose_law(P[keep], Q[keep], np.ones(int(keep.sum())), 1.0, 0)
    assert out["status"] == pr.OK and list(out["info"][[0, 5]]) == [9, 2]
    assert np.abs(out["R"] - R).max() <= 1e-12 and np.abs(out["v"] - same["v"]).max() <= 1e-12


def test_status_too_few_rows():
    P, Q, _, _ = _cloud(12)
    for n_us in (0, 1, 2):
        usable = np.zeros(12, np.int32)
        usable[:n_us] = 1
        out = pr.pose_law(P, Q, usable, 1.0, 0)
        assert out["status"] == pr.TOO_FEW and np.array_equal(out["v"], np.zeros(6)) and np.array_equal(out["R"], np.eye(3))
        assert out["info"][0] == n_us and out["info"][4] == 0
    usable[:3] = 1
    assert pr.pose_law(P, Q, usable, 1.0, 0)["status"] == pr.OK


def test_status_collinear_clouds_are_degenerate():
    line = np.outer(np.linspace(-0.3, 0.3, 9), pr.unit([1.0, -1.0, 0.2])) + np.array([0.0, 0.0, 0.6])
    R, t = _seeded_pose(np.random.default_rng(3), 0.5)
    out = pr.pose_law(pr.points_in_camera(line, R, t), line, np.ones(9), 1.0, 0)
    assert out["status"] == pr.TOO_FEW and out["info"][4] == 1 and np.array_equal(out["v"], np.zeros(6))
    # ... and a cloud that is degenerate only once its outliers are gone: 9 collinear inliers and 3 points far off the line
    P, Q = pr.points_in_camera(line, R, t), line.copy()
    P = np.concatenate([P, P[:3] + np.array([[0.3, 0.2, 0.1], [-0.2, 0.3, 0.2], [0.1, -0.3, 0.25]])])
    Q = np.concatenate([Q, Q[:3] + np.array([[-0.2, 0.3, -0.1], [0.3, 0.1, 0.2], [-0.1, -0.2, 0.3]])])
    plain, robust = pr.pose_law(P, Q, np.ones(12), 1.0, 0, 0.01), pr.pose_law(P, Q, np.ones(12), 1.0, 8, 0.01)
    assert plain["status"] == pr.OK
    assert robust["status"] == pr.TOO_FEW and robust["info"][4] == 1 and robust["info"][3] >= 3


def test_status_same_image_and_camera_failures():
    rows, T = 6, 16
    det = dict(selected=np.arange(rows, dtype=np.int32)[None], s_uv=np.zeros((1, rows, 4), np.int32),
               feat=np.ones((1, rows, 4)), info=np.array([[6, 6, 1, 6, 0, 12, 0, 0]], np.int32))
    table = np.full(T + 1, 610, np.uint16)
    K = _PARAMS.intrinsics()
    out = pr.pose_from_details(det, 0, 0, K, table, 1.0, 0, PITCH_U, PITCH_V)
    assert out["status"] == pr.OK and np.array_equal(out["v"], np.zeros(6)) and np.array_equal(out["R"], np.eye(3))
    for cam in (1, 2, 3):
        out = pr.pose_from_details(det, 0, cam, K, table, 1.0, 0, PITCH_U, PITCH_V)
        assert out["status"] == cam and np.array_equal(out["v"], np.zeros(6))


def test_points_from_details():
    """Rows past info[1], padded rows, a hole in either depth."""
    K = (500.0, 400.0, 320.0, 240.0)
    sel = np.array([3, 5, -1, 7, 9, 2], np.int32)
    s_uv = np.array([[420, 340, 0, 0], [320, 240, 0, 0], [0, 0, 0, 0], [100, 100, 0, 0], [200, 200, 0, 0], [1, 1, 0, 0]], np.int32)
    feat = np.array([[0.5, 0.1, -0.2, 1], [100.0, 0, 0, 1], [100.0, 0, 0, 0], [0.7, 0.3, 0.1, 1], [0.6, 0, 0, 1], [0.6, 0, 0, 1]])
    table = np.full(17, 800, np.uint16)
    table[9] = 0
    P, Q, us = pr.points_from_details(sel, s_uv, feat, 5, K, table)
    assert list(us) == [1, -1, 0, 1, -1, 0]
    assert np.allclose(P[0], [0.05, -0.1, 0.5]) and np.allclose(Q[0], [0.8 * 0.2, 0.8 * 0.25, 0.8])


# ---------------------------------------------------------------------------------------------- the host side of the library
def test_servo_params_validation():
    p = config.ServoParams()
    assert p.law == "ibvs" and p.pose_robust_iterations == 0
    assert config.ServoParams(law="pose", pose_robust_iterations=16).pose_robust_iterations == 16
    for bad in (-1, 17):
        with pytest.raises(ValueError):
            config.ServoParams(pose_robust_iterations=bad)
    with pytest.raises(ValueError):
        config.ServoParams(law="pbvs")
    cfg = {k: 1 for k in config._REQUIRED_KEYS}
    cfg["image_path"] = "goal.png"
    assert config.load_reference_config(cfg).servo.law == "ibvs"
    cfg.update(law="pose", pose_robust_iterations=4)
    got = config.load_reference_config(cfg)
    assert got.servo.law == "pose" and got.servo.pose_robust_iterations == 4 and "law" not in got.extras


def test_the_controllers_refuse_what_the_pose_law_cannot_do():
    from vitvs_amd import pipeline, servo
    pose = config.ServoParams(law="pose")
    eng = types.SimpleNamespace(params=pose, cfg=types.SimpleNamespace(img_size=224), apply_law_params=lambda p: None,
                                max_pairs=4, set_goal_depth=lambda z: None)
    with pytest.raises(ValueError, match="goal_depth"):
        servo.Controller(eng, goal_image=None, params=pose)
    with pytest.raises(ValueError, match="desired"):
        servo.Controller(eng, goal_image=None, params=pose.replace(interaction="desired"), goal_depth=np.zeros((480, 640), np.uint16))
    ctl = servo.Controller(eng, goal_image=None, params=pose, goal_depth=np.zeros((480, 640), np.uint16))
    assert ctl.last_pose_status is None and ctl.last_pose is None
    with pytest.raises(ValueError, match="pose"):
        servo.MultiController(eng, [None, None], params=pose)
    with pytest.raises(ValueError, match="pose"):
        pipeline.UpdatePipeline(config.baseline_config("vits16_224"), pose, {})


def test_engine_pose_velocity_checks_its_arguments_before_the_device():
    from vitvs_amd.engine import Engine
    eng = Engine.__new__(Engine)                               # no handle, no device: the checks come first
    for call in (eng.pose_velocity, eng.pose_velocity_host):
        for bad in (-1, 17):
            with pytest.raises(ValueError, match="0 .. 16"):
                call((600.0, 600.0, 320.0, 240.0), np.zeros(1, np.int32), robust_iterations=bad)


def test_the_new_symbols_load():
    lib = _lib.load()
    for name in ("vitvs_pose_velocity_dev", "vitvs_pose_velocity", "vitvs_op_pose_law", "vitvs_op_pose_scratch_bytes",
                 "vitvs_op_pose_plan"):
        assert name in _lib.PROTOTYPES and getattr(lib, name) is not None, name
    assert _lib.ABI_VERSION == 2 and lib.vitvs_abi_version() == 2


def _plan(max_rows, n_iter):
    """dynamic LDS in doubles: 8 slices x 32 quantities + 64 results | rho, w [max_rows] for the robust form"""
    lds = 8 * (320 + (2 * max_rows if n_iter > 0 else 0))
    return lds, int(n_iter > 0), int(lds > 64 * 1024)


def _call(max_rows, n_iter):
    out = (C.c_int32 * 3)(-1, -1, -1)
    return _lib.load().vitvs_op_pose_plan(max_rows, n_iter, out), tuple(out)


@pytest.mark.parametrize("shape", [(1, 0), (24, 0), (24, 4), (3136, 0), (3136, 16), (4000, 1), (4100, 1), (100000, 0)])
def test_plan_equals_its_formula(shape):
    rc, out = _call(*shape)
    assert rc == 0 and out == _plan(*shape), (shape, rc, out)


def test_plan_on_both_sides_of_160_kib():
    most = (LDS_CAP // 8 - 320) // 2
    assert _call(most, 4) == (0, _plan(most, 4)) and _plan(most, 4)[0] <= LDS_CAP
    rc, out = _call(most + 1, 4)
    assert rc == -3 and out == _plan(most + 1, 4) and out[0] > LDS_CAP
    assert _call(most + 1, 0)[0] == 0                          # the plain form keeps nothing per row in LDS


def test_plan_and_scratch_refuse_bad_arguments():
    lib = _lib.load()
    for max_rows, n_iter in ((0, 0), (-3, 4), (24, -1), (24, 17)):
        assert _call(max_rows, n_iter)[0] == -2, (max_rows, n_iter)
    assert lib.vitvs_op_pose_plan(24, 4, None) == -1
    for n, ld in ((0, 24), (1, 0), (-1, 24)):
        assert lib.vitvs_op_pose_scratch_bytes(n, ld) == -2
    for n, ld in ((1, 3), (3, 24), (1, 1100)):
        assert lib.vitvs_op_pose_scratch_bytes(n, ld) == 8 * 7 * n * ld
