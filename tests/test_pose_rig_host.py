"""The pose rig law's fp64 statement (tests/pose_rig_ref.py) on the CPU, and the law's host side: what one alignment
over the whole rig buys over the pose law per camera, its equivalences and status rules, the closed loop on exact points, the
Python arguments refused before any device call, the new symbols and the launch plan.  No GPU call.

Every bar below is the issue's; figures measured with the generators as committed are printed by the tests and quoted in §5g."""
import ctypes as C
import types

import numpy as np
import pytest

import pose_ref as pr
import pose_rig_ref as rr
import vitvs_amd  # noqa: F401
from vitvs_amd import _lib, config

LDS_CAP = 160 * 1024


def _stats(x):
    return f"{min(x):.3g} / {float(np.median(x)):.3g} / {max(x):.3g}"


# ---------------------------------------------------------------------------------------------- the two tables
def test_cameras_that_cannot_solve_alone():
    """Three cameras with 2 usable points each: every camera alone is TOO_FEW, one alignment of the 6 points in the rig frame
    recovers the true rig twist to 1e-12 relative, 64 seeded cases."""
    worst, gap = 0.0, np.inf
    for seed in range(64):
        rng = np.random.default_rng(8000 + seed)
        rig = rr.seeded_rig(rng, 3)
        R, t = rr.seeded_displacement(rng)
        X = np.concatenate([rng.uniform(-0.4, 0.4, (3, 2, 2)), rng.uniform(0.5, 1.0, (3, 2, 1))], 2)
        P, Q = rr.camera_points(X, rig, R, t)
        usable = np.ones((3, 2), np.int32)
        v_avg, alone = rr.per_camera_average(P, Q, usable, rig)
        assert alone == [pr.TOO_FEW] * 3 and v_avg is None
        out = rr.pose_rig_law(P, Q, usable, rig, None, 1.0, 0)
        assert out["status"] == pr.OK and list(out["info"][:2]) == [3, 6]
        worst = max(worst, rr.rel_miss(out["v"], rr.true_twist(R, t, 1.0)))
        gap = min(gap, min(out["gaps"]))
    print(f"2 points per camera: worst relative miss of the rig twist {worst:.2e}; smallest relative eigen-gap {gap:.3f}")
    assert worst <= 1e-12


def test_outliers_concentrated_in_one_camera():
    """3 cameras x 16 pairs, 2 mm noise, 6 gross outliers of 0.1 .. 0.4 m all in camera 0, N = 4, 64 seeded cases: every planted
    outlier ends at weight 0, robust / plain < 0.5 in 64 of 64, and the per-camera robust laws averaged miss by more (median)."""
    plain, robust, average = [], [], []
    for seed in range(64):
        c = rr.outlier_case(seed)
        v_true = rr.true_twist(c["R"], c["t"], 1.0)
        a = rr.pose_rig_law(c["P"], c["Q"], c["usable"], c["rig"], None, 1.0, 0, 0.002)
        b = rr.pose_rig_law(c["P"], c["Q"], c["usable"], c["rig"], None, 1.0, 4, 0.002)
        v_avg, _ = rr.per_camera_average(c["P"], c["Q"], c["usable"], c["rig"], 1.0, 4, 0.002)
        assert a["status"] == pr.OK and b["status"] == pr.OK and b["info"][3] == 4
        assert (b["weights"][0, c["planted"]] == 0.0).all(), seed
        plain.append(rr.rel_miss(a["v"], v_true))
        robust.append(rr.rel_miss(b["v"], v_true))
        average.append(rr.rel_miss(v_avg, v_true))
        assert robust[-1] / plain[-1] < 0.5, (seed, robust[-1], plain[-1])
    print(f"relative miss of the rig twist, min / median / max: plain stack {_stats(plain)}; per-camera robust laws averaged "
          f"{_stats(average)}; one Tukey IRLS over the stack {_stats(robust)}; worst robust / plain "
          f"{max(r / p for r, p in zip(robust, plain)):.3f}")
    assert np.median(average) > np.median(robust)


# ---------------------------------------------------------------------------------------------- equivalences
def test_one_camera_at_the_rig_origin_is_the_pose_law():
    for seed in range(8):
        rng = np.random.default_rng(8100 + seed)
        R, t = rr.seeded_displacement(rng)
        X = np.concatenate([rng.uniform(-0.3, 0.3, (1, 12, 2)), rng.uniform(0.5, 1.0, (1, 12, 1))], 2)
        ident = [(np.eye(3), np.zeros(3))]
        P, Q = rr.camera_points(X, ident, R, t)
        P = P + 0.002 * rng.standard_normal(P.shape)
        usable = np.ones((1, 12), np.int32)
        usable[0, 3], usable[0, 7] = -1, 0
        for n_iter in (0, 4):
            one = pr.pose_law(P[0], Q[0], usable[0], 0.7, n_iter, 0.001)
            rig = rr.pose_rig_law(P, Q, usable, ident, None, 0.7, n_iter, 0.001)
            assert rig["status"] == one["status"] == pr.OK
            assert np.abs(rig["v"] - one["v"]).max() <= 1e-12 and np.abs(rig["weights"][0] - one["weights"]).max() <= 1e-12
            assert list(rig["info"]) == [1] + list(one["info"][:6]) + [0]


def test_a_camera_that_does_not_contribute_changes_nothing():
    c = rr.outlier_case(3)
    base = rr.pose_rig_law(c["P"], c["Q"], c["usable"], c["rig"], None, 1.0, 4, 0.002)
    extra_P = np.concatenate([c["P"], 5.0 + c["P"][:1]])
    extra_Q = np.concatenate([c["Q"], c["Q"][:1]])
    usable = np.ones((4, 16), np.int32)
    rig = c["rig"] + [(pr.rodrigues([0.3, 0.2, 0.1]), np.array([0.5, 0.5, 0.5]))]
    for bad, same in ((pr.TOO_FEW, 0), (1, 0), (pr.OK, 1)):          # a failed camera, or one at its goal by the shortcut
        out = rr.pose_rig_law(extra_P, extra_Q, usable, rig, [0, 0, 0, bad], 1.0, 4, 0.002, same=[0, 0, 0, same])
        assert out["status"] == pr.OK and np.abs(out["v"] - base["v"]).max() <= 1e-12
        assert list(out["info"][:7]) == list(base["info"][:7]) and out["info"][7] == bad
        assert (out["weights"][3] == 0.0).all() and np.abs(out["weights"][:3] - base["weights"]).max() <= 1e-12
        assert np.abs(out["moments"] - base["moments"]).max() <= 1e-12


# ---------------------------------------------------------------------------------------------- status cases
def test_status_cases():
    c = rr.outlier_case(1)
    P, Q, usable, rig = c["P"], c["Q"], c["usable"], c["rig"]
    # every camera at its goal by the same-image shortcut: OK and zero
    out = rr.pose_rig_law(P, Q, usable, rig, [0, 0, 0], 1.0, 0, same=[1, 1, 1])
    assert out["status"] == pr.OK and np.array_equal(out["v"], np.zeros(6)) and np.array_equal(out["R"], np.eye(3))
    assert list(out["info"]) == [0] * 8 and np.array_equal(out["moments"], np.zeros(18))
    # nobody contributes: the largest camera status
    out = rr.pose_rig_law(P, Q, usable, rig, [1, 3, 2], 1.0, 0)
    assert out["status"] == 3 and np.array_equal(out["v"], np.zeros(6)) and out["info"][7] == 3
    # fewer than 3 usable rows over the whole stack
    few = np.zeros_like(usable)
    few[0, 2], few[2, 5] = 1, 1
    out = rr.pose_rig_law(P, Q, few, rig, None, 1.0, 0)
    assert out["status"] == pr.TOO_FEW and np.array_equal(out["v"], np.zeros(6)) and list(out["info"][:2]) == [3, 2]
    # a collinear stack: the cameras' points lie on ONE line of the rig frame
    line = np.outer(np.linspace(-0.3, 0.3, 12), rr.unit([1.0, 2.0, 0.5])) + np.array([0.0, 0.0, 0.8])
    X = line.reshape(3, 4, 3)
    R, t = rr.seeded_displacement(np.random.default_rng(5), 0.2)
    Pl, Ql = rr.camera_points(X, rig, R, t)
    out = rr.pose_rig_law(Pl, Ql, np.ones((3, 4), np.int32), rig, None, 1.0, 0)
    assert out["status"] == pr.TOO_FEW and out["info"][5] == 1 and np.array_equal(out["v"], np.zeros(6))
    assert max(out["gaps"]) <= 1e-10


def test_the_handle_form_builds_the_same_stack():
    """pose_rig_from_details: rows past info[1], holes, one table for all or one per camera, sigma_min over contributing cameras."""
    rows, T = 6, 16
    rng = np.random.default_rng(11)
    n = 3
    det = dict(selected=np.tile(np.array([3, 5, -1, 7, 9, 2], np.int32), (n, 1)),
               s_uv=rng.integers(50, 400, (n, rows, 4)).astype(np.int32),
               feat=np.concatenate([rng.uniform(0.5, 0.9, (n, rows, 1)), rng.uniform(-0.3, 0.3, (n, rows, 2)), np.ones((n, rows, 1))], 2),
               info=np.array([[6, 5, 0, 5, 0, 10, 0, 0]] * n, np.int32))
    det["feat"][1, 1, 0] = 100.0                                        # a hole in the current depth
    tables = np.full((n, T + 1), 800, np.uint16)
    tables[2, 9] = 0                                                    # a hole in camera 2's goal depth
    K = np.array([[500.0, 400.0, 320.0, 240.0], [600.0, 600.0, 320.0, 240.0], [300.0, 300.0, 320.0, 240.0]])
    rig = rr.toe_in_rig(3)
    out = rr.pose_rig_from_details(det, [0, 0, 0], rig, K, tables, 1.0, 2, 45.7, 34.3)
    assert out["status"] == pr.OK and list(out["info"][[0, 1, 6]]) == [3, 10, 2]
    assert (out["weights"][:, 2] == 0).all() and (out["weights"][:, 5] == 0).all()
    one = rr.pose_rig_from_details(det, [0, 0, 0], rig, K, tables[:1], 1.0, 2, 45.7, 34.3)
    assert list(one["info"][[0, 1, 6]]) == [3, 11, 1]
    # the floor of the scale takes the coarsest pixel of the CONTRIBUTING cameras only: camera 2 (f = 300) out, the floor drops
    big = rr.pose_rig_from_details(det, [0, 0, 0], rig, K, tables, 1.0, 1, 45.7, 34.3)["sigma_min"]
    small = rr.pose_rig_from_details(det, [0, 0, 2], rig, K, tables, 1.0, 1, 45.7, 34.3)["sigma_min"]
    assert big == 0.5 * (45.7 / 300.0) * 0.8 and small == 0.5 * (45.7 / 500.0) * 0.8


# ---------------------------------------------------------------------------------------------- the closed loop
@pytest.mark.parametrize("turn_deg", (5.0, 90.0, 170.0))
def test_closed_loop_on_exact_points(turn_deg):
    """Three cameras 0.15 m apart with 10 degrees of toe-in, 4 x 3 points per camera on z = 0.61, lambda 1, dt 0.05, 100 steps from
    a 3 degree tilt, a turn about the rig's z axis and t = (0.03, -0.04, 0.03): |t| and theta are 0.95^k of their start to 1e-9
    and the rig's t_z stays in [0, 0.03]."""
    rig = rr.toe_in_rig(3, 0.15, 10.0)
    grid = np.array([[x, y, 0.61] for y in np.linspace(-0.1, 0.1, 3) for x in np.linspace(-0.15, 0.15, 4)])
    X = np.stack([grid + np.array([ti[0], 0.0, 0.0]) for _, ti in rig])
    R = pr.rodrigues([0.0, 0.0, np.radians(turn_deg)]) @ pr.rodrigues([np.radians(3.0), 0.0, 0.0])
    t = np.array([0.03, -0.04, 0.03])
    usable = np.ones((3, 12), np.int32)
    t0, th0, worst = np.linalg.norm(t), None, 0.0
    for k in range(101):
        P, Q = rr.camera_points(X, rig, R, t)
        out = rr.pose_rig_law(P, Q, usable, rig, None, 1.0, 0)
        assert out["status"] == pr.OK
        th = np.linalg.norm(out["v"][3:])
        th0 = th if th0 is None else th0
        worst = max(worst, abs(np.linalg.norm(t) / t0 - 0.95 ** k), abs(th / th0 - 0.95 ** k))
        assert 0.0 <= t[2] <= 0.03, (k, t[2])
        R, t = pr.step(R, t, out["v"], 0.05)
    print(f"closed loop, turn {turn_deg:g} deg (theta_0 {np.degrees(th0):.2f}): worst miss of 0.95^k in |t| and theta {worst:.2e}")
    assert worst <= 1e-9


# ---------------------------------------------------------------------------------------------- the host side of the library
def test_servo_params_field():
    assert config.ServoParams().rig_pose_robust_iterations == 0
    assert config.ServoParams(rig_pose_robust_iterations=16).rig_pose_robust_iterations == 16
    for bad in (-1, 17):
        with pytest.raises(ValueError, match="rig_pose_robust_iterations"):
            config.ServoParams(rig_pose_robust_iterations=bad)
    cfg = {k: 1 for k in config._REQUIRED_KEYS}
    cfg["image_path"] = "goal.png"
    assert config.load_reference_config(cfg).servo.rig_pose_robust_iterations == 0
    cfg.update(rig_pose_robust_iterations=4)
    got = config.load_reference_config(cfg)
    assert got.servo.rig_pose_robust_iterations == 4 and "rig_pose_robust_iterations" not in got.extras


def test_the_controllers_refuse_what_the_pose_rig_law_cannot_do():
    from vitvs_amd import pipeline, servo
    pose = config.ServoParams(law="pose")
    seen = []
    eng = types.SimpleNamespace(params=pose, cfg=types.SimpleNamespace(img_size=224), apply_law_params=lambda p: None,
                                max_pairs=4, set_goal_depth=lambda z: seen.append(np.asarray(z).shape))
    rig = rr.toe_in_rig(2)
    depth = np.zeros((480, 640), np.uint16)
    with pytest.raises(ValueError, match="pose"):
        servo.MultiController(eng, [None, None], params=pose)                              # no rig=
    with pytest.raises(ValueError, match="pose"):
        servo.MultiController(eng, [None, None], params=pose, goal_depth=depth)            # no rig=, with a goal depth
    with pytest.raises(ValueError, match="goal_depth"):
        servo.MultiController(eng, [None, None], params=pose, rig=rig)
    with pytest.raises(ValueError, match="desired"):
        servo.MultiController(eng, [None, None], params=pose.replace(interaction="desired"), rig=rig, goal_depth=depth)
    with pytest.raises(ValueError, match="one per camera"):
        servo.MultiController(eng, [None, None], params=pose, rig=rig, goal_depth=np.zeros((3, 480, 640), np.uint16))
    pipe = pipeline.UpdatePipeline.__new__(pipeline.UpdatePipeline)
    pipe.engines = [eng]
    with pytest.raises(ValueError, match="Engine backend"):
        servo.MultiController(pipe, [None, None], params=pose, goal_depth=depth)
    with pytest.raises(ValueError, match="Engine backend"):
        servo.MultiController(pipe, [None, None], params=pose, rig=rig, goal_depth=depth)
    with pytest.raises(ValueError, match="pose"):
        pipeline.UpdatePipeline(config.baseline_config("vits16_224"), pose, {})
    # ... and what it accepts: the cameras keep the image-based law, the controller the pose rig law
    for gd in (depth, np.zeros((2, 480, 640), np.uint16)):
        mc = servo.MultiController(eng, [None, None], params=pose, rig=rig, goal_depth=gd)
        assert mc.law == "pose" and mc.params.law == "pose" and all(c.params.law == "ibvs" for c in mc.cameras)
        assert mc.rig_pose is None and mc.rig_status is None and seen[-1] == gd.shape
    ibvs = servo.MultiController(eng, [None, None], params=config.ServoParams(), rig=rig)
    assert ibvs.law == "ibvs" and ibvs.rig_W.shape == (2, 6, 6)


def test_engine_pose_rig_velocity_checks_its_arguments_before_the_device():
    from vitvs_amd.engine import Engine
    eng = Engine.__new__(Engine)                               # no handle, no device: the checks come first
    rig = rr.toe_in_rig(2)
    K = (600.0, 600.0, 320.0, 240.0)
    for call in (eng.pose_rig_velocity, eng.pose_rig_velocity_host):
        for bad in (-1, 17):
            with pytest.raises(ValueError, match="0 .. 16"):
                call(rig, K, np.zeros(2, np.int32), robust_iterations=bad)
        with pytest.raises(ValueError, match="status"):
            call(rig, K, np.zeros(3, np.int32))
        with pytest.raises(ValueError, match="per camera"):
            call(rig, np.zeros((3, 4)), np.zeros(2, np.int32))
        with pytest.raises(ValueError, match="R_i"):
            call([(np.eye(2), np.zeros(3))], K, np.zeros(1, np.int32))
        with pytest.raises(ValueError, match="R_i"):
            call([], K, np.zeros(0, np.int32))


def test_dist_refuses_the_robust_form_and_wrong_moments():
    import torch
    from vitvs_amd import dist
    with pytest.raises(ValueError, match="robust"):
        dist.pose_rig_velocity(torch.zeros(18, dtype=torch.float64), 1.0, robust_iterations=1)
    with pytest.raises(ValueError, match="18"):
        dist.pose_rig_velocity(torch.zeros(17, dtype=torch.float64), 1.0)


def test_new_symbols_and_the_launch_plan():
    lib = _lib.load()
    for name in ("vitvs_pose_rig_velocity_dev", "vitvs_pose_rig_velocity", "vitvs_op_pose_rig_law", "vitvs_op_pose_rig_scratch_bytes",
                 "vitvs_op_pose_rig_plan"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    out = (C.c_int32 * 3)()
    for n_cams, ld in ((1, 3), (2, 24), (8, 24), (3, 258), (5, 260), (2, 1024), (8, 1260), (8, 1261), (1, 10080), (1, 10081), (256, 48)):
        for n_iter in (0, 1, 4, 16):
            want = 8 * (320 + (2 * n_cams * ld if n_iter > 0 else 0))
            rc = lib.vitvs_op_pose_rig_plan(n_cams, ld, n_iter, out)
            assert rc == (-3 if want > LDS_CAP else 0), (n_cams, ld, n_iter)
            assert list(out) == [want, int(n_iter > 0), int(want > 64 * 1024)], (n_cams, ld, n_iter, list(out))
    assert 8 * (320 + 2 * 10080) == LDS_CAP                    # 10080 stack rows are the last that fit
    assert lib.vitvs_op_pose_rig_plan(8, 100000, 0, out) == 0 and out[0] == 2560      # the plain form takes any size
    for bad in ((0, 24, 0), (2, 0, 0), (2, 24, -1), (2, 24, 17)):
        assert lib.vitvs_op_pose_rig_plan(*bad, out) == -2, bad
    assert lib.vitvs_op_pose_rig_plan(2, 24, 0, None) == -1
    assert lib.vitvs_op_pose_rig_scratch_bytes(3, 24) == 8 * 7 * 3 * 24
    assert lib.vitvs_op_pose_rig_scratch_bytes(0, 24) == -2 and lib.vitvs_op_pose_rig_scratch_bytes(3, 0) == -2
    # the refusals of the op that need no device: null pointers and arguments out of range come before any launch
    assert lib.vitvs_op_pose_rig_law(2, 24, None, None, None, None, None, 1.0, 0, 0.0, None, None, None, None, None, None, None,
                                     None, None) == -1
