"""The homography law's fp64 statement (tests/homography_ref.py) on the CPU, and the law's host side: what the law
computes on exact points of a plane, its closed loop at small and large turns about the optical axis with a right and a wrong
depth scale, what the re-weighting buys with wrong matches, its status rules, the Python arguments refused before any device call,
the new symbols and the launch plan.  No GPU call.

Every bar below is the issue's; figures measured with the generators as committed are printed by the tests and quoted in §5h."""
import ctypes as C
import types

import numpy as np
import pytest

import homography_ref as hr
import vitvs_amd  # noqa: F401
from vitvs_amd import _lib, config

LDS_CAP = 160 * 1024
_PARAMS = config.ServoParams()
_PITCH = 14 * _PARAMS.u_max / _PARAMS.dino_input_size, 14 * _PARAMS.v_max / _PARAMS.dino_input_size   # dinov2_vits14 at 308
SIGMA_MIN = 0.5 * max(_PITCH[0] / _PARAMS.f_x, _PITCH[1] / _PARAMS.f_y)                            # the default configuration's


def test_exact_recovery_on_points_of_a_plane():
    """64 seeded poses, 4 / 8 / 24 points on z = 0.61: H against R + t n^T / d, scaled to det 1."""
    worst, smallest, sweeps = 0.0, np.inf, 0
    for seed in range(64):
        rng = np.random.default_rng(seed)
        R, t = hr.rodrigues(rng.normal(0.0, 0.3, 3)), rng.normal(0.0, 0.05, 3)
        n = (4, 8, 24)[seed % 3]
        X = np.stack([rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n), np.full(n, 0.61)], 1)
        out = hr.homography_law(hr.project(X, R, t), X[:, :2] / 0.61, np.ones(n), 1.0)
        sweeps = max(sweeps, int(out["info"][1]))
        if out["ratios"][0] >= 1e-4:
            assert out["status"] == hr.OK and abs(np.linalg.det(out["H"]) - 1.0) < 1e-12
            worst = max(worst, float(np.abs(out["H"] - hr.true_homography(R, t)).max()))
            smallest = min(smallest, out["ratios"][0])
    print(f"exact recovery: worst |H - H_true| {worst:.2e}; smallest ev_2 / trace among them {smallest:.2e}; most sweeps {sweeps}")
    assert worst <= 1e-11 and sweeps <= 32


def test_the_twist_moves_the_camera_against_its_pose_error():
    """To first order e_nu = t / Z + theta x m_c - (n . t / 3 d) m_c and e_omega = 2 theta + n x t / d: a small pose error comes
    back as -lambda (z^ e_nu, e_omega), which pins the sign of the law."""
    gx, gy = np.meshgrid(np.linspace(-0.25, 0.25, 5), np.linspace(-0.18, 0.18, 5))
    X = np.stack([gx.ravel(), gy.ravel(), np.full(25, 0.61)], 1)
    th, t = np.array([2e-4, -3e-4, 5e-4]), np.array([3e-4, -2e-4, 1e-4])
    out = hr.homography_law(hr.project(X, hr.rodrigues(th), t), X[:, :2] / 0.61, np.ones(25), 1.0, 0.61)
    n, d, mc = np.array([0.0, 0.0, 1.0]), 0.61, np.array([0.0, 0.0, 1.0])
    e_nu = t / 0.61 + np.cross(th, mc) - (n @ t / (3.0 * d)) * mc
    e_om = 2.0 * th + np.cross(n, t) / d
    assert np.abs(out["v"] - np.concatenate([-0.61 * e_nu, -e_om])).max() < 2e-6      # second-order terms: |theta|, |t| ~ 5e-4


GRID = np.stack([np.meshgrid(np.linspace(-0.25, 0.25, 5), np.linspace(-0.18, 0.18, 5))[0].ravel(),
                 np.meshgrid(np.linspace(-0.25, 0.25, 5), np.linspace(-0.18, 0.18, 5))[1].ravel(), np.full(25, 0.61)], 1)
T0 = np.array([0.04, -0.03, 0.03])


def _closed_loop(turn_deg, depth_scale, steps=400, dt=0.05):
    R = hr.rodrigues([0.0, 0.0, np.radians(turn_deg)]) @ hr.rodrigues([np.radians(3.0), 0.0, 0.0])
    t = T0.copy()
    start, tz = hr.pose_error(R, t), []
    for _ in range(steps):
        out = hr.homography_law(hr.project(GRID, R, t), GRID[:, :2] / 0.61, np.ones(25), 1.0, depth_scale)
        assert out["status"] == hr.OK
        R, t = hr.step(R, t, out["v"], dt)
        tz.append(t[2])
    return start, hr.pose_error(R, t), min(tz), max(tz)


@pytest.mark.parametrize("turn", [5.0, 45.0, 90.0, 170.0])
def test_closed_loop_on_exact_points(turn):
    """lambda = 1, dt = 0.05, 400 steps, the true distance as the depth scale: the camera arrives, and it never retreats."""
    start, end, tz_min, tz_max = _closed_loop(turn, 0.61)
    print(f"turn {turn:5.1f} deg: {start[0] * 100:.2f} cm / {start[1]:.2f} deg -> {end[0]:.2e} m / {end[1]:.2e} deg; "
          f"t_z in [{tz_min:.2e}, {tz_max:.5f}]")
    assert end[0] < 1e-4 and end[1] < 0.01
    assert -1e-6 <= tz_min and tz_max <= 0.03 + 1e-9


@pytest.mark.parametrize("depth_scale", [1.0, 0.2])
def test_a_wrong_depth_scale_changes_the_rate_not_the_fixed_point(depth_scale):
    start, end, _, _ = _closed_loop(5.0, depth_scale)
    print(f"depth scale {depth_scale}: {start[0]:.3e} m / {start[1]:.3f} deg -> {end[0]:.2e} m / {end[1]:.2e} deg")
    assert end[0] < start[0] and end[1] < start[1]


def _wrong_matches(s, n=24, n_out=3):
    """The issue's generator: seed 100 + s, n points uniform in +-0.3 m on the plane, rotation vector N(0, 0.1^2), t ~ N(0, 0.04^2),
    2 px Gaussian noise on the current points, the first n_out current points moved by +-U(0.1, 0.4) per axis."""
    rng = np.random.default_rng(100 + s)
    X = np.concatenate([rng.uniform(-0.3, 0.3, (n, 2)), np.full((n, 1), 0.61)], 1)
    R, t = hr.rodrigues(rng.normal(0.0, 0.1, 3)), rng.normal(0.0, 0.04, 3)
    clean, ms = hr.project(X, R, t), X[:, :2] / 0.61
    m = clean + rng.normal(0.0, 2.0, (n, 2)) / _PARAMS.f_x
    m[:n_out] += rng.uniform(0.1, 0.4, (n_out, 2)) * rng.choice([-1.0, 1.0], (n_out, 2))
    return clean, m, ms


def _wrong_match_counts(n, n_out, n_ratio):
    """-> (median plain error, median error with n_ratio re-weightings, cases with robust / plain < 0.5, cases in which N = 8 ends
    with every outlier at weight 0 and every inlier above 0); the twist error is relative to the noise-free twist."""
    plain, robust, ratio_ok, weights_ok = [], [], 0, 0
    u = np.ones(n)
    for s in range(64):
        clean, m, ms = _wrong_matches(s, n, n_out)
        v0 = hr.homography_law(clean, ms, u, 1.0, 0.61)["v"]
        err = lambda r: float(np.linalg.norm(r["v"] - v0) / np.linalg.norm(v0))   # noqa: E731
        p = hr.homography_law(m, ms, u, 1.0, 0.61, 0, SIGMA_MIN)
        r8 = hr.homography_law(m, ms, u, 1.0, 0.61, 8, SIGMA_MIN)
        rn = r8 if n_ratio == 8 else hr.homography_law(m, ms, u, 1.0, 0.61, n_ratio, SIGMA_MIN)
        plain.append(err(p))
        robust.append(err(rn))
        ratio_ok += robust[-1] / plain[-1] < 0.5
        weights_ok += bool(r8["status"] == hr.OK and (r8["weights"][:n_out] == 0.0).all() and (r8["weights"][n_out:] > 0.0).all())
    return float(np.median(plain)), float(np.median(robust)), int(ratio_ok), int(weights_ok)


def test_wrong_matches_are_rejected():
    """3 wrong matches among 24: N = 4 more than halves the twist error in 64 of 64 cases, N = 8 ends with the three at weight 0 and
    every inlier above 0 in 64 of 64."""
    plain, robust, ratio_ok, weights_ok = _wrong_match_counts(24, 3, 4)
    print(f"3 of 24 wrong: median twist error plain {plain:.3f}, N = 4 {robust:.3f}; robust / plain < 0.5 in {ratio_ok} of 64; "
          f"N = 8 weights right in {weights_ok} of 64")
    assert ratio_ok == 64 and weights_ok == 64


def test_six_wrong_matches_among_48():
    plain, robust, ratio_ok, weights_ok = _wrong_match_counts(48, 6, 8)
    print(f"6 of 48 wrong: median twist error plain {plain:.3f}, N = 8 {robust:.3f}; robust / plain < 0.5 in {ratio_ok} of 64; "
          f"N = 8 weights right in {weights_ok} of 64")
    assert ratio_ok == 64 and weights_ok == 64


# ---------------------------------------------------------------------------------------------- the status rules
def _exact(n, seed=3):
    rng = np.random.default_rng(seed)
    R, t = hr.rodrigues(rng.normal(0.0, 0.2, 3)), rng.normal(0.0, 0.04, 3)
    X = np.concatenate([rng.uniform(-0.3, 0.3, (n, 2)), np.full((n, 1), 0.61)], 1)
    return hr.project(X, R, t), X[:, :2] / 0.61


def test_status_too_few_rows():
    m, ms = _exact(8)
    for usable in ([1, 1, 1, 0, 0, 0, 0, 0], [0] * 8):
        out = hr.homography_law(m, ms, usable, 1.0, 1.0, 4, SIGMA_MIN)
        assert out["status"] == hr.TOO_FEW and np.array_equal(out["v"], np.zeros(6)) and np.array_equal(out["H"], np.eye(3))
        assert list(out["info"]) == [sum(usable), 0, 0, 0, 0, 0, 0, 0]
    assert hr.homography_law(m, ms, [1, 1, 1, 1, 0, 0, 0, 0], 1.0)["status"] == hr.OK


def test_status_degenerate_sets():
    s = np.linspace(-0.3, 0.3, 8)
    X = np.stack([s, 0.1 + 0.5 * s, np.full(8, 0.61)], 1)
    out = hr.homography_law(hr.project(X, hr.rodrigues([0.1, 0.2, -0.1]), np.array([0.02, 0.01, 0.03])), X[:, :2] / 0.61,
                            np.ones(8), 1.0)
    print(f"collinear points: ev_2 / trace = {out['ratios'][0]:.2e}")
    assert out["status"] == hr.TOO_FEW and out["info"][4] == 1 and abs(out["ratios"][0]) <= 1e-10
    assert np.array_equal(out["v"], np.zeros(6)) and np.array_equal(out["H"], np.eye(3))
    same = np.tile([[0.5, -0.25]], (8, 1))                                       # all points in one place: a mean distance of 0
    out = hr.homography_law(same, same, np.ones(8), 1.0)
    assert out["status"] == hr.TOO_FEW and list(out["info"][:5]) == [8, 0, 0, 0, 1]


def test_status_same_image_and_camera_statuses():
    rows = 6
    m, ms = _exact(rows)
    K = (500.0, 500.0, 320.0, 240.0)
    s_uv = np.zeros((1, rows, 4), np.int32)
    s_uv[0, :, 0], s_uv[0, :, 1] = np.round(ms[:, 0] * 500.0 + 320.0), np.round(ms[:, 1] * 500.0 + 240.0)
    feat = np.concatenate([np.full((rows, 1), 100.0), m, np.ones((rows, 1))], 1)[None]      # Z = 100: no depth anywhere
    det = dict(selected=np.arange(rows, dtype=np.int32)[None], s_uv=s_uv, feat=feat, info=np.array([[6, 6, 1, 6, 0, 12, 0, 0]], np.int32))
    for cam in (hr.OK, hr.NO_DEPTH):                                             # the same-image shortcut: OK, v = 0, H = I
        out = hr.homography_from_details(det, 0, cam, K, 1.0, 1.0, 0, *_PITCH)
        assert out["status"] == hr.OK and np.array_equal(out["v"], np.zeros(6)) and np.array_equal(out["H"], np.eye(3))
    for cam in (hr.NO_CORRESPONDENCE, hr.TOO_FEW):                               # the camera's own status, v = 0
        out = hr.homography_from_details(det, 0, cam, K, 1.0, 1.0, 0, *_PITCH)
        assert out["status"] == cam and np.array_equal(out["v"], np.zeros(6)) and np.array_equal(out["H"], np.eye(3))
    det["info"][0, 2] = 0
    ok = hr.homography_from_details(det, 0, hr.OK, K, 1.0, 1.0, 0, *_PITCH)
    no_depth = hr.homography_from_details(det, 0, hr.NO_DEPTH, K, 1.0, 1.0, 0, *_PITCH)     # NO_DEPTH does not stop this law
    assert ok["status"] == hr.OK and no_depth["status"] == hr.OK and np.array_equal(ok["v"], no_depth["v"])
    assert np.abs(ok["v"]).max() > 1e-3


def test_points_from_details():
    """Rows past info[1] and padded rows are not usable; the depth column is never read."""
    K = (500.0, 400.0, 320.0, 240.0)
    sel = np.array([3, 5, -1, 7, 9, 2], np.int32)
    s_uv = np.array([[420, 340, 0, 0], [320, 240, 0, 0], [0, 0, 0, 0], [100, 100, 0, 0], [200, 200, 0, 0], [1, 1, 0, 0]], np.int32)
    feat = np.array([[0.5, 0.1, -0.2, 1], [100.0, 0.3, 0.4, 1], [100.0, 0, 0, 0], [np.nan, 0.3, 0.1, 1], [0.6, 0, 0, 1], [0.6, 0, 0, 1]])
    m, ms, us = hr.points_from_details(sel, s_uv, feat, 5, K)
    assert list(us) == [1, 1, 0, 1, 1, 0]
    assert np.allclose(m[0], [0.1, -0.2]) and np.allclose(ms[0], [0.2, 0.25]) and np.allclose(m[1], [0.3, 0.4])


# ---------------------------------------------------------------------------------------------- the host side of the library
def test_servo_params_validation():
    p = config.ServoParams()
    assert p.law == "ibvs" and p.homography_robust_iterations == 0 and p.homography_depth == 1.0
    assert "homography" in config.LAWS
    q = config.ServoParams(law="homography", homography_robust_iterations=16, homography_depth=0.61)
    assert q.homography_robust_iterations == 16 and q.homography_depth == 0.61
    for bad in (-1, 17):
        with pytest.raises(ValueError):
            config.ServoParams(homography_robust_iterations=bad)
    for bad in (0.0, -0.5, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            config.ServoParams(homography_depth=bad)
    cfg = {k: 1 for k in config._REQUIRED_KEYS}
    cfg["image_path"] = "goal.png"
    got = config.load_reference_config(cfg)
    assert got.servo.law == "ibvs" and got.servo.homography_depth == 1.0 and got.servo.homography_robust_iterations == 0
    cfg.update(law="homography", homography_robust_iterations=4, homography_depth=0.61)
    got = config.load_reference_config(cfg)
    assert got.servo.law == "homography" and got.servo.homography_robust_iterations == 4 and got.servo.homography_depth == 0.61
    assert not {"law", "homography_robust_iterations", "homography_depth"} & set(got.extras)
    cfg.update(homography_depth=0)
    with pytest.raises(ValueError):
        config.load_reference_config(cfg)


def test_the_controllers_and_the_homography_law():
    from vitvs_amd import pipeline, servo
    hom = config.ServoParams(law="homography", homography_depth=0.61)
    eng = types.SimpleNamespace(params=hom, cfg=types.SimpleNamespace(img_size=224), apply_law_params=lambda p: None,
                                max_pairs=4, set_goal_depth=lambda z: None)
    ctl = servo.Controller(eng, goal_image=None, params=hom)                     # no goal_depth, no depth callback
    assert ctl.last_homography_status is None and ctl.last_homography is None and ctl.goal_depth is None
    ctl._raw_v = np.arange(6.0)
    ctl._law_step(True)                                                          # no depth image: the update is not skipped
    assert ctl.v_c is not None and len(ctl.velocity_vector_history) == 1
    other = servo.Controller(eng, goal_image=None, params=config.ServoParams())  # the reference's law still skips it
    other._raw_v = np.arange(6.0)
    other._law_step(True)
    assert other.v_c is None and other.velocity_vector_history == []
    with pytest.raises(ValueError, match="homography"):
        servo.MultiController(eng, [None, None], params=hom)
    with pytest.raises(ValueError, match="homography"):
        pipeline.UpdatePipeline(config.baseline_config("vits16_224"), hom, {})


def test_engine_homography_velocity_checks_its_arguments_before_the_device():
    from vitvs_amd.engine import Engine
    eng = Engine.__new__(Engine)                               # no handle, no device: the checks come first
    K = (600.0, 600.0, 320.0, 240.0)
    for call in (eng.homography_velocity, eng.homography_velocity_host):
        for bad in (-1, 17):
            with pytest.raises(ValueError, match="0 .. 16"):
                call(K, np.zeros(1, np.int32), robust_iterations=bad)
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            with pytest.raises(ValueError, match="depth_scale"):
                call(K, np.zeros(1, np.int32), depth_scale=bad)


def test_the_new_symbols_load():
    lib = _lib.load()
    for name in ("vitvs_homography_velocity_dev", "vitvs_homography_velocity", "vitvs_op_homography_law",
                 "vitvs_op_homography_scratch_bytes", "vitvs_op_homography_plan"):
        assert name in _lib.PROTOTYPES and getattr(lib, name) is not None, name
    assert _lib.ABI_VERSION == 2 and lib.vitvs_abi_version() == 2


def _plan(max_rows, n_iter):
    """dynamic LDS in doubles: 8 slices x 64 quantities | 48 sums | 8 centroids and scales | M and V, 81 each | H and m_c, 12 | 2
    middles | 8 of ints = 752; rho, w [max_rows] for the robust form"""
    lds = 8 * (8 * 64 + 48 + 8 + 81 + 81 + 12 + 2 + 8 + (2 * max_rows if n_iter > 0 else 0))
    return lds, int(n_iter > 0), int(lds > 64 * 1024)


def _call(max_rows, n_iter):
    out = (C.c_int32 * 3)(-1, -1, -1)
    return _lib.load().vitvs_op_homography_plan(max_rows, n_iter, out), tuple(out)


@pytest.mark.parametrize("shape", [(1, 0), (24, 0), (24, 4), (3136, 0), (3136, 16), (3800, 1), (4100, 1), (100000, 0)])
def test_plan_equals_its_formula(shape):
    rc, out = _call(*shape)
    assert rc == 0 and out == _plan(*shape), (shape, rc, out)


def test_plan_on_both_sides_of_160_kib():
    most = (LDS_CAP // 8 - 752) // 2
    assert _call(most, 4) == (0, _plan(most, 4)) and _plan(most, 4)[0] <= LDS_CAP
    rc, out = _call(most + 1, 4)
    assert rc == -3 and out == _plan(most + 1, 4) and out[0] > LDS_CAP
    assert _call(most + 1, 0)[0] == 0                          # the plain form keeps nothing per row in LDS


def test_plan_and_scratch_refuse_bad_arguments():
    lib = _lib.load()
    for max_rows, n_iter in ((0, 0), (-3, 4), (24, -1), (24, 17)):
        assert _call(max_rows, n_iter)[0] == -2, (max_rows, n_iter)
    assert lib.vitvs_op_homography_plan(24, 4, None) == -1
    for n, ld in ((0, 24), (1, 0), (-1, 24)):
        assert lib.vitvs_op_homography_scratch_bytes(n, ld) == -2
    for n, ld in ((1, 4), (3, 24), (1, 1100)):
        assert lib.vitvs_op_homography_scratch_bytes(n, ld) == 8 * 5 * n * ld
