"""The consensus start of the homography law on the CPU: what tests/homography_consensus_ref.py buys with wrong
matches, its four-point solve and its fallback, the Python arguments refused before any device call, the new symbols, the
launch plan, and the margins of every case tests/test_gpu_homography_consensus_op.py runs.  No GPU call.

The bars of the wrong-match table are the issue's; the figures measured with the reference as committed are printed by the test and
quoted in §5h."""
import ctypes as C

import numpy as np
import pytest

import homography_consensus_cases as cc
import homography_consensus_ref as cr
import homography_ref as hr
import vitvs_amd  # noqa: F401
from vitvs_amd import _lib, config

LDS_CAP = 160 * 1024
_PARAMS = config.ServoParams()
_PITCH = 14 * _PARAMS.u_max / _PARAMS.dino_input_size, 14 * _PARAMS.v_max / _PARAMS.dino_input_size   # dinov2_vits14 at 308
SIGMA_MIN = 0.5 * max(_PITCH[0] / _PARAMS.f_x, _PITCH[1] / _PARAMS.f_y)                            # the default configuration's


def _wrong_matches(s, n=24, n_out=3):
    """tests/test_homography_host.py's generator: seed 100 + s, n points uniform in +-0.3 m on the plane, rotation vector N(0,
    0.1^2), t ~ N(0, 0.04^2), 2 px Gaussian noise on the current points, the first n_out current points moved by +-U(0.1, 0.4) per
    axis."""
    rng = np.random.default_rng(100 + s)
    X = np.concatenate([rng.uniform(-0.3, 0.3, (n, 2)), np.full((n, 1), 0.61)], 1)
    R, t = hr.rodrigues(rng.normal(0.0, 0.1, 3)), rng.normal(0.0, 0.04, 3)
    clean, ms = hr.project(X, R, t), X[:, :2] / 0.61
    m = clean + rng.normal(0.0, 2.0, (n, 2)) / _PARAMS.f_x
    m[:n_out] += rng.uniform(0.1, 0.4, (n_out, 2)) * rng.choice([-1.0, 1.0], (n_out, 2))
    return clean, m, ms


# ---------------------------------------------------------------------------------------------- what the start buys
def test_eight_wrong_matches_among_24():
    """M = 256, seed 0, N = 4 against N = 4 alone, 64 seeds: the median relative twist error <= 0.1, the start weights 0 on all 8
    wrong rows in >= 60 cases, the final weights right (the 8 at 0, every inlier above 0) in >= 60, the error below half of the
    IRLS-only error in >= 50."""
    u = np.ones(24)
    irls, cons, start_ok, final_ok, irls_ok, halved = [], [], 0, 0, 0, 0
    for s in range(64):
        clean, m, ms = _wrong_matches(s, 24, 8)
        v0 = hr.homography_law(clean, ms, u, 1.0, 0.61)["v"]
        err = lambda r: float(np.linalg.norm(r["v"] - v0) / np.linalg.norm(v0))   # noqa: E731
        a = hr.homography_law(m, ms, u, 1.0, 0.61, 4, SIGMA_MIN)
        b = cr.homography_consensus_law(m, ms, u, 1.0, 0.61, 4, SIGMA_MIN, 256, 0)
        irls.append(err(a))
        cons.append(err(b))
        right = lambda r: bool(r["status"] == hr.OK and (r["weights"][:8] == 0.0).all() and (r["weights"][8:] > 0.0).all())   # noqa: E731
        start_ok += bool((b["start"][:8] == 0.0).all())
        final_ok += right(b)
        irls_ok += right(a)
        halved += cons[-1] < 0.5 * irls[-1]
    print(f"8 of 24 wrong: median twist error N = 4 alone {np.median(irls):.3f} (final weights right in {irls_ok} of 64), consensus 256 + "
          f"N = 4 {np.median(cons):.3f}; start weights 0 on all wrong rows in {start_ok}, final weights right in {final_ok}, below half "
          f"of the IRLS-only error in {halved} of 64")
    assert np.median(cons) <= 0.1 and start_ok >= 60 and final_ok >= 60 and halved >= 50


def test_without_wrong_matches_the_start_is_todays():
    """0 of 24 wrong: every start weight is 1 in 64 of 64 cases and the whole result is homography_ref.homography_law's bit for bit."""
    u = np.ones(24)
    for s in range(64):
        _, m, ms = _wrong_matches(s, 24, 0)
        a = hr.homography_law(m, ms, u, 1.0, 0.61, 4, SIGMA_MIN)
        b = cr.homography_consensus_law(m, ms, u, 1.0, 0.61, 4, SIGMA_MIN, 256, 0)
        assert (b["start"] == 1.0).all() and b["info"][6] >= 1 and b["info"][7] == 24, s
        for key in ("v", "H", "weights", "sigma", "status"):
            assert np.array_equal(a[key], b[key]), (s, key)
        assert np.array_equal(a["info"][:6], b["info"][:6]), s


def test_no_hypotheses_is_the_law_itself():
    _, m, ms = _wrong_matches(0, 24, 3)
    for n_iter in (0, 4):
        a = hr.homography_law(m, ms, np.ones(24), 1.0, 0.61, n_iter, SIGMA_MIN)
        b = cr.homography_consensus_law(m, ms, np.ones(24), 1.0, 0.61, n_iter, SIGMA_MIN, 0, 5)
        assert all(np.array_equal(a[k], b[k]) for k in ("v", "H", "weights", "sigma", "status", "info"))


# ---------------------------------------------------------------------------------------------- the four-point solve
def test_exact_recovery_from_four_points():
    """64 seeded poses, 4 points of the plane z = 0.61: H against R + t n^T / d after the det-1 scaling."""
    worst = 0.0
    for seed in range(64):
        rng = np.random.default_rng(seed)
        R, t = hr.rodrigues(rng.normal(0.0, 0.3, 3)), rng.normal(0.0, 0.05, 3)
        X = np.array([[-0.3, -0.25, 0.61], [0.28, -0.3, 0.61], [0.3, 0.27, 0.61], [-0.26, 0.3, 0.61]]) + \
            np.concatenate([rng.uniform(-0.04, 0.04, (4, 2)), np.zeros((4, 1))], 1)
        H, ok = cr.four_point(hr.project(X, R, t), X[:, :2] / 0.61)
        assert ok and np.linalg.det(H) > 0.0, seed
        worst = max(worst, float(np.abs(H / np.cbrt(np.linalg.det(H)) - hr.true_homography(R, t)).max()))
    print(f"four-point solve: worst |H - H_true| {worst:.2e}")
    assert worst <= 1e-11


def test_collinear_points_are_skipped():
    R, t = hr.rodrigues([0.1, 0.2, -0.1]), np.array([0.02, 0.01, 0.03])
    on_line = lambda s: np.stack([s, 0.1 + 0.5 * s, np.full(len(s), 0.61)], 1)   # noqa: E731
    off = np.array([[0.2, -0.2, 0.61]])
    for where in range(4):                                      # three of one line and one off it, the odd one at every place
        X = np.insert(on_line(np.array([-0.3, 0.05, 0.3])), where, off, 0)
        assert not cr.four_point(hr.project(X, R, t), X[:, :2] / 0.61)[1], where
    X = on_line(np.array([-0.3, -0.1, 0.12, 0.3]))               # all four of one line
    assert not cr.four_point(hr.project(X, R, t), X[:, :2] / 0.61)[1]
    X = np.array([[-0.3, -0.3, 0.61], [0.3, -0.3, 0.61], [0.3, 0.3, 0.61], [-0.3, 0.3, 0.61]])
    assert cr.four_point(hr.project(X, R, t), X[:, :2] / 0.61)[1]
    wrong = hr.project(X, R, t)
    wrong[2] = wrong[0]                                          # two current points in one place
    assert not cr.four_point(wrong, X[:, :2] / 0.61)[1]


def test_all_hypotheses_skipped_falls_back_to_the_start_without_consensus():
    m, ms = cc.collinear(24)
    for n_iter in (0, 4):
        out = cr.homography_consensus_law(m, ms, np.ones(24), 1.0, 0.61, n_iter, SIGMA_MIN, 256, 0)
        plain = hr.homography_law(m, ms, np.ones(24), 1.0, 0.61, n_iter, SIGMA_MIN)
        assert out["info"][6] == 0 and out["info"][7] == 24 and (out["start"] == 1.0).all()
        assert out["status"] == plain["status"] == hr.TOO_FEW and np.array_equal(out["info"][:6], plain["info"][:6])
    # a line and two points off it: the hypotheses with three of the line are skipped, the others are not
    m2, ms2 = np.concatenate([m[:6], [[0.2, 0.25], [-0.2, -0.15]]]), np.concatenate([ms[:6], [[0.21, 0.24], [-0.22, -0.13]]])
    con = cr.consensus(m2, ms2, np.ones(8), SIGMA_MIN, 256, 0)
    assert np.isinf(con["costs"]).any() and np.isfinite(con["costs"]).any() and con["winner"] >= 1


def test_fewer_than_four_usable_rows():
    _, m, ms = _wrong_matches(1, 8, 0)
    out = cr.homography_consensus_law(m, ms, [1, 1, 1, 0, 0, 0, 0, 0], 1.0, 1.0, 4, SIGMA_MIN, 256, 0)
    assert out["status"] == hr.TOO_FEW and list(out["info"]) == [3, 0, 0, 0, 0, 0, 0, 0]


# ---------------------------------------------------------------------------------------------- the host side of the library
def test_servo_params_validation():
    p = config.ServoParams()
    assert p.homography_consensus == 0 and p.homography_consensus_seed == 0
    q = config.ServoParams(law="homography", homography_consensus=4096, homography_consensus_seed=0xFFFFFFFF)
    assert q.homography_consensus == 4096 and q.homography_consensus_seed == 0xFFFFFFFF
    for bad in (-1, 4097):
        with pytest.raises(ValueError, match="homography_consensus"):
            config.ServoParams(homography_consensus=bad)
    for bad in (-1, 1 << 32):
        with pytest.raises(ValueError, match="homography_consensus_seed"):
            config.ServoParams(homography_consensus_seed=bad)
    cfg = {k: 1 for k in config._REQUIRED_KEYS}
    cfg["image_path"] = "goal.png"
    got = config.load_reference_config(cfg)
    assert got.servo.homography_consensus == 0 and got.servo.homography_consensus_seed == 0
    cfg.update(law="homography", homography_consensus=256, homography_consensus_seed=9)
    got = config.load_reference_config(cfg)
    assert got.servo.homography_consensus == 256 and got.servo.homography_consensus_seed == 9
    assert not {"homography_consensus", "homography_consensus_seed"} & set(got.extras)
    cfg.update(homography_consensus=5000)
    with pytest.raises(ValueError):
        config.load_reference_config(cfg)


def test_engine_checks_its_arguments_before_the_device():
    from vitvs_amd.engine import Engine
    eng = Engine.__new__(Engine)                               # no handle, no device: the checks come first
    K = (600.0, 600.0, 320.0, 240.0)
    for call in (eng.homography_velocity, eng.homography_velocity_host):
        for bad in (-1, 4097):
            with pytest.raises(ValueError, match="0 .. 4096"):
                call(K, np.zeros(1, np.int32), consensus=bad)
        for bad in (-1, 1 << 32):
            with pytest.raises(ValueError, match="seed"):
                call(K, np.zeros(1, np.int32), consensus=256, seed=bad)
        with pytest.raises(ValueError, match="0 .. 16"):
            call(K, np.zeros(1, np.int32), robust_iterations=17, consensus=256)


def test_the_controller_passes_the_consensus_parameters():
    import types
    from vitvs_amd import servo
    hom = config.ServoParams(law="homography", homography_depth=0.61, homography_robust_iterations=4, homography_consensus=256,
                             homography_consensus_seed=3)
    seen = []

    def law(K, status, depth_scale, robust_iterations, consensus, seed):
        seen.append((depth_scale, robust_iterations, consensus, seed))
        return np.ones((1, 6)), dict(status=np.zeros(1, np.int32), H=np.eye(3)[None])
    eng = types.SimpleNamespace(params=hom, cfg=types.SimpleNamespace(img_size=224), apply_law_params=lambda p: None, max_pairs=4,
                                set_goal_depth=lambda z: None, homography_velocity_host=law)
    ctl = servo.Controller(eng, goal_image=None, params=hom)
    ctl._homography_step(_lib.STATUS_OK)
    assert seen == [(0.61, 4, 256, 3)] and ctl.last_homography_status == 0


def test_the_new_symbols_load():
    lib = _lib.load()
    for name in ("vitvs_homography_consensus_velocity_dev", "vitvs_homography_consensus_velocity", "vitvs_op_homography_consensus_law",
                 "vitvs_op_homography_consensus_plan"):
        assert name in _lib.PROTOTYPES and getattr(lib, name) is not None, name


def _plan(max_rows, n_iter, n_hyp):
    """dynamic LDS in doubles: the law's 752, rho and w [max_rows] for the robust form; with hypotheses 4 cost cells and 4 + 4 ints (8
    doubles) and the usable rows as ints, rounded up to whole doubles"""
    lds = 8 * (752 + (2 * max_rows if n_iter > 0 else 0) + (8 + (max_rows + 1) // 2 if n_hyp > 0 else 0))
    return lds, int(n_iter > 0), int(lds > 64 * 1024), int(n_hyp > 0)


def _call(max_rows, n_iter, n_hyp):
    out = (C.c_int32 * 4)(-1, -1, -1, -1)
    return _lib.load().vitvs_op_homography_consensus_plan(max_rows, n_iter, n_hyp, out), tuple(out)


@pytest.mark.parametrize("shape", [(1, 0, 1), (24, 0, 256), (24, 4, 256), (25, 4, 1), (3136, 0, 256), (3136, 16, 4096), (3136, 4, 0),
                                   (24, 0, 0), (100000, 0, 0)])
def test_plan_equals_its_formula(shape):
    rc, out = _call(*shape)
    assert rc == 0 and out == _plan(*shape), (shape, rc, out)
    if shape[2] == 0:                                          # without hypotheses: the law's own plan
        old = (C.c_int32 * 3)()
        assert _lib.load().vitvs_op_homography_plan(shape[0], shape[1], old) == 0 and tuple(old) == out[:3]


def test_plan_on_both_sides_of_64_and_160_kib():
    assert _plan(3136, 4, 256)[0] == 68800 and _call(3136, 4, 256) == (0, (68800, 1, 1, 1))    # 3136 rows fit, past the opt-in
    for cap in (64 * 1024, LDS_CAP):
        most = max(r for r in range((cap // 8 - 760) * 2 // 5 - 2, (cap // 8 - 760) * 2 // 5 + 3) if _plan(r, 4, 256)[0] <= cap)
        assert _plan(most, 4, 256)[0] <= cap < _plan(most + 1, 4, 256)[0]
        for rows in (most, most + 1):
            rc, out = _call(rows, 4, 256)
            over = _plan(rows, 4, 256)[0] > LDS_CAP
            assert rc == (-3 if over else 0) and out == _plan(rows, 4, 256), (rows, rc, out)
            assert out[2] == int(out[0] > 64 * 1024)
        most = (cap // 8 - 760) * 2                            # the plain form keeps only the usable rows' list
        assert _plan(most, 0, 256)[0] <= cap < _plan(most + 1, 0, 256)[0]
        for rows in (most, most + 1):
            rc, out = _call(rows, 0, 256)
            assert rc == (-3 if _plan(rows, 0, 256)[0] > LDS_CAP else 0) and out == _plan(rows, 0, 256), (rows, rc, out)


def test_plan_refuses_bad_arguments():
    for max_rows, n_iter, n_hyp in ((0, 0, 256), (-3, 4, 256), (24, -1, 256), (24, 17, 256), (24, 4, -1), (24, 4, 4097)):
        rc, out = _call(max_rows, n_iter, n_hyp)
        assert rc == -2 and out == (0, 0, 0, 0), (max_rows, n_iter, n_hyp)
    assert _lib.load().vitvs_op_homography_consensus_plan(24, 4, 256, None) == -1


# ---------------------------------------------------------------------------------------------- the GPU test's cases
@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_the_gpu_cases_keep_their_margins(name):
    """Every (case, hypotheses, N) tests/test_gpu_homography_consensus_op.py runs: the winner's cost >= 1e-6 (relative) below the best
    of another row set, no residual within 1e-6 of the cut-off T or of a re-weighting's rejection edge, every solve's second-smallest
    eigenvalue >= 1e-4 of the trace (degenerate cases: or <= 1e-10) and, where the status is OK, an eigen-gap >= 1e-4."""
    degenerate = cc.CASES[name]["degenerate"]
    for n_hyp in cc.N_HYPS:
        for n_iter in cc.N_ITERS:
            for b, ref in enumerate(cc.reference(name, n_hyp, n_iter)):
                what = (name, n_hyp, n_iter, b)
                assert ref["gap"] >= 1e-6 and ref["edge_T"] >= 1e-6 and ref["edge"] >= 1e-6, (what, ref["gap"], ref["edge_T"], ref["edge"])
                assert all(g >= 1e-4 or (degenerate and g <= 1e-10) for g in ref["ratios"]), (what, ref["ratios"])
                if ref["status"] == hr.OK:
                    assert min(ref["gaps"]) >= 1e-4 and ref["info"][2] == n_iter, (what, ref["gaps"])
    last = cc.reference(name, 512, 4)
    if name == "1x24_three_usable":
        assert all(list(cc.reference(name, m, n)[0]["info"]) == [3, 0, 0, 0, 0, 0, 0, 0] for m in cc.N_HYPS for n in cc.N_ITERS)
    elif name == "1x24_collinear":
        assert all(list(cc.reference(name, m, n)[0]["info"][4:]) == [1, 0, 0, 24] for m in cc.N_HYPS for n in cc.N_ITERS)
    elif name == "1x24_behind":
        for m in cc.N_HYPS[1:]:
            c = cc.CASES[name]
            con = cr.consensus(c["m"][0], c["ms"][0], c["usable"][0], cc.SMIN, m, cc.SEED)
            q = cr.transfer_sq(con["H"], c["m"][0], c["ms"][0])
            assert np.isinf(q[cc.BEHIND_ROW]) and con["start"][cc.BEHIND_ROW] == 0.0 and con["n_start"] == 23
    elif name == "3x24":
        assert [int(r["info"][0]) for r in last] == [19, 20, 21]                             # odd and even usable counts
        assert [int(r["info"][7]) for r in last] == [13, 15, 21]                             # 6, 5 and no wrong matches left out
        assert len({int(r["info"][6]) for r in last}) == 3                                   # other usable counts, other draws
    elif name == "3x300":
        assert [int(r["info"][0]) for r in last] == [297, 259, 289] and [int(r["info"][7]) for r in last] == [207, 199, 289]
    elif name == "1x4":
        assert all(cc.reference(name, m, 0)[0]["info"][6] == 1 for m in cc.N_HYPS)           # one row set: ties go to j = 0
    if not degenerate:
        winners = {m: [int(r["info"][6]) for r in cc.reference(name, m, 0)] for m in cc.N_HYPS}
        assert all(1 <= w <= m for m, ws in winners.items() for w in ws)


def test_some_gpu_case_is_won_in_the_second_round_of_the_workgroup():
    winners = [int(r["info"][6]) for name in ("3x24", "3x300", "1x257") for r in cc.reference(name, 512, 0)]
    assert any(w > 256 for w in winners), winners
