"""The consensus start of the pose law on the CPU ("The consensus start"): what tests/pose_consensus_ref.py buys with
wrong matches, its three-point solve and its fallback, the Python arguments refused before any device call, the new symbols,
the launch plan, and the margins of every case tests/test_gpu_pose_consensus_op.py runs.  No GPU call.

The bars of the wrong-match table are the issue's; the figures measured with the reference as committed are printed by the tests and
quoted in §5f."""
import ctypes as C
import functools
import types

import numpy as np
import pytest

import pose_consensus_cases as cc
import pose_consensus_ref as cr
import pose_ref as pr
import vitvs_amd  # noqa: F401
from vitvs_amd import _lib, config

LDS_CAP = 160 * 1024
_PARAMS = config.ServoParams()
PITCH_U, PITCH_V = 14 * _PARAMS.u_max / 308, 14 * _PARAMS.v_max / 308      # dinov2_vits14 at 308: the default configuration


def _outlier_case(seed, n_bad, rows=24):
    """tests/test_pose_host.py's generator with the count of wrong rows (and the row count) a parameter."""
    rng = np.random.default_rng(7000 + seed)
    R, t = pr.rodrigues(pr.unit(rng.standard_normal(3)) * rng.uniform(0.05, 0.6)), rng.uniform(-0.08, 0.08, 3)
    Z = rng.uniform(0.5, 0.8, rows)
    Q = np.stack([rng.uniform(-0.4, 0.4, rows) * Z, rng.uniform(-0.3, 0.3, rows) * Z, Z], 1)
    P = pr.points_in_camera(Q, R, t) + rng.standard_normal((rows, 3)) * 0.002
    bad = rng.choice(rows, n_bad, replace=False)
    if n_bad:
        P[bad] += np.stack([pr.unit(d) for d in rng.standard_normal((n_bad, 3))]) * rng.uniform(0.1, 0.4, (n_bad, 1))
    smin = 0.5 * max(PITCH_U / _PARAMS.f_x, PITCH_V / _PARAMS.f_y) * pr.median_middle(Q[:, 2])
    return P, Q, bad, R, t, smin


@functools.lru_cache(maxsize=None)
def _table_row(n_bad, rows, n_iter, n_hyp):
    """64 seeds -> (translation misses [64], cases with the final weights right, cases whose start weights are 0 on every wrong row)."""
    miss, right, start_ok = [], 0, 0
    for seed in range(64):
        P, Q, bad, R, t, smin = _outlier_case(seed, n_bad, rows)
        out = cr.pose_consensus_law(P, Q, np.ones(rows), 1.0, n_iter, smin, n_hyp, 0)
        good = np.setdiff1d(np.arange(rows), bad)
        miss.append(float(np.linalg.norm(out["t"] - t)) if out["status"] == pr.OK else np.inf)
        right += bool(out["status"] == pr.OK and (out["weights"][bad] == 0.0).all() and (out["weights"][good] > 0.0).all())
        start_ok += bool((out["start"][bad] == 0.0).all())
    return np.array(miss), right, start_ok


def _say(what, row):
    miss, right, start_ok = row
    print(f"{what}: translation miss median {np.median(miss):.4f} max {miss.max():.4f} m; final weights right in {right} of 64; start "
          f"weights 0 on every wrong row in {start_ok} of 64")


# ---------------------------------------------------------------------------------------------- what the start buys
def test_ten_wrong_matches_among_24():
    """M = 256, seed 0, N = 4 against N = 4 alone, 64 seeds."""
    alone, start = _table_row(10, 24, 4, 0), _table_row(10, 24, 4, 256)
    _say("10 of 24 wrong, N = 4 alone", alone)
    _say("10 of 24 wrong, consensus 256 + N = 4", start)
    assert start[0].max() <= 0.02 and start[1] >= 60 and start[2] >= 60
    assert alone[1] < start[1]


def test_fourteen_wrong_matches_among_24_without_re_weighting():
    """M = 256, seed 0, N = 0: the alignment of the consensus set alone.  The N = 4 figures at 12 and 14 wrong are printed, not
    asserted: they are the limit the docs state (the re-weightings' MAD scale is a median over all usable rows)."""
    start = _table_row(14, 24, 0, 256)
    _say("14 of 24 wrong, consensus 256, N = 0", start)
    assert np.median(start[0]) <= 0.01 and start[2] >= 58
    for n_bad in (12, 14):
        _say(f"{n_bad} of 24 wrong, N = 4 alone", _table_row(n_bad, 24, 4, 0))
        _say(f"{n_bad} of 24 wrong, consensus 256 + N = 4", _table_row(n_bad, 24, 4, 256))
    _say("12 of 24 wrong, consensus 256, N = 0", _table_row(12, 24, 0, 256))
    _say("24 of 48 wrong, consensus 256, N = 0", _table_row(24, 48, 0, 256))
    _say("24 of 48 wrong, consensus 256 + N = 4", _table_row(24, 48, 4, 256))
    _say("6 of 24 wrong, consensus 256 + N = 4", _table_row(6, 24, 4, 256))


def test_without_wrong_matches_the_start_is_todays():
    """0 of 24 wrong: every start weight is 1 in 64 of 64 cases and the whole result is pose_ref.pose_law's bit for bit."""
    for seed in range(64):
        P, Q, _, _, _, smin = _outlier_case(seed, 0)
        a = pr.pose_law(P, Q, np.ones(24), 1.0, 4, smin)
        b = cr.pose_consensus_law(P, Q, np.ones(24), 1.0, 4, smin, 256, 0)
        assert (b["start"] == 1.0).all() and b["info"][6] >= 1 and b["info"][7] == 24, seed
        for key in ("v", "R", "t", "weights", "sigma", "status"):
            assert np.array_equal(a[key], b[key]), (seed, key)
        assert np.array_equal(a["info"][:6], b["info"][:6]), seed


def test_no_hypotheses_is_the_law_itself():
    P, Q, _, _, _, smin = _outlier_case(0, 6)
    for n_iter in (0, 4):
        a = pr.pose_law(P, Q, np.ones(24), 1.0, n_iter, smin)
        b = cr.pose_consensus_law(P, Q, np.ones(24), 1.0, n_iter, smin, 0, 5)
        assert all(np.array_equal(a[k], b[k]) for k in ("v", "R", "t", "weights", "sigma", "status", "info"))


# ---------------------------------------------------------------------------------------------- the three-point solve
def test_exact_recovery_from_three_points():
    """64 seeded poses at rotation angles up to pi - 1e-3, 3 exact points: R and t to 1e-12, det R = 1."""
    worst = 0.0
    for seed in range(64):
        rng = np.random.default_rng(seed)
        angle = (0.1, 1.0, 3.0, np.pi - 1e-3)[seed % 4]
        R, t = pr.rodrigues(pr.unit(rng.standard_normal(3)) * angle), rng.uniform(-0.1, 0.1, 3)
        Q = np.array([[-0.2, -0.15, 0.55], [0.22, -0.1, 0.7], [0.05, 0.2, 0.6]]) + rng.uniform(-0.03, 0.03, (3, 3))
        Rh, th, ok = cr.three_point(pr.points_in_camera(Q, R, t), Q)
        assert ok and abs(np.linalg.det(Rh) - 1.0) < 1e-12, seed
        worst = max(worst, float(np.abs(Rh - R).max()), float(np.abs(th - t).max()))
    print(f"three-point solve: worst |R|, |t| miss {worst:.2e}")
    assert worst <= 1e-12


def test_collinear_and_coincident_points_are_skipped():
    R, t = pr.rodrigues(pr.unit([0.2, 0.5, -0.3]) * 0.5), np.array([0.03, -0.02, 0.04])
    line = np.outer(np.array([-0.3, 0.05, 0.3]), pr.unit([1.0, -1.0, 0.2])) + np.array([0.0, 0.0, 0.6])
    assert not cr.three_point(pr.points_in_camera(line, R, t), line)[2]
    Q = np.array([[-0.2, -0.15, 0.55], [0.22, -0.1, 0.7], [0.05, 0.2, 0.6]])
    P = pr.points_in_camera(Q, R, t)
    assert cr.three_point(P, Q)[2]
    assert not cr.three_point(pr.points_in_camera(line, R, t), Q)[2]     # the current points alone on a line
    assert not cr.three_point(P, line)[2]                                # the goal points alone
    for a, b in ((0, 1), (0, 2), (1, 2)):                                # two points in one place, in either cloud
        twice = P.copy()
        twice[b] = twice[a]
        assert not cr.three_point(twice, Q)[2] and not cr.three_point(Q, twice)[2], (a, b)
    assert not cr.three_point(np.zeros((3, 3)), Q)[2]                    # all in one place: 0 / 0, not finite


def test_all_hypotheses_skipped_falls_back_to_the_start_without_consensus():
    P, Q = cc.collinear(24)
    for n_iter in (0, 4):
        out = cr.pose_consensus_law(P, Q, np.ones(24), 1.0, n_iter, cc.SMIN, 256, 0)
        plain = pr.pose_law(P, Q, np.ones(24), 1.0, n_iter, cc.SMIN)
        assert out["info"][6] == 0 and out["info"][7] == 24 and (out["start"] == 1.0).all()
        assert out["status"] == plain["status"] == pr.TOO_FEW and np.array_equal(out["info"][:6], plain["info"][:6])
    # a line and two points off it: the hypotheses with three of the line are skipped, the others are not
    off = np.array([[0.2, 0.25, 0.7], [-0.2, -0.15, 0.5]])
    R, t = pr.rodrigues(pr.unit([0.2, 0.5, -0.3]) * 0.5), np.array([0.03, -0.02, 0.04])
    P2, Q2 = np.concatenate([P[:6], pr.points_in_camera(off, R, t)]), np.concatenate([Q[:6], off])
    con = cr.consensus(P2, Q2, np.ones(8), cc.SMIN, 256, 0)
    assert np.isinf(con["costs"]).any() and np.isfinite(con["costs"]).any() and con["winner"] >= 1 and con["n_start"] == 8


def test_fewer_than_three_usable_rows():
    P, Q, _, _, _, smin = _outlier_case(1, 0)
    usable = np.zeros(24, np.int32)
    usable[[3, 9]] = 1
    usable[5] = -1
    out = cr.pose_consensus_law(P, Q, usable, 1.0, 4, smin, 256, 0)
    assert out["status"] == pr.TOO_FEW and list(out["info"]) == [2, 0, 0, 0, 0, 1, 0, 0]


def test_a_consensus_set_below_three_rows_is_too_few():
    """Three usable rows whose triangles are not congruent (one current point is 0.25 m off): the only row set wins, but its fit
    leaves the moved row outside the cut-off: a consensus set of 2."""
    P, Q, _, _, _, _ = _outlier_case(2, 0, rows=3)
    P[2] += pr.unit([0.3, 0.2, -0.3]) * 0.25
    con = cr.consensus(P, Q, np.ones(3), cc.SMIN, 16, 0)
    assert con["winner"] == 1 and con["n_start"] == 2                     # (a condition on the inputs)
    for n_iter in (0, 4):
        out = cr.pose_consensus_law(P, Q, np.ones(3), 1.0, n_iter, cc.SMIN, 16, 0)
        assert out["status"] == pr.TOO_FEW and list(out["info"]) == [3, 0, 0, 1, 0, 0, 1, 2]
        assert np.array_equal(out["v"], np.zeros(6)) and np.array_equal(out["R"], np.eye(3))
        assert pr.pose_law(P, Q, np.ones(3), 1.0, n_iter, cc.SMIN)["status"] == pr.OK       # without the start all three align


# ---------------------------------------------------------------------------------------------- the host side of the library
def test_servo_params_validation():
    p = config.ServoParams()
    assert p.pose_consensus == 0 and p.pose_consensus_seed == 0
    q = config.ServoParams(law="pose", pose_consensus=4096, pose_consensus_seed=0xFFFFFFFF)
    assert q.pose_consensus == 4096 and q.pose_consensus_seed == 0xFFFFFFFF
    for bad in (-1, 4097):
        with pytest.raises(ValueError, match="pose_consensus"):
            config.ServoParams(pose_consensus=bad)
    for bad in (-1, 1 << 32):
        with pytest.raises(ValueError, match="pose_consensus_seed"):
            config.ServoParams(pose_consensus_seed=bad)
    cfg = {k: 1 for k in config._REQUIRED_KEYS}
    cfg["image_path"] = "goal.png"
    got = config.load_reference_config(cfg)
    assert got.servo.pose_consensus == 0 and got.servo.pose_consensus_seed == 0
    cfg.update(law="pose", pose_consensus=256, pose_consensus_seed=9)
    got = config.load_reference_config(cfg)
    assert got.servo.pose_consensus == 256 and got.servo.pose_consensus_seed == 9
    assert not {"pose_consensus", "pose_consensus_seed"} & set(got.extras)
    cfg.update(pose_consensus=5000)
    with pytest.raises(ValueError):
        config.load_reference_config(cfg)


def test_engine_checks_its_arguments_before_the_device():
    from vitvs_amd.engine import Engine
    eng = Engine.__new__(Engine)                               # no handle, no device: the checks come first
    K = (600.0, 600.0, 320.0, 240.0)
    for call in (eng.pose_velocity, eng.pose_velocity_host):
        for bad in (-1, 4097):
            with pytest.raises(ValueError, match="0 .. 4096"):
                call(K, np.zeros(1, np.int32), consensus=bad)
        for bad in (-1, 1 << 32):
            with pytest.raises(ValueError, match="seed"):
                call(K, np.zeros(1, np.int32), consensus=256, seed=bad)
        with pytest.raises(ValueError, match="0 .. 16"):
            call(K, np.zeros(1, np.int32), robust_iterations=17, consensus=256)
    assert Engine.POSE_INFO_FIELDS == ("usable", "sweeps", "reweighted", "zero_weights", "degenerate", "holes")


def test_the_controller_passes_the_consensus_parameters():
    from vitvs_amd import servo
    pose = config.ServoParams(law="pose", pose_robust_iterations=4, pose_consensus=256, pose_consensus_seed=3)
    seen = []

    def law(K, status, robust_iterations, consensus, seed):
        seen.append((robust_iterations, consensus, seed))
        return np.ones((1, 6)), dict(status=np.zeros(1, np.int32), R=np.eye(3)[None], t=np.zeros((1, 3)))
    eng = types.SimpleNamespace(params=pose, cfg=types.SimpleNamespace(img_size=224), apply_law_params=lambda p: None, max_pairs=4,
                                set_goal_depth=lambda z: None, pose_velocity_host=law)
    ctl = servo.Controller(eng, goal_image=None, params=pose, goal_depth=np.zeros((480, 640), np.uint16))
    ctl._pose_step(_lib.STATUS_OK)
    assert seen == [(4, 256, 3)] and ctl.last_pose_status == 0
    # behind the roll search the update ends in the same bookkeeping, and so in the same pose step
    rolled = servo.Controller(eng, goal_image=None, params=pose.replace(roll_search=True), selection="order",
                              goal_depth=np.zeros((480, 640), np.uint16))
    assert rolled._absorb(np.zeros(6), _lib.STATUS_OK) and seen[-1] == (4, 256, 3) and len(seen) == 2


def test_the_new_symbols_load():
    lib = _lib.load()
    for name in ("vitvs_pose_consensus_velocity_dev", "vitvs_pose_consensus_velocity", "vitvs_op_pose_consensus_law",
                 "vitvs_op_pose_consensus_plan"):
        assert name in _lib.PROTOTYPES and getattr(lib, name) is not None, name
    assert _lib.ABI_VERSION == 2 and lib.vitvs_abi_version() == 2           # no ABI version change


def _plan(max_rows, n_iter, n_hyp):
    """dynamic LDS in doubles: the law's 320, rho and w [max_rows] for the robust form, rho alone for the plain form with hypotheses
    (the median of Z* behind the cut-off); with hypotheses 4 cost cells and 4 + 4 ints (8 doubles) and the usable rows as ints,
    rounded up to whole doubles"""
    per_row = 2 * max_rows if n_iter > 0 else (max_rows if n_hyp > 0 else 0)
    lds = 8 * (320 + per_row + (8 + (max_rows + 1) // 2 if n_hyp > 0 else 0))
    return lds, int(n_iter > 0), int(lds > 64 * 1024), int(n_hyp > 0)


def _call(max_rows, n_iter, n_hyp):
    out = (C.c_int32 * 4)(-1, -1, -1, -1)
    return _lib.load().vitvs_op_pose_consensus_plan(max_rows, n_iter, n_hyp, out), tuple(out)


@pytest.mark.parametrize("shape", [(1, 0, 1), (24, 0, 256), (24, 4, 256), (25, 4, 1), (3136, 0, 256), (3136, 16, 4096), (3136, 4, 0),
                                   (24, 0, 0), (100000, 0, 0)])
def test_plan_equals_its_formula(shape):
    rc, out = _call(*shape)
    assert rc == 0 and out == _plan(*shape), (shape, rc, out)
    if shape[2] == 0:                                          # without hypotheses: the law's own plan
        old = (C.c_int32 * 3)()
        assert _lib.load().vitvs_op_pose_plan(shape[0], shape[1], old) == 0 and tuple(old) == out[:3]


def test_plan_on_both_sides_of_64_and_160_kib():
    assert _plan(3136, 4, 256)[0] == 65344 and _call(3136, 4, 256) == (0, (65344, 1, 0, 1))     # 3136 rows fit below the opt-in
    for n_iter, per_row in ((4, 2.5), (0, 1.5)):
        for cap in (64 * 1024, LDS_CAP):
            guess = int((cap // 8 - 328) / per_row)
            most = max(r for r in range(guess - 3, guess + 4) if _plan(r, n_iter, 256)[0] <= cap)
            assert _plan(most, n_iter, 256)[0] <= cap < _plan(most + 1, n_iter, 256)[0]
            for rows in (most, most + 1):
                rc, out = _call(rows, n_iter, 256)
                over = _plan(rows, n_iter, 256)[0] > LDS_CAP
                assert rc == (-3 if over else 0) and out == _plan(rows, n_iter, 256), (rows, rc, out)
                assert out[2] == int(out[0] > 64 * 1024)


def test_plan_refuses_bad_arguments():
    for max_rows, n_iter, n_hyp in ((0, 0, 256), (-3, 4, 256), (24, -1, 256), (24, 17, 256), (24, 4, -1), (24, 4, 4097)):
        rc, out = _call(max_rows, n_iter, n_hyp)
        assert rc == -2 and out == (0, 0, 0, 0), (max_rows, n_iter, n_hyp)
    assert _lib.load().vitvs_op_pose_consensus_plan(24, 4, 256, None) == -1


# ---------------------------------------------------------------------------------------------- the GPU test's cases
@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_the_gpu_cases_keep_their_margins(name):
    """Every (case, hypotheses, N) tests/test_gpu_pose_consensus_op.py runs: the winner's cost >= 1e-6 (relative) below the best of
    another row set, no residual within 1e-6 of the cut-off T or of a re-weighting's rejection edge, every solve's relative eigen-gap
    >= 1e-6 (degenerate cases: or <= 1e-10), as tests/test_gpu_pose_op.py asks of the law's own cases."""
    degenerate = cc.CASES[name]["degenerate"]
    for n_hyp in cc.N_HYPS:
        for n_iter in cc.N_ITERS:
            for b, ref in enumerate(cc.reference(name, n_hyp, n_iter)):
                what = (name, n_hyp, n_iter, b)
                assert ref["cgap"] >= 1e-6 and ref["edge_T"] >= 1e-6 and ref["edge"] >= 1e-6, (what, ref["cgap"], ref["edge_T"], ref["edge"])
                assert all(g >= 1e-6 or (degenerate and g <= 1e-10) for g in ref["gaps"]), (what, ref["gaps"])
                if not degenerate and n_hyp >= 64:
                    assert ref["status"] == pr.OK and ref["info"][2] == n_iter, what
    last = cc.reference(name, 512, 4)
    if name == "1x24_two_usable":
        assert all(list(cc.reference(name, m, n)[0]["info"]) == [2, 0, 0, 0, 0, 11, 0, 0] for m in cc.N_HYPS for n in cc.N_ITERS)
    elif name == "1x24_collinear":
        assert all(list(cc.reference(name, m, n)[0]["info"][4:]) == [1, 0, 0, 24] for m in cc.N_HYPS for n in cc.N_ITERS)
    elif name == "3x24":
        assert [int(r["info"][0]) for r in last] == [19, 20, 21]                             # odd and even usable counts
        assert [int(r["info"][7]) for r in last] == [11, 14, 21]                             # 8, 6 and no wrong matches left out
        assert [int(r["info"][5]) for r in last] == [2, 2, 1]                                # holes among the unusable rows
        assert len({int(r["info"][6]) for r in last}) == 3                                   # other usable counts, other draws
    elif name == "3x300":
        assert [int(r["info"][0]) for r in last] == [297, 259, 289] and [int(r["info"][7]) for r in last] == [177, 179, 289]
    elif name == "1x257":
        assert int(last[0]["info"][0]) == 248 and int(last[0]["info"][7]) == 148
    elif name == "1x3":
        assert all(cc.reference(name, m, 0)[0]["info"][6] == 1 for m in cc.N_HYPS)           # one row set: ties go to j = 0
    if not degenerate:
        winners = {m: [int(r["info"][6]) for r in cc.reference(name, m, 0)] for m in cc.N_HYPS}
        assert all(1 <= w <= m for m, ws in winners.items() for w in ws)


def test_some_gpu_case_is_won_in_the_second_round_of_the_workgroup():
    winners = [int(r["info"][6]) for name in ("3x24", "3x300", "1x257", "1x48") for r in cc.reference(name, 512, 0)]
    assert any(w > 256 for w in winners), winners
