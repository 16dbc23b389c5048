"""The rig law's fp64 statement (tests/rig_ref.py) on the CPU: the twist transform against a finite difference of poses, the
property that makes the law worth having (the stacked solution recovers a rig twist that the average of the cameras' own
pseudo-inverse twists misses), and its edge cases.  No GPU, no library call except ``servo.twist_matrix``."""
import numpy as np

import vitvs_amd  # noqa: F401
from vitvs_amd import servo

import rig_ref as rg


def _log_so3(R):
    th = np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0))
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / 2.0
    return w if th < 1e-12 else w * th / np.sin(th)


def test_twist_matrix_is_the_references_and_matches_a_finite_difference_of_poses():
    """planar_sim's body-twist convention: t += R v dt, R = R expm([w]x dt); camera pose = rig pose o extrinsic.  The camera's
    finite-difference body twist equals W v_r to O(dt)."""
    rng = np.random.default_rng(5)
    for _ in range(16):
        Rr, tr = rg.random_extrinsic(rng, 1.0, 1.0)                  # the rig's pose in the world
        Re, te = rg.random_extrinsic(rng, 1.0, 0.5)                  # the camera's pose in the rig frame
        v_r = rng.standard_normal(6)
        W = servo.twist_matrix(Re, te)
        assert W.dtype == np.float64 and W.shape == (6, 6)
        assert np.array_equal(W, rg.twist_matrix(Re, te))
        errs = []
        for dt in (1e-4, 1e-5):
            tr2 = tr + Rr @ v_r[:3] * dt
            Rr2 = Rr @ rg.rodrigues(v_r[3:] * dt)
            Rc, tc = Rr @ Re, Rr @ te + tr
            Rc2, tc2 = Rr2 @ Re, Rr2 @ te + tr2
            v_c = np.concatenate([Rc.T @ (tc2 - tc) / dt, _log_so3(Rc.T @ Rc2) / dt])
            errs.append(np.linalg.norm(v_c - W @ v_r) / np.linalg.norm(W @ v_r))
        assert errs[0] < 1e-3 and errs[1] < 1e-4 and errs[1] < 0.2 * errs[0], errs    # first order in dt


def test_the_stacked_law_recovers_the_rig_twist_and_the_averaged_twists_do_not():
    """64 seeded rigs of 3 cameras x 2 feature pairs with e_i = L_i W_i v*: no camera alone observes six degrees of freedom (4
    rows), the stack does.  The rig law returns v* to <= 1e-12 in all 64; the average of the cameras' own twists mapped back
    misses it by > 0.1 in all 64."""
    worst_rig, best_avg, worst_cond = 0.0, np.inf, 0.0
    for seed in range(64):
        Ls, es, Ws, v_star = rg.scenario(seed)
        ref = rg.rig_law(Ls, es, Ws, [0, 0, 0], 1.0)
        assert ref["status"] == 0 and ref["rows"] == 12 and ref["cameras"] == 3
        worst_cond = max(worst_cond, np.linalg.cond(ref["M"]))
        nv = np.linalg.norm(v_star)
        worst_rig = max(worst_rig, np.linalg.norm(-ref["v_rig"] - v_star) / nv)
        best_avg = min(best_avg, np.linalg.norm(-rg.averaged_law(Ls, es, Ws, [0, 0, 0], 1.0) - v_star) / nv)
    print(f"64 rigs, cond(M) <= {worst_cond:.1f}: rig law off by <= {worst_rig:.2e}, averaged twists off by >= {best_avg:.3f}")
    assert worst_rig <= 1e-12
    assert best_avg > 0.1


def test_one_camera_at_the_rig_origin_is_that_cameras_own_law():
    rng = np.random.default_rng(9)
    for pairs in (2, 3, 24):
        L = rg.camera_system(rng, pairs)
        e = rng.standard_normal(2 * pairs) * 0.05
        ref = rg.rig_law([L], [e], [np.eye(6)], [0], 0.7)
        assert np.array_equal(rg.twist_matrix(np.eye(3), np.zeros(3)), np.eye(6))
        assert np.array_equal(ref["v_rig"], -0.7 * (np.linalg.pinv(L, rcond=1e-15) @ e))


def test_cameras_that_do_not_contribute_drop_out():
    Ls, es, Ws, _ = rg.scenario(3, n_cams=4, pairs=6)
    full = rg.rig_law(Ls, es, Ws, [0, 0, 0, 0], 1.0)
    for st in (1, 2, 3):
        part = rg.rig_law(Ls, es, Ws, [0, st, 0, 0], 1.0)
        want = rg.rig_law([Ls[0], Ls[2], Ls[3]], [es[0], es[2], es[3]], [Ws[0], Ws[2], Ws[3]], [0, 0, 0], 1.0)
        assert part["status"] == 0 and part["cameras"] == 3 and part["rows"] == 36
        assert np.array_equal(part["v_rig"], want["v_rig"]) and not np.array_equal(part["v_rig"], full["v_rig"])
    # garbage in a failed camera's rows cannot reach the twist
    Ls[1] = np.full_like(Ls[1], np.nan)
    assert np.array_equal(rg.rig_law(Ls, es, Ws, [0, 2, 0, 0], 1.0)["v_rig"], want["v_rig"])
    # a camera without rows, whatever its status
    empty = rg.rig_law([Ls[0], np.zeros((0, 6)), Ls[2], Ls[3]], [es[0], np.zeros(0), es[2], es[3]], Ws, [0, 0, 0, 0], 1.0)
    assert np.array_equal(empty["v_rig"], want["v_rig"]) and empty["cameras"] == 3


def test_no_camera_contributing_gives_zero_and_the_largest_status():
    Ls, es, Ws, _ = rg.scenario(4, n_cams=3, pairs=4)
    for sts, want in (([1, 1, 1], 1), ([2, 1, 2], 2), ([1, 3, 2], 3)):
        ref = rg.rig_law(Ls, es, Ws, sts, 1.0)
        assert ref["status"] == want and ref["rows"] == 0 and ref["cameras"] == 0
        assert np.array_equal(ref["v_rig"], np.zeros(6))
        assert np.array_equal(rg.averaged_law(Ls, es, Ws, sts, 1.0), np.zeros(6))


def test_normal_equations_of_a_stack_are_the_sums_of_its_parts():
    """What dist.rig_velocity rests on."""
    Ls, es, Ws, _ = rg.scenario(6, n_cams=5, pairs=24)
    whole = rg.normal_packed(*rg.stacked(Ls, es, Ws, [0] * 5))
    parts = sum(rg.normal_packed(*rg.stacked(Ls[a:b], es[a:b], Ws[a:b], [0] * (b - a))) for a, b in ((0, 2), (2, 3), (3, 5)))
    assert whole[27] == parts[27] == 240.0
    assert np.allclose(whole, parts, rtol=1e-13, atol=0)
    assert rg.ldlt_margin(rg.stacked(Ls, es, Ws, [0] * 5)[0]) >= 100
