"""The robust rig law's fp64 statement (tests/rig_robust_ref.py) on the CPU: what the law buys on planted-outlier rigs, and its
equivalences with the laws it is built from.  No device, no library.

Seeds 7000 .. 7063, s_min = 0.03, lambda = 1, N = 4.  The ratios 0.25 / 0.5 / 5 are conditions; measured with the generator as
committed (``test_planted_*`` print the figures):
  case A  3 cameras x 16 pairs, 6 gross outliers all in camera 0 (37 % of that camera, 12.5 % of the rig):
          every planted outlier ends with w = 0 in 64 of 64; robust / plain miss: largest 0.179 (bar < 0.25), cond(M) <= 7.8;
          median miss 0.019 against 0.311 for the stack under each camera's own Tukey weights (bar: >= 5 x), 0.447 plain
  case B  cameras of 4, 16, 16, 16 pairs, 2 of camera 0's 4 wrong: robust / plain miss largest 0.327 (bar < 0.5)"""
import numpy as np
import pytest

import rig_ref as rg
import rig_robust_ref as rr
import robust_ref

SEEDS = range(7000, 7064)
SMIN, LAM, N = 0.03, 1.0, 4


def _per_camera_weights_law(Ls, es, Ws):
    """The stacked solve under each camera's OWN robust_ref weights: what re-weighting per camera and then stacking gives."""
    w = np.concatenate([robust_ref.robust_velocity(L, e, LAM, N, SMIN)["w"] for L, e in zip(Ls, es)])
    M, e = rg.stacked(Ls, es, Ws, [0] * len(Ls))
    return -LAM * robust_ref.weighted_solve(M, e, w)


@pytest.fixture(scope="module")
def case_a():
    rows = []
    for seed in SEEDS:
        Ls, es, Ws, v, outs = rr.planted(seed, [16, 16, 16], [6, 0, 0], smin=SMIN)
        st = [0, 0, 0]
        v_rob, w, _, _, _, _, M, _ = rr.robust_rig_law(Ls, es, Ws, st, None, LAM, N, SMIN)
        rows.append(dict(robust=rr.rel_miss(v_rob, -LAM * v), plain=rr.rel_miss(rg.rig_law(Ls, es, Ws, st, LAM)["v_rig"], -LAM * v),
                         own=rr.rel_miss(_per_camera_weights_law(Ls, es, Ws), -LAM * v), w_out=w[outs[0]], cond=np.linalg.cond(M)))
    return rows


def test_planted_a_every_outlier_is_rejected(case_a):
    assert all((r["w_out"] == 0.0).all() for r in case_a)


def test_planted_a_robust_beats_plain_four_times(case_a):
    ratios = [r["robust"] / r["plain"] for r in case_a]
    print(f"case A robust/plain: largest {max(ratios):.3f}; cond(M) <= {max(r['cond'] for r in case_a):.1f}")
    for key in ("plain", "own", "robust"):
        m = [r[key] for r in case_a]
        print(f"  {key}: min {min(m):.3f} median {np.median(m):.3f} max {max(m):.3f}")
    assert max(ratios) < 0.25, max(ratios)


def test_planted_a_each_cameras_own_weights_are_not_this_law(case_a):
    own, one = np.median([r["own"] for r in case_a]), np.median([r["robust"] for r in case_a])
    print(f"case A median miss: own weights {own:.3f}, one median {one:.3f}")
    assert own >= 5.0 * one, (own, one)


def test_planted_b_a_small_camera_half_wrong():
    ratios = []
    for seed in SEEDS:
        Ls, es, Ws, v, _ = rr.planted(seed, [4, 16, 16, 16], [2, 0, 0, 0], smin=SMIN)
        st = [0] * 4
        rob = rr.rel_miss(rr.robust_rig_law(Ls, es, Ws, st, None, LAM, N, SMIN)[0], -LAM * v)
        ratios.append(rob / rr.rel_miss(rg.rig_law(Ls, es, Ws, st, LAM)["v_rig"], -LAM * v))
    print(f"case B robust/plain: largest {max(ratios):.3f}")
    assert max(ratios) < 0.5, max(ratios)


# ----------------------------------------------------------------------------- equivalences
def test_one_camera_at_the_rig_origin_is_the_cameras_robust_law():
    for seed in (7100, 7101, 7102):
        Ls, es, _, _, _ = rr.planted(seed, [24], [5], smin=SMIN)
        for live in (24, 17):
            L, e = Ls[0].copy(), es[0].copy()
            L[2 * live:] = 0.0
            e[2 * live:] = 0.0
            want = robust_ref.robust_velocity(L, e, 0.35, N, SMIN, n_live=live)
            v, w, rho, sigma, n_zero, margin, _, _ = rr.robust_rig_law([L], [e], [np.eye(6)], [0], [live], 0.35, N, SMIN)
            assert np.linalg.norm(v - want["v_c"]) <= 1e-12 * np.linalg.norm(want["v_c"])
            assert np.abs(w - want["w"]).max() <= 1e-12 and abs(sigma - want["sigma"]) <= 1e-12 * sigma
            assert n_zero == want["n_zero"] and margin == pytest.approx(want["margin"], rel=1e-9)


def test_weights_that_all_stay_one_give_the_plain_rig_law():
    for seed in (1, 2, 3):
        Ls, es, Ws, v_star = rg.scenario(seed, n_cams=3, pairs=8)          # e = M v*, no noise: every residual ~ 0
        st = [0, 0, 0]
        for n in (1, 4):
            v, w, _, sigma, n_zero, _, _, _ = rr.robust_rig_law(Ls, es, Ws, st, None, 0.35, n, SMIN)
            want = rg.rig_law(Ls, es, Ws, st, 0.35)["v_rig"]
            assert sigma == SMIN and n_zero == 0 and np.abs(w - 1.0).max() <= 1e-12
            assert np.linalg.norm(v - want) <= 1e-12 * np.linalg.norm(want)


def test_a_camera_that_does_not_contribute_changes_nothing():
    Ls, es, Ws, _, _ = rr.planted(7200, [8, 8, 8], [2, 0, 1], smin=SMIN)
    base = rr.robust_rig_law(Ls, es, Ws, [0, 0, 0], None, LAM, N, SMIN)
    rng = np.random.default_rng(5)
    extra_L, extra_e, extra_W = rg.camera_system(rng, 8), rng.standard_normal(16), rg.twist_matrix(*rg.random_extrinsic(rng))
    for pos in (0, 1, 3):
        for status, live in ((2, None), (0, 0)):                            # a failed camera; a camera without a live pair
            ins = lambda xs, x: xs[:pos] + [x] + xs[pos:]  # noqa: E731
            got = rr.robust_rig_law(ins(Ls, extra_L), ins(es, extra_e), ins(Ws, extra_W), ins([0, 0, 0], status),
                                    ins([None] * 3, live), LAM, N, SMIN)
            assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1]) and got[3] == base[3]
    none = rr.robust_rig_law(Ls, es, Ws, [2, 1, 3], None, LAM, N, SMIN)
    assert not none[0].any() and none[3] == 0.0 and none[6].shape == (0, 6)


def test_zero_error_gives_a_zero_twist_exactly():
    Ls, es, Ws, _, _ = rr.planted(7201, [8, 8], [0, 0], smin=SMIN)
    v, w, _, sigma, n_zero, _, _, _ = rr.robust_rig_law(Ls, [np.zeros(16)] * 2, Ws, [0, 0], None, LAM, N, SMIN)
    assert np.array_equal(v, np.zeros(6)) and sigma == SMIN and n_zero == 0 and (w == 1.0).all()
