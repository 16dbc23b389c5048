"""The pose law through a handle (vitvs_pose_velocity[_dev], Engine.pose_velocity): on a token grid through
``Engine.servo_from_nn`` (a tiny handle without weights: the law alone) and through a ViT-S/16 handle's velocity call.

The reference is tests/pose_ref.py on what the velocity call left — ``Engine.last_details``' selected / s_uv / feat / info — and
the goal-depth table restated on the host (the goal depth at every goal token's patch centre).  Bars as at the kernel's seam:
v_pose, R, t, weights <= 1e-9, sigma <= 1e-12, status and pose_info exact; every reference solve keeps a relative eigen-gap >= 1e-6
and every residual stays >= 1e-6 off the rejection edge (asserted here, on the CPU side of each comparison)."""
import ctypes as C

import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib, config, synth, weights
from vitvs_amd.engine import Engine, VitvsError

import interaction_ref as ir
import pose_ref as pr
import robust_ref as rr
import law_support as ls
from law_support import TinyEngines, close_engines  # noqa: F401

pytestmark = pytest.mark.gpu

ENGINES = TinyEngines()           # this module's tiny handles: close_engines closes them at its teardown

G = 14
IMG = 16 * G


def _reference(det, b, cam_status, K, table, lam, n_iter, pitches, degenerate=False):
    with np.errstate(all="ignore"):
        ref = pr.pose_from_details(det, b, cam_status, K, table, lam, n_iter, *pitches)
    if not degenerate:
        assert all(g >= 1e-6 for g in ref["gaps"]) and ref["edge"] >= 1e-6, ("choose other inputs", ref["gaps"], ref["edge"])
    return ref


def _compare(v, info, b, ref, what, up_to_sign=False):
    info = ls.host(info)
    v = v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
    assert int(info["status"][b]) == ref["status"], (what, info["status"][b], ref["status"])
    got_info = [int(info[name][b]) for name in Engine.POSE_INFO_FIELDS]
    assert got_info == list(ref["info"][:6]), (what, got_info, ref["info"])
    w_ref = v[b, 3:] if not up_to_sign or np.dot(v[b, 3:], ref["v"][3:]) >= 0 else -v[b, 3:]
    errs = dict(v=np.abs(v[b, :3] - ref["v"][:3]).max(), w=np.abs(w_ref - ref["v"][3:]).max(), R=np.abs(info["R"][b] - ref["R"]).max(),
                t=np.abs(info["t"][b] - ref["t"]).max(), weights=np.abs(info["weights"][b] - ref["weights"]).max())
    print(f"{what}: " + ", ".join(f"{k} {e:.1e}" for k, e in errs.items()) + f", gaps {['%.1e' % g for g in ref['gaps']]}")
    assert all(e <= 1e-9 for e in errs.values()), (what, errs)
    assert abs(float(info["sigma"][b]) - ref["sigma"]) <= 1e-12, what


def _scenario(seed, num_pairs, share=0.125):
    eng, params = ENGINES.fetch(G, 130, reset=ls.LAW_OPTIONS)
    rng = np.random.default_rng(seed)
    K = (float(rng.uniform(300, 700)), float(rng.uniform(300, 700)), params.u_max / 2 + float(rng.uniform(-20, 20)),
         params.v_max / 2 + float(rng.uniform(-20, 20)))
    sc = rr.planted_scenario(rng, num_pairs, share, params, K=K, g=G, holes=True)
    return eng, params, sc, ls.goal_depth(rng)


@pytest.mark.parametrize("num_pairs", [8, 24, 130])
def test_device_equals_the_reference_and_leaves_the_call_untouched(num_pairs):
    """Holes in both depth images, random intrinsics, 12 % wrong matches; N = 0 and 4; 130 pairs: L of the camera's law is global."""
    eng, params, sc, zg = _scenario(61000 + num_pairs, num_pairs)
    eng.set_goal_depth(zg)
    v_c, st = ls.servo_law(eng, sc)
    assert st == _lib.STATUS_OK
    before = ls.snapshot(eng, v_c)
    table, pitches = ls.goal_table(zg, G, IMG, params), ls.pitches(params, 16, IMG)
    holes = 0
    for n_iter in (0, 4):
        v, info = eng.pose_velocity(sc["K"], [st], n_iter)
        ref = _reference(before, 0, st, sc["K"], table, params.lambda_, n_iter, pitches)
        _compare(v, info, 0, ref, f"{num_pairs} pairs, N = {n_iter}")
        holes = int(ref["info"][5])
        # the host-pointer form: the same launch
        v_h, info_h = eng.pose_velocity_host(sc["K"], [st], n_iter)
        assert np.array_equal(v_h, v.cpu().numpy()) and ls.same_values(ls.host(info), info_h)
    assert holes > 0 or num_pairs == 8                          # the depth images have holes: some rows are dropped
    assert ls.same_values(ls.snapshot(eng, v_c), before)                   # v_c and every vitvs_last_* output as the velocity call left them


def test_quarter_turn_has_no_retreat():
    """§5c's case: the image-based law backs away at 0.61 m/s for lambda = 1; the pose law turns on the spot."""
    case = ir.quarter_turn_case()
    eng, params = ENGINES.fetch(G, 130, lam=case["lam"], reset=ls.LAW_OPTIONS)
    eng.set_goal_depth(case["goal_depth"])
    v_c, st = ls.servo_law(eng, case)
    assert st == _lib.STATUS_OK and abs(v_c[2] + 0.61) < 0.01
    det = eng.last_details(1)
    v, info = eng.pose_velocity(case["K"], [st])
    ref = _reference(det, 0, st, case["K"], ls.goal_table(case["goal_depth"], G, IMG, params), case["lam"], 0, ls.pitches(params, 16, IMG))
    _compare(v, info, 0, ref, "quarter turn")
    v = v.cpu().numpy()[0]
    print(f"quarter turn: image-based v_z = {v_c[2]:+.4f}, pose law v_z = {v[2]:+.2e}, w_z = {v[5]:+.4f}")
    assert abs(v[2]) <= 1e-9 and abs(abs(v[5]) - case["lam"] * np.pi / 2) < 0.02 and np.abs(v[3:5]).max() <= 1e-9


def test_half_turn():
    """nn_1 is the point reflection of the grid: the image-based law sees no rotation at all, the pose law turns by pi (whose
    sign is free at exactly pi: the twist's rotation is compared up to it)."""
    case = ir.quarter_turn_case()
    t = G * G
    nn1 = (t - 1 - np.arange(t)).astype(np.int64)
    nn2 = nn1.copy()
    nn2[[nn1[0], nn1[1], nn1[2]]] = (np.array([0, 1, 2]) + 50) % t          # tokens 0, 1, 2 are not mutual (no goal token of `ids`)
    case = dict(case, nn_1=nn1, nn_2=nn2)
    eng, params = ENGINES.fetch(G, 130, lam=case["lam"], reset=ls.LAW_OPTIONS)
    eng.set_goal_depth(case["goal_depth"])
    v_c, st = ls.servo_law(eng, case)
    assert st == _lib.STATUS_OK
    det = eng.last_details(1)
    v, info = eng.pose_velocity(case["K"], [st])
    ref = _reference(det, 0, st, case["K"], ls.goal_table(case["goal_depth"], G, IMG, params), case["lam"], 0, ls.pitches(params, 16, IMG))
    _compare(v, info, 0, ref, "half turn", up_to_sign=True)
    v = v.cpu().numpy()[0]
    print(f"half turn: image-based w_z = {v_c[5]:+.4f}, pose law |w_z| = {abs(v[5]):.6f}, v_z = {v[2]:+.2e}")
    assert abs(abs(v[5]) - case["lam"] * np.pi) < 0.02 and abs(v[2]) <= 1e-9 and abs(v_c[5]) < 0.02


@pytest.mark.parametrize("option", ["subpatch", "interaction", "robust_law"])
def test_with_the_other_law_options(option):
    """subpatch: the moved match (feat's x, y) and the depth under it; interaction 2: feat keeps Z; robust_law: the camera's own
    weights do not reach the pose law."""
    eng, params, sc, zg = _scenario(62000 + len(option), 24)
    eng.set_goal_depth(zg)
    offsets = None
    if option == "subpatch":
        offsets = np.random.default_rng(7).uniform(-0.5, 0.5, size=(G * G, 2)).astype(np.float32)
    else:
        eng.set_option(option, 2 if option == "interaction" else 4)
    v_c, st = ls.servo_law(eng, sc, offsets=offsets)
    assert st == _lib.STATUS_OK
    det = eng.last_details(1)
    if option == "subpatch":
        assert det["offsets"][0, :24].any()
    table, pitches = ls.goal_table(zg, G, IMG, params), ls.pitches(params, 16, IMG)
    for n_iter in (0, 4):
        v, info = eng.pose_velocity(sc["K"], [st], n_iter)
        _compare(v, info, 0, _reference(det, 0, st, sc["K"], table, params.lambda_, n_iter, pitches), f"{option}, N = {n_iter}")
    eng.set_option(option, 0)


def test_camera_statuses_and_the_same_image():
    eng, params, sc, zg = _scenario(63000, 24)
    eng.set_goal_depth(zg)
    t = G * G
    # fewer than 4 matches of a short selection: the camera is TOO_FEW, and so is the pose law
    mutual = np.nonzero(sc["nn_2"][sc["nn_1"]] == np.arange(t))[0]
    few = np.intersect1d(mutual, sc["ids"])[:3].astype(np.int32)
    assert len(few) == 3
    v_c, st = ls.servo_law(eng, sc, num_pairs=24, ids=few)
    assert st == _lib.STATUS_TOO_FEW
    v, info = eng.pose_velocity(sc["K"], [st], 4)
    info = ls.host(info)
    assert int(info["status"][0]) == _lib.STATUS_TOO_FEW and not v.cpu().numpy().any() and np.array_equal(info["R"][0], np.eye(3))
    assert not info["weights"].any() and float(info["sigma"][0]) == 0.0
    # no correspondence
    ident = dict(sc, nn_1=np.arange(t), nn_2=np.arange(t), sim_1=np.full(t, 0.5, np.float32))
    order = np.random.default_rng(1).permutation(t).astype(np.int32)
    v_c, st = ls.servo_law(eng, ident, num_pairs=24, ids=order, select=_lib.SELECT_ORDER)
    assert st == _lib.STATUS_NO_CORRESPONDENCE
    v, info = eng.pose_velocity(sc["K"], [st])
    assert int(info["status"][0]) == _lib.STATUS_NO_CORRESPONDENCE and not v.cpu().numpy().any()
    # the same image: OK, v = 0 and R = I exactly
    same = dict(sc, sim_1=np.ones(t, np.float32))
    v_c, st = ls.servo_law(eng, same, num_pairs=24, ids=order, select=_lib.SELECT_ORDER)
    det = eng.last_details(1)
    assert st == _lib.STATUS_OK and int(det["info"][0, 2]) == 1
    v, info = eng.pose_velocity(sc["K"], [st], 4)
    info = ls.host(info)
    assert int(info["status"][0]) == _lib.STATUS_OK and not v.cpu().numpy().any()
    assert np.array_equal(info["R"][0], np.eye(3)) and not info["t"].any()
    # a law of four rows: the pose law counts its own usable rows (a hole in either depth leaves fewer than the camera's four)
    four = np.intersect1d(mutual, sc["ids"])[:4].astype(np.int32)
    v_c, st = ls.servo_law(eng, sc, num_pairs=4, ids=four)
    assert st == _lib.STATUS_OK
    det = eng.last_details(1)
    table, pitches = ls.goal_table(zg, G, IMG, params), ls.pitches(params, 16, IMG)
    ref = _reference(det, 0, st, sc["K"], table, params.lambda_, 0, pitches, degenerate=True)
    v, info = eng.pose_velocity(sc["K"], [st])
    _compare(v, info, 0, ref, "four rows")


def test_error_returns():
    params = config.ServoParams(dino_input_size=IMG)
    eng = Engine(ls.tiny_cfg(IMG), params, precision="fp32", max_pairs=2, max_rows=48)
    rng = np.random.default_rng(64)
    sc = rr.planted_scenario(rng, 24, 0.0, params, g=G, holes=True)
    zg = ls.goal_depth(rng)
    K, st = params.intrinsics(), [0]
    eng.set_goal_depth(zg)
    with pytest.raises(VitvsError, match=r"\(-5\)"):           # no law evaluation yet
        eng.pose_velocity(K, st)
    ls.servo_law(eng, sc)
    eng.pose_velocity(K, st)
    with pytest.raises(VitvsError, match=r"\(-5\)"):           # not the pair count of the last law evaluation
        eng.pose_velocity(K, [0, 0])
    eng.set_goal_depth(None)
    with pytest.raises(VitvsError, match=r"\(-5\)"):           # no goal depth
        eng.pose_velocity(K, st)
    with pytest.raises(VitvsError, match=r"\(-5\)"):
        eng.pose_velocity_host(K, st)
    eng.set_goal_depth(np.stack([zg, zg]))
    with pytest.raises(VitvsError, match=r"\(-5\)"):           # two goal images, one pair
        eng.pose_velocity(K, st)
    eng.set_goal_depth(zg)
    eng.set_option("interaction", 1)
    ls.servo_law(eng, sc)
    with pytest.raises(VitvsError, match=r"\(-5\)"):           # feat holds Z*, not Z
        eng.pose_velocity(K, st)
    eng.set_option("interaction", 0)
    ls.servo_law(eng, sc)
    v, info = eng.pose_velocity(K, st)
    assert int(info["status"][0]) == _lib.STATUS_OK
    # the C entry points' own checks
    dev = eng.device
    kd = torch.tensor([K], dtype=torch.float64, device=dev)
    sd = torch.zeros(1, dtype=torch.int32, device=dev)
    out, ps = torch.zeros(6, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    f = eng.lib.vitvs_pose_velocity_dev
    assert f(eng.handle, 1, p(kd), p(sd), 0, p(out), p(ps), None, None, None, None, None) == 0          # NULL optional outputs
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), v.cpu().numpy()[0])
    for n_iter in (-1, 17):
        assert f(eng.handle, 1, p(kd), p(sd), n_iter, p(out), p(ps), None, None, None, None, None) == -2
    assert f(eng.handle, 1, None, p(sd), 0, p(out), p(ps), None, None, None, None, None) == -1
    assert f(eng.handle, 1, p(kd), None, 0, p(out), p(ps), None, None, None, None, None) == -1
    assert f(eng.handle, 1, p(kd), p(sd), 0, None, p(ps), None, None, None, None, None) == -1
    assert f(eng.handle, 1, p(kd), p(sd), 0, p(out), None, None, None, None, None, None) == -1
    eng.close()


def test_through_a_vits16_handle():
    """Three pairs sharing one goal depth image through the forward's velocity call; a captured update replayed before and after
    the goal depth is rewritten in place."""
    cfg = config.baseline_config("vits16_224")
    params = config.ServoParams(dino_input_size=cfg.img_size, use_feature_binning=False)
    eng = Engine(cfg, params, precision="fp32", max_pairs=3).load_state_dict(weights.synthetic_state_dict(cfg, 0))
    des, cur = synth.frame_pair(cfg.img_size, 20250705)
    rng = np.random.default_rng(65)
    depth, K = synth.depth_pattern(), params.intrinsics()
    zg, zg2 = ls.goal_depth(rng), ls.goal_depth(rng)
    k, g, n = params.num_pairs, cfg.grid, 3
    three = lambda a: np.stack([a] * n)   # noqa: E731
    orders = np.stack([np.random.default_rng(70 + b).permutation(cfg.tokens) for b in range(n)]).astype(np.int32)
    eng.set_goal_depth(zg)                                      # n_goal = 1 serves the three pairs
    pitches = ls.pitches(params, cfg.stride, cfg.img_size)

    def check(v_c, st, goal, what):
        st_h = st.cpu().numpy()
        before = dict(eng.last_details(n), v_c=v_c.cpu().numpy().copy())
        table = ls.goal_table(goal, g, cfg.img_size, params)
        for n_iter in (0, 4):
            v, info = eng.pose_velocity(K, st, n_iter)
            for b in range(n):
                ref = _reference(before, b, st_h[b], K, table, params.lambda_, n_iter, pitches)
                _compare(v, info, b, ref, f"{what}, pair {b}, N = {n_iter}")
        assert ls.same_values(dict(eng.last_details(n), v_c=v_c.cpu().numpy()), before)
        return v.cpu().numpy()

    v_c, st = eng.compute_velocity(three(cur), three(des), three(depth), K, mode=_lib.SELECT_ORDER, selection=orders)
    assert not st.cpu().numpy().any()
    v1 = check(v_c, st, zg, "eager")
    assert not np.array_equal(v1[0], v1[1])                     # other draws, other rows
    # a captured update, replayed: the pose law is valid behind it
    eng.set_option("graph_replay", 1)
    cur_d, des_d = eng._frames(three(cur)), eng._frames(three(des))
    z_d = torch.as_tensor(three(depth)).to(eng.device).contiguous()
    k_d = torch.as_tensor(K, dtype=torch.float64).reshape(1, 4).expand(n, 4).contiguous().to(eng.device)
    sel_d, cnt_d = eng._selection_args(_lib.SELECT_ORDER, torch.from_numpy(orders), n, cfg.tokens, k)
    out_v = torch.zeros((n, 6), dtype=torch.float64, device=eng.device)
    out_s = torch.zeros(n, dtype=torch.int32, device=eng.device)
    for _ in range(2):
        eng.compute_velocity_dev(cur_d, des_d, z_d, k_d, _lib.SELECT_ORDER, sel_d, cnt_d, out_v=out_v, out_status=out_s, num_pairs=k)
    v2 = check(out_v, out_s, zg, "replayed")
    assert np.array_equal(v2, v1)
    eng.set_goal_depth(torch.as_tensor(zg2).to(eng.device))     # rewritten in place, in stream order
    eng.compute_velocity_dev(cur_d, des_d, z_d, k_d, _lib.SELECT_ORDER, sel_d, cnt_d, out_v=out_v, out_status=out_s, num_pairs=k)
    v3 = check(out_v, out_s, zg2, "replayed, new goal depth")
    assert not np.array_equal(v3, v1)
    eng.close()
