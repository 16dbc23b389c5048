"""The homography law through a handle (vitvs_homography_velocity[_dev], Engine.homography_velocity): on a token grid
through ``Engine.servo_from_nn`` (a tiny handle without weights: the law alone) and through a ViT-S/16 handle's velocity call.

The reference is tests/homography_ref.py on what the velocity call left — ``Engine.last_details``' selected / s_uv / feat / info.
Bars as at the kernel's seam: v_h, H, weights <= 1e-9, sigma <= 1e-12, status and h_info exact; every reference solve keeps its
second-smallest eigenvalue >= 1e-4 of trace(M) and an eigen-gap >= 1e-6, and every residual stays >= 1e-6 off the rejection edge
(asserted here, on the CPU side of each comparison).  The law reads no depth: a velocity call without a depth image (camera status
NO_DEPTH) is followed by the same twist, bit for bit, as one with it."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib, config, synth, weights
from vitvs_amd.engine import Engine, VitvsError

import homography_ref as hr
import robust_ref as rr
import law_support as ls
from law_support import TinyEngines, close_engines  # noqa: F401

pytestmark = pytest.mark.gpu

ENGINES = TinyEngines()           # this module's tiny handles: close_engines closes them at its teardown

G = 14
IMG = 16 * G
_scenario = functools.partial(ls.planted_case, ENGINES, G)
ZHAT = 0.61


def _reference(det, b, cam_status, K, lam, n_iter, pitches, margins=True):
    ref = hr.homography_from_details(det, b, cam_status, K, lam, ZHAT, n_iter, *pitches)
    if margins:
        assert all(g >= 1e-4 for g in ref["ratios"]) and all(g >= 1e-6 for g in ref["gaps"]) and ref["edge"] >= 1e-6, \
            ("choose other inputs", ref["ratios"], ref["gaps"], ref["edge"])
    return ref


def _compare(v, info, b, ref, what):
    info = ls.host(info)
    v = v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
    assert int(info["status"][b]) == ref["status"], (what, info["status"][b], ref["status"])
    got_info = [int(info[name][b]) for name in Engine.HOMOGRAPHY_INFO_FIELDS]
    assert got_info == list(ref["info"][:6]), (what, got_info, ref["info"])
    errs = dict(v=np.abs(v[b] - ref["v"]).max(), H=np.abs(info["H"][b] - ref["H"]).max() / max(1.0, np.abs(ref["H"]).max()),
                weights=np.abs(info["weights"][b] - ref["weights"]).max())
    print(f"{what}: " + ", ".join(f"{k} {e:.1e}" for k, e in errs.items()) + f", ratios {['%.1e' % g for g in ref['ratios']]}")
    assert all(e <= 1e-9 for e in errs.values()), (what, errs)
    assert float(info["sigma"][b]) == ref["sigma"] or abs(float(info["sigma"][b]) - ref["sigma"]) <= 1e-12, what


@pytest.mark.parametrize("num_pairs", [8, 24, 130])
def test_device_equals_the_reference_with_and_without_a_depth_image(num_pairs):
    """Random intrinsics, 12 % wrong matches; N = 0 and 4; 130 pairs: L of the camera's law is global.  The call changes nothing
    the velocity call left, and a velocity call with Z = None (NO_DEPTH) is followed by the same twist bit for bit."""
    eng, params, sc = _scenario(71000 + num_pairs, num_pairs)
    pitches = ls.pitches(params, 16, IMG)
    v_c, st = ls.servo_law(eng, sc)
    assert st == _lib.STATUS_OK
    before = ls.snapshot(eng, v_c)
    with_depth = {}
    for n_iter in (0, 4):
        v, info = eng.homography_velocity(sc["K"], [st], ZHAT, n_iter)
        ref = _reference(before, 0, st, sc["K"], params.lambda_, n_iter, pitches)
        assert ref["status"] == hr.OK or (num_pairs == 8 and n_iter == 4)      # (8 pairs with one wrong match: the first fit maps 6
        _compare(v, info, 0, ref, f"{num_pairs} pairs, N = {n_iter}")          # behind the camera, and 2 rows are too few)
        v_h, info_h = eng.homography_velocity_host(sc["K"], [st], ZHAT, n_iter)          # the host-pointer form: the same launch
        assert np.array_equal(v_h, v.cpu().numpy()) and ls.same_values(ls.host(info), info_h)
        with_depth[n_iter] = (v.cpu().numpy(), ls.host(info))
    assert ls.same_values(ls.snapshot(eng, v_c), before)                   # v_c and every vitvs_last_* output as the velocity call left them
    v_c, st = ls.servo_law(eng, sc, depth=False)
    assert st == _lib.STATUS_NO_DEPTH and not v_c.any()
    for n_iter in (0, 4):
        v, info = eng.homography_velocity(sc["K"], [st], ZHAT, n_iter)
        assert np.array_equal(v.cpu().numpy(), with_depth[n_iter][0]) and ls.same_values(ls.host(info), with_depth[n_iter][1])
        if n_iter == 0:
            assert int(info["status"][0]) == _lib.STATUS_OK and v.cpu().numpy().any()


def test_the_depth_scale_scales_the_translation_alone():
    eng, params, sc = _scenario(71500, 24)
    v_c, st = ls.servo_law(eng, sc)
    v1, i1 = eng.homography_velocity(sc["K"], [st], 1.0)
    v2, i2 = eng.homography_velocity(sc["K"], [st], 0.25)
    v1, v2 = v1.cpu().numpy()[0], v2.cpu().numpy()[0]
    assert np.array_equal(v2[3:], v1[3:]) and np.array_equal(v2[:3], 0.25 * v1[:3]) and torch.equal(i1["H"], i2["H"])


@pytest.mark.parametrize("option", ["subpatch", "interaction_1", "interaction_2", "robust_law"])
def test_with_the_other_law_options(option):
    """subpatch: the moved match (feat's x, y); interaction 1 / 2: feat's depth column holds Z* or Z, which this law never reads;
    robust_law: the camera's own weights do not reach the homography law."""
    eng, params, sc = _scenario(72000 + len(option), 24)
    offsets = None
    if option == "subpatch":
        offsets = np.random.default_rng(7).uniform(-0.5, 0.5, size=(G * G, 2)).astype(np.float32)
    elif option == "robust_law":
        eng.set_option("robust_law", 4)
    else:
        eng.set_goal_depth(np.full((params.v_max, params.u_max), 610, np.uint16))
        eng.set_option("interaction", int(option[-1]))
    v_c, st = ls.servo_law(eng, sc, offsets=offsets)
    assert st == _lib.STATUS_OK
    before = ls.snapshot(eng, v_c)
    if option == "subpatch":
        assert before["offsets"][0, :24].any()
    pitches = ls.pitches(params, 16, IMG)
    for n_iter in (0, 4):
        v, info = eng.homography_velocity(sc["K"], [st], ZHAT, n_iter)
        _compare(v, info, 0, _reference(before, 0, st, sc["K"], params.lambda_, n_iter, pitches), f"{option}, N = {n_iter}")
    assert ls.same_values(ls.snapshot(eng, v_c), before)
    eng.set_option("interaction", 0)
    eng.set_option("robust_law", 0)
    eng.set_goal_depth(None)


def test_camera_statuses_and_the_same_image():
    eng, params, sc = _scenario(73000, 24)
    t = G * G
    # fewer than 4 matches of a short selection: the camera is TOO_FEW, and so is the homography law
    mutual = np.nonzero(sc["nn_2"][sc["nn_1"]] == np.arange(t))[0]
    few = np.intersect1d(mutual, sc["ids"])[:3].astype(np.int32)
    assert len(few) == 3
    v_c, st = ls.servo_law(eng, sc, num_pairs=24, ids=few)
    assert st == _lib.STATUS_TOO_FEW
    v, info = eng.homography_velocity(sc["K"], [st], ZHAT, 4)
    info = ls.host(info)
    assert int(info["status"][0]) == _lib.STATUS_TOO_FEW and not v.cpu().numpy().any() and np.array_equal(info["H"][0], np.eye(3))
    assert not info["weights"].any() and float(info["sigma"][0]) == 0.0
    # the same camera without a depth image reports NO_DEPTH and has written no usable row: the law counts them itself
    v_c, st = ls.servo_law(eng, sc, num_pairs=24, ids=few, depth=False)
    assert st == _lib.STATUS_NO_DEPTH
    v, info = eng.homography_velocity(sc["K"], [st], ZHAT, 4)
    info = ls.host(info)
    assert int(info["status"][0]) == _lib.STATUS_TOO_FEW and not v.cpu().numpy().any() and int(info["usable"][0]) == 0
    # no correspondence
    ident = dict(sc, nn_1=np.arange(t), nn_2=np.arange(t), sim_1=np.full(t, 0.5, np.float32))
    order = np.random.default_rng(1).permutation(t).astype(np.int32)
    v_c, st = ls.servo_law(eng, ident, num_pairs=24, ids=order, select=_lib.SELECT_ORDER)
    assert st == _lib.STATUS_NO_CORRESPONDENCE
    v, info = eng.homography_velocity(sc["K"], [st], ZHAT)
    assert int(info["status"][0]) == _lib.STATUS_NO_CORRESPONDENCE and not v.cpu().numpy().any()
    # the same image: OK, v = 0 and H = I exactly, with and without a depth image
    same = dict(sc, sim_1=np.ones(t, np.float32))
    for depth in (True, False):
        v_c, st = ls.servo_law(eng, same, num_pairs=24, ids=order, select=_lib.SELECT_ORDER, depth=depth)
        det = eng.last_details(1)
        assert st == (_lib.STATUS_OK if depth else _lib.STATUS_NO_DEPTH) and int(det["info"][0, 2]) == 1
        v, info = eng.homography_velocity(sc["K"], [st], ZHAT, 4)
        info = ls.host(info)
        assert int(info["status"][0]) == _lib.STATUS_OK and not v.cpu().numpy().any() and np.array_equal(info["H"][0], np.eye(3))
    # a law of four rows: the fewest the homography takes (spread over the grid: OK), and four of one grid row (collinear)
    cand = np.intersect1d(mutual, sc["ids"])
    for what, four in (("four rows", cand[[0, len(cand) // 3, 2 * len(cand) // 3, -1]]), ("four rows of one line", cand[:4])):
        v_c, st = ls.servo_law(eng, sc, num_pairs=4, ids=four.astype(np.int32))
        assert st == _lib.STATUS_OK
        det = eng.last_details(1)
        ref = _reference(det, 0, st, sc["K"], params.lambda_, 0, ls.pitches(params, 16, IMG), margins=False)
        assert ref["info"][0] == 4
        if what == "four rows":
            assert ref["status"] == hr.OK and ref["ratios"][0] >= 1e-4 and ref["gaps"][0] >= 1e-6
        else:
            assert ref["status"] == hr.TOO_FEW and ref["info"][4] == 1 and abs(ref["ratios"][0]) <= 1e-10
        v, info = eng.homography_velocity(sc["K"], [st], ZHAT)
        _compare(v, info, 0, ref, what)


def test_error_returns():
    params = config.ServoParams(dino_input_size=IMG)
    eng = Engine(ls.tiny_cfg(IMG), params, precision="fp32", max_pairs=2, max_rows=48)
    rng = np.random.default_rng(64)
    sc = rr.planted_scenario(rng, 24, 0.0, params, g=G, holes=True)
    K, st = params.intrinsics(), [0]
    with pytest.raises(VitvsError, match=r"\(-5\)"):           # no law evaluation yet
        eng.homography_velocity(K, st)
    with pytest.raises(VitvsError, match=r"\(-5\)"):
        eng.homography_velocity_host(K, st)
    ls.servo_law(eng, sc)
    v, info = eng.homography_velocity(K, st)
    assert int(info["status"][0]) == _lib.STATUS_OK
    with pytest.raises(VitvsError, match=r"\(-5\)"):           # not the pair count of the last law evaluation
        eng.homography_velocity(K, [0, 0])
    # the C entry points' own checks
    dev = eng.device
    kd = torch.tensor([K], dtype=torch.float64, device=dev)
    sd = torch.zeros(1, dtype=torch.int32, device=dev)
    out, hs = torch.zeros(6, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    f = eng.lib.vitvs_homography_velocity_dev
    assert f(eng.handle, 1, p(kd), p(sd), 1.0, 0, p(out), p(hs), None, None, None, None, None) == 0      # NULL optional outputs
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), v.cpu().numpy()[0])
    for n_iter in (-1, 17):
        assert f(eng.handle, 1, p(kd), p(sd), 1.0, n_iter, p(out), p(hs), None, None, None, None, None) == -2
    for z in (0.0, -1.0, float("inf"), float("nan")):
        assert f(eng.handle, 1, p(kd), p(sd), z, 0, p(out), p(hs), None, None, None, None, None) == -2
    assert f(eng.handle, 1, None, p(sd), 1.0, 0, p(out), p(hs), None, None, None, None, None) == -1
    assert f(eng.handle, 1, p(kd), None, 1.0, 0, p(out), p(hs), None, None, None, None, None) == -1
    assert f(eng.handle, 1, p(kd), p(sd), 1.0, 0, None, p(hs), None, None, None, None, None) == -1
    assert f(eng.handle, 1, p(kd), p(sd), 1.0, 0, p(out), None, None, None, None, None, None) == -1
    eng.close()


def test_through_a_vits16_handle():
    """Three pairs in one call through the forward's velocity call, with a depth image and without; a captured update replayed."""
    cfg = config.baseline_config("vits16_224")
    params = config.ServoParams(dino_input_size=cfg.img_size, use_feature_binning=False)
    eng = Engine(cfg, params, precision="fp32", max_pairs=3).load_state_dict(weights.synthetic_state_dict(cfg, 0))
    des, cur = synth.frame_pair(cfg.img_size, 20250705)
    depth, K = synth.depth_pattern(), params.intrinsics()
    k, n = params.num_pairs, 3
    three = lambda a: np.stack([a] * n)   # noqa: E731
    orders = np.stack([np.random.default_rng(70 + b).permutation(cfg.tokens) for b in range(n)]).astype(np.int32)
    pitches = ls.pitches(params, cfg.stride, cfg.img_size)

    def check(v_c, st, what):
        st_h = st.cpu().numpy()
        before = dict(eng.last_details(n), v_c=v_c.cpu().numpy().copy())
        out = {}
        for n_iter in (0, 4):
            v, info = eng.homography_velocity(K, st, ZHAT, n_iter)
            for b in range(n):
                ref = _reference(before, b, st_h[b], K, params.lambda_, n_iter, pitches)
                _compare(v, info, b, ref, f"{what}, pair {b}, N = {n_iter}")
            out[n_iter] = (v.cpu().numpy(), ls.host(info))
        assert ls.same_values(dict(eng.last_details(n), v_c=v_c.cpu().numpy()), before)
        return out

    v_c, st = eng.compute_velocity(three(cur), three(des), three(depth), K, mode=_lib.SELECT_ORDER, selection=orders)
    assert not st.cpu().numpy().any()
    first = check(v_c, st, "eager")
    assert not np.array_equal(first[0][0][0], first[0][0][1])   # other draws, other rows
    assert all(int(s) == _lib.STATUS_OK for s in first[0][1]["status"])
    # no depth image: every camera reports NO_DEPTH, the homography twists are the same bit for bit
    v_c, st = eng.compute_velocity(three(cur), three(des), None, K, mode=_lib.SELECT_ORDER, selection=orders)
    assert list(st.cpu().numpy()) == [_lib.STATUS_NO_DEPTH] * n
    for n_iter in (0, 4):
        v, info = eng.homography_velocity(K, st, ZHAT, n_iter)
        assert np.array_equal(v.cpu().numpy(), first[n_iter][0]) and ls.same_values(ls.host(info), first[n_iter][1])
    # a captured update, replayed: the homography law is valid behind it
    eng.set_option("graph_replay", 1)
    cur_d, des_d = eng._frames(three(cur)), eng._frames(three(des))
    z_d = torch.as_tensor(three(depth)).to(eng.device).contiguous()
    k_d = torch.as_tensor(K, dtype=torch.float64).reshape(1, 4).expand(n, 4).contiguous().to(eng.device)
    sel_d, cnt_d = eng._selection_args(_lib.SELECT_ORDER, torch.from_numpy(orders), n, cfg.tokens, k)
    out_v = torch.zeros((n, 6), dtype=torch.float64, device=eng.device)
    out_s = torch.zeros(n, dtype=torch.int32, device=eng.device)
    for _ in range(2):
        eng.compute_velocity_dev(cur_d, des_d, z_d, k_d, _lib.SELECT_ORDER, sel_d, cnt_d, out_v=out_v, out_status=out_s, num_pairs=k)
    replayed = check(out_v, out_s, "replayed")
    assert all(np.array_equal(replayed[n_iter][0], first[n_iter][0]) for n_iter in (0, 4))
    eng.close()
