"""The roll search through the handle (vitvs_roll_velocity[_dev]) on tiny engines WITH weights (GPU).

``Engine.roll_velocity`` must equal the composition of calls that existed before it: ``numpy.rot90`` on the host, one
``compute_velocity(des_shared=True)`` over the four copies, ``last_details`` for the tables, tests/roll_ref.py for the pick and
the carry-back, ``servo_from_nn`` with the real depth image.  The launches and their inputs are the same, so k*, the tables,
s_uv, v_c and the status are compared bit for bit; v_c is also held against the oracle's law on the carried-back tables.

A square camera whose current frame is exactly ``rot90(goal, 1)`` is the case the law's change exists for: candidate 3 falls
under the same-image shortcut, and the twist must turn the camera instead of being zero.

Configurations: 2-block, 128-wide networks (``law_support.tiny_cfg``) with ``weights.synthetic_state_dict``, token grids of 4 and
14 per side, max_pairs = 4, fp32 and bf16."""
import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib, config, synth, weights
from vitvs_amd.engine import Engine, VitvsError
import law_support as ls
from law_support import close_engines  # noqa: F401
import robust_ref as rr
import roll_ref as rf

pytestmark = pytest.mark.gpu


class _Engines:
    """Tiny engines with weights, one per (g, precision, square camera, max_pairs), made on first use."""

    def __init__(self):
        self.engines = {}

    def fetch(self, g, precision="fp32", square=False, max_pairs=4):
        key = (g, precision, square, max_pairs)
        if key not in self.engines:
            img = 16 * g
            cam = dict(u_max=480, v_max=480) if square else {}
            params = config.ServoParams(dino_input_size=img, use_feature_binning=False, **cam)
            cfg = ls.tiny_cfg(img)
            eng = Engine(cfg, params, precision=precision, max_pairs=max_pairs, max_rows=max(48, g * g))
            self.engines[key] = (eng.load_state_dict(weights.synthetic_state_dict(cfg, 0)), params)
        eng, params = self.engines[key]
        for option in ls.LAW_OPTIONS:
            eng.set_option(option, 0)
        eng.set_frame_size()
        return eng, params

    def close(self):
        for eng, _ in self.engines.values():
            eng.close()
        self.engines.clear()


ENGINES = _Engines()


def _frames(g, m, seed=20250705):
    """(goal, current): a synthetic pair at 16 g pixels, the current frame turned by m quarter turns."""
    des, cur = synth.frame_pair(16 * g, seed)
    return des, np.ascontiguousarray(np.rot90(cur, m))


def _composition(eng, g, cur, des, Z, K, mode, selection, num_pairs, cached):
    """The roll call spelled out with the calls that existed before it -> (pick, v_c, status, details)."""
    turned = np.stack([np.rot90(cur, k) for k in range(4)])
    if cached:
        eng.set_goal(des)
    eng.compute_velocity(turned, None if cached else des[None], np.stack([Z] * 4), K, mode=_lib.SELECT_DENSE, des_shared=True)
    tabs = eng.last_details(4)
    want = rf.pick(tabs["nn_1"], tabs["nn_2"], tabs["sim_1"], g)
    v, st = eng.servo_from_nn(want["nn_1"], want["nn_2"], want["sim_1"], Z, K, mode=mode, selection=selection, num_pairs=num_pairs)
    return want, v.cpu().numpy(), int(st), eng.last_details(1)


def _same_update(want, v, st, det, v2, st2, info, det2, what):
    assert info["roll"] == want["roll"], (what, info, want["roll_info"])
    assert np.array_equal(info["n_mutual"], want["n_mutual"]) and info["same_image"] == want["same_image"], (what, info)
    assert np.array_equal(np.isnan(info["scores"]), np.isnan(want["scores"])), (what, info["scores"], want["scores"])
    ok = ~np.isnan(want["scores"])
    assert np.all(np.abs(info["scores"][ok] - want["scores"][ok]) <= 1e-12 * np.abs(want["scores"][ok])), what
    for name in ("nn_1", "nn_2"):
        assert np.array_equal(det2[name][0], want[name]), (what, name)
    assert np.array_equal(det2["sim_1"][0].view(np.uint32), want["sim_1"].view(np.uint32)), what
    assert st2 == st, (what, st2, st)
    assert np.array_equal(v2.view(np.uint64), v.view(np.uint64)), (what, v2, v)
    for name in ("info", "selected", "s_uv", "feat", "L", "weights", "Z_goal"):
        assert np.array_equal(det2[name], det[name], equal_nan=True), (what, name)


def _selection(mode, T, seed):
    if mode != _lib.SELECT_ORDER:
        return None
    return torch.randperm(T, generator=torch.Generator().manual_seed(seed)).to(torch.int32)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("g,m", [(4, 1), (14, 1), (14, 2)])
def test_roll_velocity_is_the_composition_of_existing_calls(g, m, precision):
    eng, params = ENGINES.fetch(g, precision)
    T, img = g * g, 16 * g
    rng = np.random.default_rng(10 * g + m)
    des, cur = _frames(g, m)
    Z, K = ls.depth(rng), ls.intrinsics(rng, params)
    want, v, st, det = _composition(eng, g, cur, des, Z, K, _lib.SELECT_DENSE, None, None, cached=False)
    v2, st2, info = eng.roll_velocity(cur, des, Z, K, mode=_lib.SELECT_DENSE)
    det2 = eng.last_details(1)
    _same_update(want, v, st, det, v2.cpu().numpy(), int(st2), info, det2, (g, m, precision))
    print(f"g {g}, turned by {m}, {precision}: k* = {info['roll']}, scores {np.round(info['scores'], 4)}, n_mutual {info['n_mutual']}, status {st}")
    # ... and the oracle's law on the carried-back tables
    if st == _lib.STATUS_OK:
        ids = np.nonzero(rf.mutual(want["nn_1"], want["nn_2"]))[0]
        assert int(det2["info"][0, 0]) == len(ids) and int(det2["info"][0, 2]) == 0
        _, _, ref = ls.oracle(g, img, params, want["nn_1"].astype(np.int64), ids, len(ids), Z, K)
        if ls.ldlt_passes(ref["L"]):                              # (a well-conditioned system: the bar of tests/test_gpu_servo_cover.py)
            assert rr.rel_l2(v2.cpu().numpy(), ref["v_c"]) <= 1e-9, (g, m, precision)
        else:
            assert g == 4, "only the 16-token grid may leave too few matches for a well-conditioned system"


@pytest.mark.parametrize("variant", ["cached goal", "order", "best", "robust_law", "interaction", "host form"])
def test_the_composition_holds_under_the_options(variant):
    g, m = 14, 3
    eng, params = ENGINES.fetch(g, "fp32")
    T = g * g
    rng = np.random.default_rng(sum(map(ord, variant)))
    des, cur = _frames(g, m, seed=20250715)
    Z, K = ls.depth(rng), ls.intrinsics(rng, params)
    mode = {"order": _lib.SELECT_ORDER, "best": _lib.SELECT_BEST}.get(variant, _lib.SELECT_DENSE)
    num_pairs = 24 if mode != _lib.SELECT_DENSE else None
    sel = _selection(mode, T, 5)
    if variant == "robust_law":
        eng.set_option("robust_law", 2)
    if variant == "interaction":
        eng.set_goal_depth(ls.goal_depth(rng))
        eng.set_option("interaction", 2)
    cached = variant == "cached goal"
    want, v, st, det = _composition(eng, g, cur, des, Z, K, mode, sel, num_pairs, cached)
    if variant == "host form":
        v2, st2, info = eng.roll_velocity_host(cur, des, Z, K, mode=mode, selection=sel, num_pairs=num_pairs)
    else:
        v2, st2, info = eng.roll_velocity(cur, None if cached else des, Z, K, mode=mode, selection=sel, num_pairs=num_pairs)
        v2, st2 = v2.cpu().numpy(), int(st2)
    det2 = eng.last_details(1)
    _same_update(want, v, st, det, v2, st2, info, det2, variant)
    assert st == _lib.STATUS_OK, (variant, st)                  # (the case exercises the law, not a refusal)
    if variant == "robust_law":
        assert int(det2["info"][0, 6]) == 2
    if variant == "interaction":
        assert det2["Z_goal"].any()
    if variant == "best":
        assert sorted(eng.last_order(1)[0].tolist()) == list(range(T))      # the roll call's own BEST order: a permutation
    eng.set_goal_depth(None)


def _angle_about_z(R):
    R = np.asarray(R, np.float64)
    return float(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0))), float(R[2, 2])


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("g", [4, 14])
def test_a_quarter_turn_from_the_goal_turns_the_camera(g, precision):
    """A square camera exactly a quarter turn from the goal: candidate 3 IS the goal image.  Without the law's change the shortcut
    pairs every token with itself, the twist is zero forever and the follow-on laws take their at-goal early out."""
    eng, params = ENGINES.fetch(g, precision, square=True)
    T = g * g
    goal = synth.texture(16 * g, 31)
    cur = np.ascontiguousarray(np.rot90(goal, 1))
    Z = np.full((480, 480), 610, np.uint16)                       # a fronto-parallel plane: Z = Z* at every matched point
    K = params.intrinsics()
    eng.set_goal_depth(Z)
    v, st, info = eng.roll_velocity(cur, goal, Z, K, mode=_lib.SELECT_DENSE)
    det = eng.last_details(1)
    v = v.cpu().numpy()
    assert info["roll"] == 3 and info["same_image"], info
    assert int(st) == _lib.STATUS_OK and int(det["info"][0, 2]) == 0 and int(det["info"][0, 1]) == T, det["info"]
    assert np.array_equal(det["nn_1"][0], rf.perm(g, 3)), "candidate 3's identity table, carried back"
    assert np.all(det["feat"][0, :T, 3] == 1.0)                   # the shortcut's similarity stays 1
    assert abs(v[5]) > 1e-3 and abs(v[5]) > 10 * max(abs(v[3]), abs(v[4])), v     # it turns about the optical axis
    vp, pinfo = eng.pose_velocity(K, [int(st)], 0)
    pinfo = ls.host(pinfo)
    assert int(pinfo["status"][0]) == _lib.STATUS_OK and int(pinfo["usable"][0]) == T
    ang, rzz = _angle_about_z(pinfo["R"][0])
    assert abs(ang - np.pi / 2) <= 1e-9 and abs(rzz - 1.0) <= 1e-9, (ang, rzz)
    assert np.linalg.norm(pinfo["t"][0]) <= 1e-9
    assert abs(abs(vp.cpu().numpy()[0, 5]) - params.lambda_ * np.pi / 2) <= 1e-9
    vh, hinfo = eng.homography_velocity(K, [int(st)], 0.61, 0)
    hinfo = ls.host(hinfo)
    assert int(hinfo["status"][0]) == _lib.STATUS_OK
    ang, rzz = _angle_about_z(hinfo["H"][0])
    assert abs(ang - np.pi / 2) <= 1e-9 and abs(rzz - 1.0) <= 1e-9, (ang, rzz)
    assert np.linalg.norm(vh.cpu().numpy()[0, 3:]) > 1e-3
    eng.set_goal_depth(None)


def test_at_the_goal_the_search_changes_nothing():
    g = 14
    eng, params = ENGINES.fetch(g, "fp32")
    rng = np.random.default_rng(8)
    goal = synth.texture(16 * g, 31)
    Z, K = ls.depth(rng), ls.intrinsics(rng, params)
    v1, st1 = eng.compute_velocity(goal[None], goal[None], Z[None], K, mode=_lib.SELECT_ORDER, selection=_selection(_lib.SELECT_ORDER, g * g, 9),
                                   num_pairs=24)
    det1 = eng.last_details(1)
    v2, st2, info = eng.roll_velocity(goal, goal, Z, K, mode=_lib.SELECT_ORDER, selection=_selection(_lib.SELECT_ORDER, g * g, 9), num_pairs=24)
    det2 = eng.last_details(1)
    assert info["roll"] == 0 and info["same_image"] and int(det2["info"][0, 2]) == 1
    assert int(st2) == int(st1[0]) == _lib.STATUS_OK
    assert np.array_equal(v2.cpu().numpy(), v1.cpu().numpy()[0]) and not v2.cpu().numpy().any()
    for name in ("info", "selected", "s_uv", "feat", "nn_1", "nn_2"):
        assert np.array_equal(det2[name], det1[name]), name


def test_refusals():
    g = 4
    des, cur = _frames(g, 1)
    rng = np.random.default_rng(1)
    small, params = ENGINES.fetch(g, "fp32", max_pairs=3)
    Z, K = ls.depth(rng), ls.intrinsics(rng, params)
    with pytest.raises(VitvsError, match=r"\(-3\).*max_pairs"):
        small.roll_velocity(cur, des, Z, K)
    with pytest.raises(VitvsError, match=r"\(-3\)"):
        small.roll_velocity_host(cur, des, Z, K)
    eng, params = ENGINES.fetch(g, "fp32")
    eng.set_option("subpatch", 1)
    with pytest.raises(VitvsError, match=r"\(-5\).*subpatch"):
        eng.roll_velocity(cur, des, Z, K)
    eng.set_option("subpatch", 0)
    eng.set_frame_size(480, 640)
    with pytest.raises(VitvsError, match=r"\(-5\).*img_size"):
        eng.roll_velocity(cur, des, Z, K)
    eng.set_frame_size()
    with pytest.raises(VitvsError, match=r"\(-5\).*cached"):
        eng.roll_velocity(cur, None, Z, K)                       # no goal of one image is cached
    with pytest.raises(VitvsError):
        eng.roll_velocity(np.zeros((16 * g, 8 * g, 3), np.uint8), des, Z, K)
    v, st, info = eng.roll_velocity(cur, des, Z, K)              # and the handle still works
    assert info["roll"] in (-1, 0, 1, 2, 3)
    # quarter_turns through the handle, whatever frame size is set
    eng.set_frame_size(480, 640)
    out = eng.quarter_turns(np.stack([des, cur])).cpu().numpy()
    eng.set_frame_size()
    for i, f in enumerate((des, cur)):
        for k in range(4):
            assert np.array_equal(out[i, k], np.rot90(f, k))


@pytest.mark.parametrize("selection", ["best", "order"])
def test_controller_runs_every_update_through_the_search(selection):
    """``ServoParams(roll_search=True)``: camera frames are resized one by one by the stand-alone launch, the engine's frame size is
    reset, the update is ``roll_velocity`` on the resized frames, and ``best_roll`` reports the same pick."""
    from vitvs_amd import servo
    g = 14
    eng, params = ENGINES.fetch(g, "fp32")
    on = params.replace(roll_search=True)
    goal_cam, cur_cam = synth.texture(640, 5)[:480], np.ascontiguousarray(synth.texture(640, 5)[:480][::-1, ::-1])   # half a turn
    Z = ls.depth(np.random.default_rng(3))
    small = eng.resize_frames(np.stack([cur_cam, goal_cam]))
    mode = _lib.SELECT_BEST if selection == "best" else _lib.SELECT_ORDER
    v, st, info = eng.roll_velocity(small[0], small[1], Z, on.intrinsics(), mode=mode, selection=_selection(mode, g * g, 21), num_pairs=on.num_pairs)
    eng.set_frame_size(480, 640)                                  # whatever an earlier user of the engine left set
    ctl = servo.Controller(eng, goal_cam, on, selection=selection)
    ctl.generator = torch.Generator().manual_seed(21)
    ctl.image_callback_rgb(cur_cam)
    ctl.image_callback_depth(Z)
    ctl.ibvs()
    assert tuple(eng.frame_size) == (16 * g, 16 * g)
    assert ctl.last_roll == info["roll"] and ctl.last_status == int(st) and np.array_equal(ctl.last_roll_info["scores"], info["scores"], equal_nan=True)
    assert np.array_equal(ctl._raw_v, v.cpu().numpy()) and (ctl.v_c is not None) == (int(st) != _lib.STATUS_NO_CORRESPONDENCE)
    k, scores = ctl.best_roll()
    assert k == (info["roll"] if info["roll"] >= 0 else None)
    assert [None if s is None else float(s) for s in scores] == [None if np.isnan(s) else float(s) for s in info["scores"]]
    print(f"controller, selection {selection}: k* = {ctl.last_roll}, scores {scores}")


@pytest.mark.parametrize("n_iter", [0, 2])
def test_follow_on_laws_behind_a_roll_call(n_iter):
    """pose_velocity and homography_velocity (n_pairs = 1) after a roll call equal the same laws after servo_from_nn on the
    carried-back tables, bit for bit."""
    g, m = 14, 1
    eng, params = ENGINES.fetch(g, "fp32")
    rng = np.random.default_rng(40 + n_iter)
    des, cur = _frames(g, m)
    Z, K = ls.depth(rng), ls.intrinsics(rng, params)
    eng.set_goal_depth(ls.goal_depth(rng, holes=False))

    def laws(st):
        vp, pi = eng.pose_velocity(K, [st], n_iter)
        vh, hi = eng.homography_velocity(K, [st], 0.61, n_iter, consensus=64, seed=3)
        return dict(ls.host(pi), v=vp.cpu().numpy()), dict(ls.host(hi), v=vh.cpu().numpy())
    want, v, st, det = _composition(eng, g, cur, des, Z, K, _lib.SELECT_BEST, None, 48, cached=False)
    pose_a, hom_a = laws(st)
    v2, st2, info = eng.roll_velocity(cur, des, Z, K, mode=_lib.SELECT_BEST, num_pairs=48)
    pose_b, hom_b = laws(int(st2))
    _same_update(want, v, st, det, v2.cpu().numpy(), int(st2), info, eng.last_details(1), n_iter)
    assert st == _lib.STATUS_OK
    assert ls.same_values(pose_a, pose_b) and ls.same_values(hom_a, hom_b)
    assert int(pose_b["status"][0]) == _lib.STATUS_OK and int(hom_b["status"][0]) == _lib.STATUS_OK
    eng.set_goal_depth(None)
