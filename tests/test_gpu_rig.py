"""The rig law through a handle (vitvs_rig_velocity[_dev], Engine.rig_velocity, MultiController(rig=...)) against the fp64 numpy
statement of tests/rig_ref.py evaluated on the handle's OWN last_details L and e: this tests the rig stage, not the forward.
ViT-S/16 224², synthetic weights, max_pairs = 3, fp32, ORDER and EXPLICIT selections.  Bar: v_rig <= 1e-9 relative L2."""
import ctypes as C

import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib, config, servo, synth, weights
from vitvs_amd.engine import Engine, VitvsError

import rig_ref as rg
import robust_ref as rr
import law_support as ls

pytestmark = pytest.mark.gpu

KEY = "vits16_224"
N = ls.N_CAMERAS


@pytest.fixture(scope="module")
def setup():
    cfg = config.baseline_config(KEY)
    params = config.ServoParams(dino_input_size=cfg.img_size, use_feature_binning=False)
    sd = weights.synthetic_state_dict(cfg, 0)
    des, cur = synth.frame_pair(cfg.img_size, synth.ACCEPTED_FRAME_SEEDS[KEY])
    # three cameras: the accepted pair, its current frame drifting by a few pixels per camera and per round
    curs = [[np.roll(cur, shift=2 * c - 2 + r, axis=1).copy() for c in range(N)] for r in range(3)]
    depth = np.stack([np.roll(synth.depth_pattern(), 7 * c, axis=1) for c in range(N)])
    eng = Engine(cfg, params, precision="fp32", max_pairs=N).load_state_dict(sd)
    yield dict(cfg=cfg, params=params, sd=sd, des=np.stack([des] * N), curs=[np.stack(c) for c in curs], depth=depth, eng=eng,
               Ws=np.stack([servo.twist_matrix(R, t) for R, t in ls.extrinsics()]))
    eng.close()


def _reference(eng, n, Ws, status, lam):
    det = eng.last_details(n)
    rows = det["info"][:, 5]
    Ls = [det["L"][i, :6, :rows[i]].T for i in range(n)]
    es = [det["L"][i, 6, :rows[i]] for i in range(n)]
    return rg.rig_law(Ls, es, Ws[:n], status, lam), det


def test_order_selection_equals_the_reference(setup):
    s, eng = setup, setup["eng"]
    v, st = ls.rig_velocity(s)
    v_rig, rs, info = eng.rig_velocity(s["Ws"], st)
    st = st.cpu().numpy()
    assert (st == 0).all(), st                                     # (the set-up: three live cameras)
    ref, det = _reference(eng, N, s["Ws"], st, s["params"].lambda_)
    assert rs == 0 and info["cameras"] == 3 and info["rows"] == ref["rows"] == 3 * 2 * s["params"].num_pairs and info["sweeps"] == -1
    assert rg.ldlt_margin(ref["M"]) >= 100
    err = rr.rel_l2(v_rig.cpu().numpy(), ref["v_rig"])
    print(f"3 cameras, ORDER: v_rig rel err {err:.2e}")
    assert err <= 1e-9
    normal = info["normal"].cpu().numpy()
    assert np.allclose(normal, rg.normal_packed(ref["M"], ref["e"]), rtol=1e-11, atol=1e-12 * np.abs(normal).max()) and normal[27] == ref["rows"]
    # ... which is not what averaging the cameras' own twists gives
    avg = np.mean([np.linalg.solve(W, vc) for W, vc in zip(s["Ws"], v.cpu().numpy())], axis=0)
    print(f"  averaged camera twists differ from it by {rr.rel_l2(avg, ref['v_rig']):.3f} (relative)")


def test_one_camera_at_the_rig_origin_is_its_own_twist(setup):
    s, eng = setup, setup["eng"]
    v, st = ls.rig_velocity(s, n=1)
    v_rig, rs, info = eng.rig_velocity(np.eye(6)[None], st)
    assert rs == 0 and int(st[0]) == 0 and info["cameras"] == 1 and info["sweeps"] == -1
    assert rr.rel_l2(v_rig.cpu().numpy(), v.cpu().numpy()[0]) <= 1e-12


def test_explicit_selection_and_a_camera_with_too_few_features_is_excluded(setup):
    s, eng = setup, setup["eng"]
    ls.rig_velocity(s)
    tab = eng.last_tables(N)
    ids = []
    for b in range(N):
        mutual = np.nonzero(tab["nn_2"][b][tab["nn_1"][b]] == np.arange(s["cfg"].tokens))[0]
        ids.append(mutual[:12].astype(np.int32))
    for dead in (None, 1):
        sel = [ids[b] if b != dead else np.zeros(0, np.int32) for b in range(N)]
        v, st = eng.compute_velocity(s["curs"][0], s["des"], s["depth"], s["params"].intrinsics(), mode=_lib.SELECT_EXPLICIT,
                                     selection=sel, num_pairs=12)
        v_rig, rs, info = eng.rig_velocity(s["Ws"], st)
        st = st.cpu().numpy()
        assert list(st) == [0 if b != dead else _lib.STATUS_TOO_FEW for b in range(N)], st
        ref, _ = _reference(eng, N, s["Ws"], st, s["params"].lambda_)
        live = N - (dead is not None)
        assert rs == 0 and info["cameras"] == live and info["rows"] == ref["rows"] == live * 24 and info["worst_status"] == int(st.max())
        assert rr.rel_l2(v_rig.cpu().numpy(), ref["v_rig"]) <= 1e-9
    # nobody contributes: zero twist, the largest camera status
    v, st = eng.compute_velocity(s["curs"][0], s["des"], s["depth"], s["params"].intrinsics(), mode=_lib.SELECT_EXPLICIT,
                                 selection=[np.zeros(0, np.int32)] * N, num_pairs=12)
    v_rig, rs, info = eng.rig_velocity(s["Ws"], st)
    assert rs == _lib.STATUS_TOO_FEW and info["cameras"] == 0 and info["rows"] == 0 and not v_rig.cpu().numpy().any()


@pytest.mark.parametrize("option", ["interaction", "subpatch"])
def test_the_law_reads_whatever_matrix_the_camera_law_built(setup, option):
    s, eng = setup, setup["eng"]
    try:
        if option == "interaction":
            eng.set_goal_depth(np.ascontiguousarray(synth.depth_pattern()[::-1, ::-1]))
            eng.set_option("interaction", 2)
        else:
            eng.set_option("subpatch", 1)
        _, st = ls.rig_velocity(s)
        v_rig, rs, info = eng.rig_velocity(s["Ws"], st)
        st = st.cpu().numpy()
        ref, det = _reference(eng, N, s["Ws"], st, s["params"].lambda_)
        assert (st == 0).all() and rs == 0 and info["rows"] == ref["rows"] > 0
        assert (det["Z_goal"].any() if option == "interaction" else det["offsets"].any())     # the option really was on
        assert rr.rel_l2(v_rig.cpu().numpy(), ref["v_rig"]) <= 1e-9
    finally:
        eng.set_option(option, 0)
        eng.set_goal_depth(None)


def test_error_returns(setup):
    s, eng = setup, setup["eng"]
    lib = eng.lib
    fresh = Engine(s["cfg"], s["params"], precision="fp32", max_pairs=N)          # no velocity call yet (not even weights)
    with pytest.raises(VitvsError, match=r"\(-5\)"):
        fresh.rig_velocity(s["Ws"], np.zeros(N, np.int32))
    fresh.close()
    _, st = ls.rig_velocity(s)
    with pytest.raises(VitvsError, match=r"\(-5\)"):
        eng.rig_velocity(s["Ws"][:2], st[:2])                                     # not the call's pair count
    w = torch.as_tensor(s["Ws"]).reshape(N, 36).to(eng.device)
    out = torch.zeros(6, dtype=torch.float64, device=eng.device)
    rs = torch.zeros(1, dtype=torch.int32, device=eng.device)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    assert lib.vitvs_rig_velocity_dev(eng.handle, N, None, p(st), p(out), p(rs), None, None, None) == -1
    assert lib.vitvs_rig_velocity_dev(eng.handle, N, p(w), p(st), None, p(rs), None, None, None) == -1
    assert lib.vitvs_rig_velocity_dev(eng.handle, N, p(w), p(st), p(out), p(rs), None, None, None) == 0   # info and normal may be NULL
    try:
        eng.set_option("robust_law", 2)
        with pytest.raises(VitvsError, match=r"\(-5\)"):
            eng.rig_velocity(s["Ws"], st)                                         # on, before any robust evaluation
        _, st2 = ls.rig_velocity(s)
        with pytest.raises(VitvsError, match=r"\(-5\)"):
            eng.rig_velocity(s["Ws"], st2)
    finally:
        eng.set_option("robust_law", 0)
    with pytest.raises(VitvsError, match=r"\(-5\)"):
        eng.rig_velocity(s["Ws"], st)                                             # the last evaluation was still a robust one
    _, st = ls.rig_velocity(s)
    assert eng.rig_velocity(s["Ws"], st)[1] == 0


def test_under_graph_replay_with_new_frames(setup):
    s, eng = setup, setup["eng"]
    dev = eng.device
    cur = torch.as_tensor(s["curs"][0]).to(dev)
    des = torch.as_tensor(s["des"]).to(dev)
    z = torch.as_tensor(s["depth"]).to(dev)
    K = torch.tensor([s["params"].intrinsics()] * N, dtype=torch.float64, device=dev)
    order = ls.order(s["cfg"], N, 12).to(dev)
    v = torch.zeros((N, 6), dtype=torch.float64, device=dev)
    st = torch.zeros(N, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(dev)
    eng.set_option("graph_replay", 1)
    try:
        twists = []
        with torch.cuda.stream(stream):
            for r in range(3):                                                    # the capture, then two replays
                cur.copy_(torch.as_tensor(s["curs"][r]).to(dev))
                eng.compute_velocity_dev(cur, des, z, K, _lib.SELECT_ORDER, order, None, False, v, st, 0)
                v_rig, rs, info = eng.rig_velocity(s["Ws"], st)
                ref, _ = _reference(eng, N, s["Ws"], st.cpu().numpy(), s["params"].lambda_)
                assert rs == 0 and info["rows"] == ref["rows"]
                assert rr.rel_l2(v_rig.cpu().numpy(), ref["v_rig"]) <= 1e-9, r
                twists.append(v_rig.cpu().numpy())
        assert not np.array_equal(twists[0], twists[1]) and not np.array_equal(twists[1], twists[2])   # new frames, new twists
    finally:
        eng.set_option("graph_replay", 0)
        torch.cuda.synchronize()


def test_host_pointer_form_equals_the_device_form(setup):
    s, eng = setup, setup["eng"]
    _, st = ls.rig_velocity(s)
    v_rig, rs, info = eng.rig_velocity(s["Ws"], st)
    hv, hrs, hinfo, hnormal = eng.rig_velocity_host(s["Ws"], st.cpu().numpy())
    assert hrs == rs and list(hinfo[:3]) == [info["cameras"], info["rows"], info["sweeps"]]
    assert np.array_equal(hv, v_rig.cpu().numpy()) and np.array_equal(hnormal, info["normal"].cpu().numpy())
    # ... and behind a host-pointer velocity call
    order = ls.order(s["cfg"], N, 11).numpy()
    v2, st2 = eng.compute_velocity_host(s["curs"][0], s["des"], s["depth"], s["params"].intrinsics(), _lib.SELECT_ORDER, order)
    hv2, hrs2, _, _ = eng.rig_velocity_host(s["Ws"], st2)
    ref, _ = _reference(eng, N, s["Ws"], st2, s["params"].lambda_)
    assert hrs2 == 0 and rr.rel_l2(hv2, ref["v_rig"]) <= 1e-9


def _snapshot(eng, v, st):
    det = eng.last_details(N)
    return dict(det, v_c=v.cpu().numpy(), status=st.cpu().numpy())


def test_nothing_else_moves(setup):
    """v_c, status and every last_details array of a velocity call are bit-identical with and without a rig call after it, and to
    those of a fresh handle that never saw the feature."""
    s, eng = setup, setup["eng"]
    v, st = ls.rig_velocity(s)
    before = _snapshot(eng, v, st)
    eng.rig_velocity(s["Ws"], st)
    eng.rig_velocity_host(s["Ws"], st.cpu().numpy())
    after = _snapshot(eng, v, st)
    v2, st2 = ls.rig_velocity(s)                                                        # and the next velocity call after it
    again = _snapshot(eng, v2, st2)
    fresh = Engine(s["cfg"], s["params"], precision="fp32", max_pairs=N).load_state_dict(s["sd"])
    v3, st3 = ls.rig_velocity(s, eng=fresh)
    never = _snapshot(fresh, v3, st3)
    fresh.close()
    for key in before:
        for other, what in ((after, "after a rig call"), (again, "in the next call"), (never, "on a fresh handle")):
            a, b = np.asarray(before[key]), np.asarray(other[key])
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (key, what)


def test_multi_controller_with_a_rig(setup):
    s, eng = setup, setup["eng"]
    goals = [s["des"][i] for i in range(N)]
    ext = ls.extrinsics()

    def run(rig):
        mc = servo.MultiController(eng, goals, selection="order", rig=rig, generator=torch.Generator().manual_seed(4))
        raws, smooth, rigs = [], [], []
        for r in range(3):
            for c in range(N):
                mc.image_callback_rgb(c, s["curs"][r][c])
                mc.image_callback_depth(c, s["depth"][c])
            mc.ibvs()
            raws.append([np.array(c._raw_v, np.float64) for c in mc.cameras])
            smooth.append([np.array(c.v_c) for c in mc.cameras])
            if rig is not None:
                ref, _ = _reference(eng, N, s["Ws"], [c.last_status for c in mc.cameras], s["params"].lambda_)
                assert mc.rig_status == 0 and rr.rel_l2(mc.rig_velocity_raw, ref["v_rig"]) <= 1e-9
                rigs.append(mc.rig_velocity_raw.copy())
                state = [None] * 6
                for x in rigs:
                    want = servo.ema_update(state, x, s["params"].ema_alpha)
                assert np.array_equal(mc.v_rig, want)
        return raws, smooth, mc

    with_rig = run(ext)
    without = run(None)
    assert without[2].v_rig is None and without[2].rig_velocity_raw is None
    for a, b in ((with_rig[0], without[0]), (with_rig[1], without[1])):
        assert all(np.array_equal(x, y) for ra, rb in zip(a, b) for x, y in zip(ra, rb))
    with pytest.raises(ValueError):
        servo.MultiController(eng, goals, rig=ext[:2])


def test_multi_controller_rig_needs_the_engine_backend(setup):
    from vitvs_amd.pipeline import UpdatePipeline
    s = setup
    pipe = UpdatePipeline(s["cfg"], s["params"], s["sd"], precision="fp32", depth=2)
    try:
        with pytest.raises(ValueError, match="Engine backend"):
            servo.MultiController(pipe, [s["des"][i] for i in range(N)], rig=ls.extrinsics())
    finally:
        pipe.close()
