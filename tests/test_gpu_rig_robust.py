"""The robust rig law through a handle (vitvs_rig_robust_velocity[_dev], Engine.rig_velocity(robust_iterations=N),
MultiController(rig=..., rig_robust_iterations)) against the fp64 numpy statement of tests/rig_robust_ref.py evaluated on the
handle's OWN last_details L, e, rows and matched pairs: this tests the rig stage, not the forward.  The set-up of
tests/test_gpu_rig.py (its shared helpers are in tests/law_support.py): ViT-S/16 224², synthetic weights, max_pairs = 3, fp32.
Bar: v_rig <= 1e-9."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib, config, servo, synth, weights
from vitvs_amd.engine import Engine, VitvsError

import rig_robust_ref as rr
import robust_ref
import law_support as ls

pytestmark = pytest.mark.gpu

KEY = "vits16_224"
N = ls.N_CAMERAS
ITER = 4


@pytest.fixture(scope="module")
def setup():
    cfg = config.baseline_config(KEY)
    params = config.ServoParams(dino_input_size=cfg.img_size, use_feature_binning=False)
    sd = weights.synthetic_state_dict(cfg, 0)
    des, cur = synth.frame_pair(cfg.img_size, synth.ACCEPTED_FRAME_SEEDS[KEY])
    curs = [[np.roll(cur, shift=2 * c - 2 + r, axis=1).copy() for c in range(N)] for r in range(3)]
    depth = np.stack([np.roll(synth.depth_pattern(), 7 * c, axis=1) for c in range(N)])
    eng = Engine(cfg, params, precision="fp32", max_pairs=N).load_state_dict(sd)
    K = np.array([params.intrinsics()] * N)
    yield dict(cfg=cfg, params=params, sd=sd, des=np.stack([des] * N), curs=[np.stack(c) for c in curs], depth=depth, eng=eng, K=K,
               Ws=np.stack([servo.twist_matrix(R, t) for R, t in ls.extrinsics()]))
    eng.close()


def _smin(s, K, contributing):
    p, cfg = s["params"], s["cfg"]
    return max([robust_ref.sigma_min(cfg.stride, p.u_max, p.v_max, cfg.img_size, K[i][0], K[i][1]) for i in contributing] or [0.0])


def _reference(s, eng, n, status, K, n_iter=ITER):
    det = eng.last_details(n)
    rows, lives = det["info"][:, 5], det["info"][:, 3]
    Ls = [det["L"][i, :6, :rows[i]].T for i in range(n)]
    es = [det["L"][i, 6, :rows[i]] for i in range(n)]
    con = rr.contributing(Ls, status, lives)
    smin = _smin(s, K, [i for i, (r, _) in enumerate(con) if r])
    v, w, _, sigma, n_zero, margin, M, _ = rr.robust_rig_law(Ls, es, s["Ws"][:n], status, lives, s["params"].lambda_, n_iter, smin)
    return dict(v=v, w=rr.camera_weights(w, Ls, status, lives, eng.max_rows), sigma=sigma, n_zero=n_zero, margin=margin, rows=M.shape[0],
                cameras=sum(1 for r, _ in con if r), smin=smin)


def _check(got, ref, n_iter=ITER):
    v_rig, rs, info = got
    assert ref["margin"] >= 1e-6                                                   # (no weight on the rejection edge)
    assert rs == 0 and (info["cameras"], info["rows"], info["reweighted"], info["zero_weights"]) == \
        (ref["cameras"], ref["rows"], n_iter, ref["n_zero"]), (info, ref)
    assert robust_ref.rel_l2(v_rig.cpu().numpy(), ref["v"]) <= 1e-9
    assert np.abs(info["weights"].cpu().numpy() - ref["w"]).max() <= 1e-9
    assert abs(info["sigma"] - ref["sigma"]) <= 1e-12 * ref["sigma"]


def _snapshot(eng, v, st):
    return dict(eng.last_details(N), v_c=v.cpu().numpy(), status=st.cpu().numpy(), weights=eng.last_weights(N))


def _same(a, b):
    for key in a:
        x, y = np.asarray(a[key]), np.asarray(b[key])
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), key


@pytest.mark.parametrize("robust_law", [0, 2])
def test_order_selection_equals_the_reference_and_nothing_else_moves(setup, robust_law):
    s, eng = setup, setup["eng"]
    try:
        eng.set_option("robust_law", robust_law)
        v, st = ls.rig_velocity(s)
        before = _snapshot(eng, v, st)
        got = eng.rig_velocity(s["Ws"], st, robust_iterations=ITER, K=s["K"])
        stn = st.cpu().numpy()
        assert (stn == 0).all(), stn
        ref = _reference(s, eng, N, stn, s["K"])
        _check(got, ref)
        assert got[2]["cameras"] == 3 and got[2]["rows"] == 3 * 2 * s["params"].num_pairs
        print(f"3 cameras, ORDER, robust_law {robust_law}: sigma {got[2]['sigma']:.4g} (floor {ref['smin']:.4g}), "
              f"{got[2]['zero_weights']} zero weights, v_rig rel err {robust_ref.rel_l2(got[0].cpu().numpy(), ref['v']):.2e}")
        _same(before, _snapshot(eng, v, st))                                      # v_c, statuses, details and the cameras' own weights
        if robust_law:
            with pytest.raises(VitvsError, match=r"\(-5\)"):
                eng.rig_velocity(s["Ws"], st)                                     # the plain rig law still refuses
            assert int(eng.last_features(N)["info"][0, 6]) == robust_law          # (the cameras' laws really were robust)
    finally:
        eng.set_option("robust_law", 0)
        ls.rig_velocity(s)


def test_one_iteration_and_sixteen_and_cameras_with_their_own_intrinsics(setup):
    s, eng = setup, setup["eng"]
    _, st = ls.rig_velocity(s)
    stn = st.cpu().numpy()
    for n_iter in (1, 16):
        _check(eng.rig_velocity(s["Ws"], st, robust_iterations=n_iter, K=s["K"]), _reference(s, eng, N, stn, s["K"], n_iter), n_iter)
    K = s["K"].copy()
    K[1, :2] *= 0.05                                                              # camera 1 sets the floor: sigma_min is the largest
    ref = _reference(s, eng, N, stn, K)
    assert ref["smin"] == pytest.approx(20 * _smin(s, s["K"], [0])) and ref["sigma"] == ref["smin"]
    _check(eng.rig_velocity(s["Ws"], st, robust_iterations=ITER, K=K), ref)
    one = eng.rig_velocity(s["Ws"], st, robust_iterations=ITER, K=s["params"].intrinsics())       # one (fx, fy, cx, cy) for all
    _check(one, _reference(s, eng, N, stn, s["K"]))


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
        got = eng.rig_velocity(s["Ws"], st, robust_iterations=ITER, K=s["K"])
        st = st.cpu().numpy()
        assert list(st) == [0 if b != dead else _lib.STATUS_TOO_FEW for b in range(N)], st
        ref = _reference(s, eng, N, st, s["K"])
        live = N - (dead is not None)
        assert ref["cameras"] == live and ref["rows"] == live * 24 and got[2]["worst_status"] == int(st.max())
        _check(got, ref)
        if dead is not None:
            assert not got[2]["weights"][dead].any()
    v, st = eng.compute_velocity(s["curs"][0], s["des"], s["depth"], s["params"].intrinsics(), mode=_lib.SELECT_EXPLICIT,
                                 selection=[np.zeros(0, np.int32)] * N, num_pairs=12)
    v_rig, rs, info = eng.rig_velocity(s["Ws"], st, robust_iterations=ITER, K=s["K"])
    assert rs == _lib.STATUS_TOO_FEW and info["cameras"] == 0 and info["rows"] == 0 and not v_rig.cpu().numpy().any()
    assert info["reweighted"] == 0 and info["sigma"] == 0.0 and not info["weights"].any()


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
        got = eng.rig_velocity(s["Ws"], st, robust_iterations=ITER, K=s["K"])
        st = st.cpu().numpy()
        det = eng.last_details(N)
        assert (st == 0).all() and (det["Z_goal"].any() if option == "interaction" else det["offsets"].any())
        _check(got, _reference(s, eng, N, st, s["K"]))
    finally:
        eng.set_option(option, 0)
        eng.set_goal_depth(None)


def test_host_pointer_form_equals_the_device_form(setup):
    s, eng = setup, setup["eng"]
    _, st = ls.rig_velocity(s)
    v_rig, rs, info = eng.rig_velocity(s["Ws"], st, robust_iterations=ITER, K=s["K"])
    hv, hrs, hinfo, hnormal, hw, hsigma = eng.rig_velocity_host(s["Ws"], st.cpu().numpy(), robust_iterations=ITER, K=s["K"])
    assert hrs == rs and list(hinfo[:3]) == [info["cameras"], info["rows"], info["sweeps"]]
    assert list(hinfo[5:7]) == [info["reweighted"], info["zero_weights"]] and hsigma == info["sigma"]
    assert np.array_equal(hv, v_rig.cpu().numpy()) and np.array_equal(hnormal, info["normal"].cpu().numpy())
    assert np.array_equal(hw, info["weights"].cpu().numpy())
    order = ls.order(s["cfg"], N, 11).numpy()
    v2, st2 = eng.compute_velocity_host(s["curs"][0], s["des"], s["depth"], s["params"].intrinsics(), _lib.SELECT_ORDER, order)
    hv2, hrs2, _, _, hw2, _ = eng.rig_velocity_host(s["Ws"], st2, robust_iterations=ITER, K=s["K"])
    ref = _reference(s, eng, N, st2, s["K"])
    assert hrs2 == 0 and robust_ref.rel_l2(hv2, ref["v"]) <= 1e-9 and np.abs(hw2 - ref["w"]).max() <= 1e-9


def test_under_graph_replay_with_new_frames(setup):
    s, eng = setup, setup["eng"]
    dev = eng.device
    cur = torch.as_tensor(s["curs"][0]).to(dev)
    des = torch.as_tensor(s["des"]).to(dev)
    z = torch.as_tensor(s["depth"]).to(dev)
    K = torch.tensor(s["K"], dtype=torch.float64, device=dev)
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
                got = eng.rig_velocity(s["Ws"], st, robust_iterations=ITER, K=s["K"])
                _check(got, _reference(s, eng, N, st.cpu().numpy(), s["K"]))
                twists.append(got[0].cpu().numpy())
        assert not np.array_equal(twists[0], twists[1]) and not np.array_equal(twists[1], twists[2])
    finally:
        eng.set_option("graph_replay", 0)
        torch.cuda.synchronize()


def test_error_returns(setup):
    s, eng = setup, setup["eng"]
    lib = eng.lib
    fresh = Engine(s["cfg"], s["params"], precision="fp32", max_pairs=N)          # no velocity call yet
    with pytest.raises(VitvsError, match=r"\(-5\)"):
        fresh.rig_velocity(s["Ws"], np.zeros(N, np.int32), robust_iterations=ITER, K=s["K"])
    fresh.close()
    _, st = ls.rig_velocity(s)
    with pytest.raises(VitvsError, match=r"\(-5\)"):
        eng.rig_velocity(s["Ws"][:2], st[:2], robust_iterations=ITER, K=s["K"][:2])   # not the call's pair count
    w = torch.as_tensor(s["Ws"]).reshape(N, 36).to(eng.device)
    k = torch.as_tensor(s["K"]).to(eng.device)
    out = torch.zeros(6, dtype=torch.float64, device=eng.device)
    rs = torch.zeros(1, dtype=torch.int32, device=eng.device)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    f = lambda W=p(w), K=p(k), n_iter=ITER, v=p(out): \
        lib.vitvs_rig_robust_velocity_dev(eng.handle, N, W, p(st), K, n_iter, v, p(rs), None, None, None, None, None)  # noqa: E731
    assert f(W=None) == -1 and f(K=None) == -1 and f(v=None) == -1
    assert f(n_iter=0) == -2 and f(n_iter=17) == -2
    assert f() == 0                                                               # every optional output may be NULL
    torch.cuda.synchronize()
    ref = _reference(s, eng, N, st.cpu().numpy(), s["K"])
    assert int(rs[0]) == 0 and robust_ref.rel_l2(out.cpu().numpy(), ref["v"]) <= 1e-9


def test_multi_controller_with_a_robust_rig(setup):
    s, eng = setup, setup["eng"]
    goals = [s["des"][i] for i in range(N)]
    ext = ls.extrinsics()

    def run(n_iter):
        params = dataclasses.replace(s["params"], rig_robust_iterations=n_iter) if n_iter is not None else None
        mc = servo.MultiController(eng, goals, params=params, selection="order", rig=ext, generator=torch.Generator().manual_seed(4))
        raws, smooth, rigs = [], [], []
        for r in range(3):
            for c in range(N):
                mc.image_callback_rgb(c, s["curs"][r][c])
                mc.image_callback_depth(c, s["depth"][c])
            mc.ibvs()
            raws.append([np.array(c._raw_v, np.float64) for c in mc.cameras])
            smooth.append([np.array(c.v_c) for c in mc.cameras])
            rigs.append((mc.rig_velocity_raw.copy(), mc.v_rig.copy()))
            if n_iter:
                ref = _reference(s, eng, N, [c.last_status for c in mc.cameras], s["K"], n_iter)
                assert mc.rig_status == 0 and robust_ref.rel_l2(mc.rig_velocity_raw, ref["v"]) <= 1e-9
                assert mc.rig_weights.shape == (N, eng.max_rows) and np.abs(mc.rig_weights - ref["w"]).max() <= 1e-9
                assert mc.rig_info["reweighted"] == n_iter
        return raws, smooth, rigs, mc

    robust = run(ITER)
    zero = run(0)
    today = run(None)                                                             # the controller as it is without the field
    assert zero[3].rig_weights is None and today[3].rig_weights is None
    for a, b in zip(zero[:3], today[:3]):                                         # field 0: today's controller, bit for bit
        assert all(np.array_equal(x, y) for ra, rb in zip(a, b) for x, y in zip(ra, rb))
    for a, b in ((robust[0], today[0]), (robust[1], today[1])):                   # the cameras' own state is untouched
        assert all(np.array_equal(x, y) for ra, rb in zip(a, b) for x, y in zip(ra, rb))
    assert not np.array_equal(robust[2][0][0], today[2][0][0])                    # (and the rig twist is another law's)
