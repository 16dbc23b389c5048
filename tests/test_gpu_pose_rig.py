"""The pose rig law through a handle (vitvs_pose_rig_velocity[_dev], Engine.pose_rig_velocity, MultiController(law="pose", rig=...);
DESIGN.md §5g) against the fp64 numpy statement of tests/pose_rig_ref.py evaluated on what the handle's OWN velocity call left
(``Engine.last_details``' selected / s_uv / feat / info) and the goal-depth table restated on the host: this tests the rig stage,
not the forward.  ViT-S/16 224², synthetic weights, max_pairs = 3, fp32.  Bars as at the kernel's seam: v_rig, R, t, weights <=
1e-9, sigma <= 1e-12, moments <= 1e-12 of their largest, status and rig_info exact; every reference solve keeps a relative
eigen-gap >= 1e-6 and every residual stays >= 1e-6 off the rejection edge (asserted on the CPU side of each comparison)."""
import ctypes as C

import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib, config, servo, synth, weights
from vitvs_amd.engine import Engine, VitvsError

import pose_rig_ref as rr
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
    curs = [[np.roll(cur, shift=2 * c - 2 + r, axis=1).copy() for c in range(N)] for r in range(3)]
    depth = np.stack([np.roll(synth.depth_pattern(), 7 * c, axis=1) for c in range(N)])
    eng = Engine(cfg, params, precision="fp32", max_pairs=N).load_state_dict(sd)
    rng = np.random.default_rng(3)
    rig = rr.seeded_rig(rng, N)
    goals = np.stack([ls.goal_depth_of(s) for s in range(N)])
    yield dict(cfg=cfg, params=params, sd=sd, des=np.stack([des] * N), curs=[np.stack(c) for c in curs], depth=depth, eng=eng,
               rig=rig, goals=goals, tables=np.stack([ls.goal_table(z, cfg.grid, cfg.img_size, params) for z in goals]),
               pitches=(cfg.stride * params.u_max / cfg.img_size, cfg.stride * params.v_max / cfg.img_size),
               K=np.array([params.intrinsics()] * N))
    eng.close()


def _reference(s, det, status, n_iter, tables, rig=None, K=None, degenerate=False):
    with np.errstate(all="ignore"):
        ref = rr.pose_rig_from_details(det, status, rig or s["rig"], s["K"] if K is None else K, tables, s["params"].lambda_, n_iter,
                                       *s["pitches"])
    if not degenerate:
        assert all(g >= 1e-6 for g in ref["gaps"]) and ref["edge"] >= 1e-6, ("choose other inputs", ref["gaps"], ref["edge"])
    return ref


def _host(x):
    return x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def _compare(v, rs, info, ref, what):
    assert rs == ref["status"], (what, rs, ref["status"])
    got = [int(info[name]) for name in Engine.POSE_RIG_INFO_FIELDS]
    assert got == list(ref["info"]), (what, got, ref["info"])
    errs = dict(v=np.abs(_host(v) - ref["v"]).max(), R=np.abs(_host(info["R"]) - ref["R"]).max(),
                t=np.abs(_host(info["t"]) - ref["t"]).max(), weights=np.abs(_host(info["weights"]) - ref["weights"]).max())
    print(f"{what}: " + ", ".join(f"{k} {e:.1e}" for k, e in errs.items()) + f", gaps {['%.1e' % g for g in ref['gaps']]}")
    assert all(e <= 1e-9 for e in errs.values()), (what, errs)
    assert abs(float(_host(info["sigma"]).reshape(-1)[0]) - ref["sigma"]) <= 1e-12, what
    m = _host(info["moments"])
    assert np.abs(m - ref["moments"]).max() <= 1e-12 * max(np.abs(ref["moments"]).max(), 1e-300), what


def _snapshot(eng, v, st):
    det = eng.last_details(N)
    return dict(det, v_c=_host(v).copy(), status=_host(st).copy())


def _same(a, b):
    return sorted(a) == sorted(b) and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)


@pytest.mark.parametrize("per_camera", [False, True])
def test_device_equals_the_reference_and_leaves_the_call_untouched(setup, per_camera):
    """One goal depth for all cameras, or one per camera; N = 0 and 4; the host-pointer form is the same launch; v_c, every
    vitvs_last_* output and the pose law's own results are what they were."""
    s, eng = setup, setup["eng"]
    eng.set_goal_depth(s["goals"] if per_camera else s["goals"][0])
    tables = s["tables"] if per_camera else s["tables"][:1]
    try:
        v_c, st = ls.rig_velocity(s)
        assert not st.cpu().numpy().any()
        before = _snapshot(eng, v_c, st)
        pose_before = eng.pose_velocity_host(s["params"].intrinsics(), before["status"], 4)
        holes = 0
        for n_iter in (0, 4):
            v, rs, info = eng.pose_rig_velocity(s["rig"], s["params"].intrinsics(), st, n_iter)
            ref = _reference(s, before, before["status"], n_iter, tables)
            _compare(v, rs, info, ref, f"per camera {per_camera}, N = {n_iter}")
            assert rs == 0 and info["cameras"] == N
            holes = info["holes"]
            hv, hrs, hinfo = eng.pose_rig_velocity_host(s["rig"], s["params"].intrinsics(), before["status"], n_iter)
            assert hrs == rs and np.array_equal(hv, v.cpu().numpy())
            for key, val in info.items():
                assert np.array_equal(_host(val).reshape(-1), np.asarray(hinfo[key]).reshape(-1)), key
        assert holes > 0                                            # the depth images have holes: some rows are dropped
        assert _same(_snapshot(eng, v_c, st), before)
        pose_after = eng.pose_velocity_host(s["params"].intrinsics(), before["status"], 4)
        assert np.array_equal(pose_before[0], pose_after[0]) and _same(pose_before[1], pose_after[1])
    finally:
        eng.set_goal_depth(None)


def test_a_camera_with_too_few_features_and_nobody(setup):
    s, eng = setup, setup["eng"]
    eng.set_goal_depth(s["goals"])
    try:
        ls.rig_velocity(s)
        tab = eng.last_tables(N)
        ids = []
        for b in range(N):
            mutual = np.nonzero(tab["nn_2"][b][tab["nn_1"][b]] == np.arange(s["cfg"].tokens))[0]
            ids.append(mutual[:12].astype(np.int32))
        for dead in (None, 1):
            sel = [ids[b] if b != dead else np.zeros(0, np.int32) for b in range(N)]
            v_c, st = eng.compute_velocity(s["curs"][0], s["des"], s["depth"], s["params"].intrinsics(), mode=_lib.SELECT_EXPLICIT,
                                           selection=sel, num_pairs=12)
            sth = st.cpu().numpy()
            assert list(sth) == [0 if b != dead else _lib.STATUS_TOO_FEW for b in range(N)], sth
            det = eng.last_details(N)
            for n_iter in (0, 4):
                v, rs, info = eng.pose_rig_velocity(s["rig"], s["params"].intrinsics(), st, n_iter)
                _compare(v, rs, info, _reference(s, det, sth, n_iter, s["tables"]), f"dead {dead}, N = {n_iter}")
                assert info["cameras"] == N - (dead is not None) and info["worst_status"] == int(sth.max())
                if dead is not None:
                    assert not info["weights"][dead].cpu().numpy().any()
        v_c, st = eng.compute_velocity(s["curs"][0], s["des"], s["depth"], s["params"].intrinsics(), mode=_lib.SELECT_EXPLICIT,
                                       selection=[np.zeros(0, np.int32)] * N, num_pairs=12)
        v, rs, info = eng.pose_rig_velocity(s["rig"], s["params"].intrinsics(), st, 4)
        assert rs == _lib.STATUS_TOO_FEW and info["cameras"] == 0 and info["usable"] == 0 and not v.cpu().numpy().any()
        assert np.array_equal(info["R"].cpu().numpy(), np.eye(3)) and not info["moments"].cpu().numpy().any()
    finally:
        eng.set_goal_depth(None)


@pytest.mark.parametrize("option", ["subpatch", "interaction", "robust_law"])
def test_with_the_other_law_options(setup, option):
    s, eng = setup, setup["eng"]
    eng.set_goal_depth(s["goals"])
    try:
        eng.set_option(option, {"subpatch": 1, "interaction": 2, "robust_law": 4}[option])
        v_c, st = ls.rig_velocity(s)
        sth = st.cpu().numpy()
        assert not sth.any()
        det = eng.last_details(N)
        if option == "subpatch":
            assert det["offsets"].any()
        for n_iter in (0, 4):
            v, rs, info = eng.pose_rig_velocity(s["rig"], s["params"].intrinsics(), st, n_iter)
            _compare(v, rs, info, _reference(s, det, sth, n_iter, s["tables"]), f"{option}, N = {n_iter}")
    finally:
        eng.set_option(option, 0)
        eng.set_goal_depth(None)


def test_error_returns(setup):
    s, eng = setup, setup["eng"]
    K = s["params"].intrinsics()
    fresh = Engine(s["cfg"], s["params"], precision="fp32", max_pairs=N)          # no velocity call yet (not even weights)
    with pytest.raises(VitvsError, match=r"\(-5\)"):
        fresh.pose_rig_velocity(s["rig"], K, np.zeros(N, np.int32))
    fresh.close()
    try:
        eng.set_goal_depth(None)
        _, st = ls.rig_velocity(s)
        with pytest.raises(VitvsError, match=r"\(-5\)"):           # no goal depth
            eng.pose_rig_velocity(s["rig"], K, st)
        with pytest.raises(VitvsError, match=r"\(-5\)"):
            eng.pose_rig_velocity_host(s["rig"], K, st.cpu().numpy())
        eng.set_goal_depth(s["goals"][:2])
        with pytest.raises(VitvsError, match=r"\(-5\)"):           # two goal images, three cameras
            eng.pose_rig_velocity(s["rig"], K, st)
        eng.set_goal_depth(s["goals"][0])
        with pytest.raises(VitvsError, match=r"\(-5\)"):           # not the call's pair count
            eng.pose_rig_velocity(s["rig"][:2], K, st[:2])
        eng.set_option("interaction", 1)
        _, st = ls.rig_velocity(s)
        with pytest.raises(VitvsError, match=r"\(-5\)"):           # feat holds Z*, not Z
            eng.pose_rig_velocity(s["rig"], K, st)
        eng.set_option("interaction", 0)
        _, st = ls.rig_velocity(s)
        v, rs, info = eng.pose_rig_velocity(s["rig"], K, st)
        assert rs == 0
        # the C entry points' own checks
        dev = eng.device
        rd = torch.from_numpy(rr.rtc_rows(s["rig"])).to(dev)
        kd = torch.tensor([K] * N, dtype=torch.float64, device=dev)
        out, ps = torch.zeros(6, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
        f = eng.lib.vitvs_pose_rig_velocity_dev
        tail = (None,) * 6
        assert f(eng.handle, N, p(rd), p(kd), p(st), 0, p(out), p(ps), *tail) == 0          # NULL optional outputs
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), v.cpu().numpy()) and int(ps.cpu()[0]) == 0
        for n_iter in (-1, 17):
            assert f(eng.handle, N, p(rd), p(kd), p(st), n_iter, p(out), p(ps), *tail) == -2
        assert f(eng.handle, 0, p(rd), p(kd), p(st), 0, p(out), p(ps), *tail) == -2
        assert f(eng.handle, N, None, p(kd), p(st), 0, p(out), p(ps), *tail) == -1
        assert f(eng.handle, N, p(rd), None, p(st), 0, p(out), p(ps), *tail) == -1
        assert f(eng.handle, N, p(rd), p(kd), None, 0, p(out), p(ps), *tail) == -1
        assert f(eng.handle, N, p(rd), p(kd), p(st), 0, None, p(ps), *tail) == -1
        assert f(eng.handle, N, p(rd), p(kd), p(st), 0, p(out), None, *tail) == -1
    finally:
        eng.set_option("interaction", 0)
        eng.set_goal_depth(None)


def test_under_graph_replay_with_new_frames(setup):
    s, eng = setup, setup["eng"]
    dev = eng.device
    eng.set_goal_depth(s["goals"])
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
                v_rig, rs, info = eng.pose_rig_velocity(s["rig"], s["params"].intrinsics(), st, 4)
                ref = _reference(s, eng.last_details(N), st.cpu().numpy(), 4, s["tables"])
                _compare(v_rig, rs, info, ref, f"round {r}")
                twists.append(v_rig.cpu().numpy())
        assert not np.array_equal(twists[0], twists[1]) and not np.array_equal(twists[1], twists[2])   # new frames, new twists
    finally:
        eng.set_option("graph_replay", 0)
        torch.cuda.synchronize()
        eng.set_goal_depth(None)


def test_multi_controller_with_the_pose_law(setup):
    """law="pose" with rig=: the cameras' raw and smoothed v_c are those of the controller without it, bit for bit; the rig's twist
    is the reference's on what each round left; a partial round re-pairs the per-camera goal depths with the live cameras."""
    s, eng = setup, setup["eng"]
    goals = [s["des"][i] for i in range(N)]
    pose = s["params"].replace(law="pose", rig_pose_robust_iterations=4)

    def run(with_pose):
        kw = dict(params=pose, rig=s["rig"], goal_depth=s["goals"]) if with_pose else {}
        mc = servo.MultiController(eng, goals, selection="order", generator=torch.Generator().manual_seed(4), **kw)
        raws, smooth, rigs = [], [], []
        for r in range(4):
            live = [0, 2] if r == 2 else list(range(N))                           # round 2: camera 1 has no image
            for c in range(N):
                mc.cameras[c].latest_image = None
            for c in live:
                mc.image_callback_rgb(c, s["curs"][r % 3][c])
                mc.image_callback_depth(c, s["depth"][c])
            mc.ibvs()
            raws.append([np.array(mc.cameras[c]._raw_v, np.float64) for c in live])
            smooth.append([np.array(mc.cameras[c].v_c) for c in live])
            if with_pose:
                det = eng.last_details(len(live))
                ref = _reference(s, det, [mc.cameras[c].last_status for c in live], 4, s["tables"][live],
                                 rig=[s["rig"][c] for c in live], K=s["K"][live])
                assert mc.rig_status == ref["status"] == 0 and mc.rig_info["cameras"] == len(live)
                assert np.abs(mc.rig_velocity_raw - ref["v"]).max() <= 1e-9
                assert np.abs(mc.rig_pose[0] - ref["R"]).max() <= 1e-9 and np.abs(mc.rig_pose[1] - ref["t"]).max() <= 1e-9
                assert np.abs(mc.rig_weights[live] - ref["weights"]).max() <= 1e-9
                assert all(not mc.rig_weights[c].any() for c in range(N) if c not in live)
                rigs.append(mc.rig_velocity_raw.copy())
                state = [None] * 6
                for x in rigs:
                    want = servo.ema_update(state, x, s["params"].ema_alpha)
                assert np.array_equal(mc.v_rig, want)
        return raws, smooth, mc

    try:
        with_pose = run(True)
        eng.set_goal_depth(None)
        without = run(False)
        assert without[2].v_rig is None and without[2].rig_pose is None
        for a, b in ((with_pose[0], without[0]), (with_pose[1], without[1])):
            assert all(np.array_equal(x, y) for ra, rb_ in zip(a, b) for x, y in zip(ra, rb_))
    finally:
        eng.set_goal_depth(None)
