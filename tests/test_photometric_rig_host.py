"""The photometric rig law away from the GPU: the Python layer's refusals and the MultiController's hand-over on a
fake engine, the new symbols, and tests/photometric_rig_ref.py itself, the fp64 reference the device tests compare with: its
identity with the robust photometric reference for one camera, its statuses, and closed loops on tests/photometric_rig_scene.py.

The closed loops (30 updates, level 2, "desired" with each camera's goal depth, mu 0.01, lambda 0.5, three cameras under three
lightings, 60 % of camera 0 covered), as measured when this test was written:
  stacked, one median over all cameras' residuals, N = 4   ends at 0.0497 cm / 0.0400 deg, never above its start; camera 0 has
                                                           85.7 % of its rows at weight 0; gains 0.900 / 1.048 on cameras 1, 2
  stacked, each camera's own median (scale="camera")       ends at 10.5430 cm / 7.7464 deg
  the three robust one-camera laws, rig twists averaged    ends at 10.3643 cm / 8.0813 deg
  stacked, no illumination, N = 0                          ends at 14.8664 cm / 12.1421 deg
The first must end below 0.1 cm / 0.1 deg, each of the others above the 1.5 cm start.  (The prototype these bars come from solved
with numpy.linalg.solve and ended at 0.050 / 10.5 / 10.4 / 14.9 cm.)  On clean frames (the lightings, no occluder) the stacked law
ends at 0.0305 cm / 0.0268 deg and the average at 0.0278 cm / 0.0243 deg: both at the goal, neither ahead by more than the
other's last step."""
import os
import types

import numpy as np
import pytest

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib, config, servo, synth
import photometric_ref as pr
import photometric_robust_ref as rr
import photometric_rig_ref as rg
import photometric_rig_scene as rs
import closed_loop as cl
from planar_sim import PlanarScene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = config.ServoParams(dino_input_size=224, use_feature_binning=False)
K = PARAMS.intrinsics()


# ---------------------------------------------------------------------------------------------- (a) refusals and the hand-over
class _FakeTwist:
    def __init__(self, v):
        self.v = np.asarray(v, np.float64)

    def cpu(self):
        return self

    def numpy(self):
        return self.v


def _fake_engine(params, calls, status=0):
    def rig_law(*a):
        calls.append(a)
        n = len(a[0])
        return _FakeTwist([0.01, 0, 0, 0, 0, 0.02]), dict(status=status, cost=2.0, n=7 * n, gain=np.full(n, 1.1), bias=np.full(n, 3.0),
                                                           sigma=np.full(n, 1.5), weight=np.full(n, 35.0))
    return types.SimpleNamespace(params=params, cfg=types.SimpleNamespace(img_size=224), apply_law_params=lambda p: None, max_pairs=4,
                                 set_goal_depth=lambda z: None, device="cpu", photometric_rig_velocity=rig_law)


RIG2 = [(np.eye(3), np.array([-0.1, 0.0, 0.0])), (np.eye(3), np.array([0.1, 0.0, 0.0]))]
SMALL = dict(photometric_handover=0.02, lambda_=0.03, u_max=32, v_max=24, homography_depth=0.6)


def test_the_refusals_each_with_its_reason():
    from vitvs_amd import pipeline
    on = config.ServoParams(**SMALL)
    goal = np.zeros((24, 32, 3), np.uint8)
    with pytest.raises(ValueError, match="rig="):                                  # no rig
        servo.MultiController(_fake_engine(on, []), [goal, goal], params=on)
    pipe = pipeline.UpdatePipeline.__new__(pipeline.UpdatePipeline)               # a pipeline backend, with and without rig=
    pipe.engines = [_fake_engine(on, [])]
    with pytest.raises(ValueError, match="Engine backend"):
        servo.MultiController(pipe, [goal, goal], params=on)
    with pytest.raises(ValueError, match="Engine backend"):
        servo.MultiController(pipe, [goal, goal], params=on, rig=RIG2)
    rolled = config.ServoParams(roll_search=True)
    object.__setattr__(rolled, "photometric_handover", 0.02)
    with pytest.raises(ValueError, match="roll_search"):
        servo.MultiController(_fake_engine(rolled, []), [goal, goal], params=rolled, rig=RIG2)
    with pytest.raises(ValueError, match="v_max x u_max"):                         # a goal the law could never be handed
        servo.MultiController(_fake_engine(on, []), [goal, np.zeros((48, 64, 3), np.uint8)], params=on, rig=RIG2)
    mc = servo.MultiController(_fake_engine(on, []), [goal, goal], params=on, rig=RIG2)
    assert mc.photometric_active is False and mc.last_photometric is None
    off = config.ServoParams(u_max=32, v_max=24)                                   # the parameter at 0: nothing of it anywhere
    mc = servo.MultiController(_fake_engine(off, []), [goal, np.zeros((48, 64, 3), np.uint8)], params=off)
    assert mc.photometric_active is False


def _controller(calls, status=0, goal_depth=None, **extra):
    p = config.ServoParams(**dict(SMALL, **extra))
    goal = np.zeros((24, 32, 3), np.uint8)
    mc = servo.MultiController(_fake_engine(p, calls, status), [goal, goal + 1, goal + 2], params=p, goal_depth=goal_depth,
                               rig=RIG2 + [(np.eye(3), np.zeros(3))])
    return mc, p


def test_the_hand_over_criterion():
    """max |raw rig twist| / lambda_ against the threshold, behind a round whose rig status is OK."""
    def after(raw, status):
        mc, _ = _controller([])
        for i in range(3):
            mc.image_callback_rgb(i, np.zeros((24, 32, 3), np.uint8))
        mc.rig_velocity_raw, mc.rig_status = np.asarray(raw, np.float64), status
        mc._watch_handover([0, 1, 2])
        return mc.photometric_active

    assert after([0, 0, 0, 0, 0, 0.03 * 0.0199], _lib.STATUS_OK)
    assert not after([0, 0, 0, 0, 0, 0.03 * 0.0201], _lib.STATUS_OK)
    assert not after([0, -0.03 * 0.0201, 0, 0, 0, 0], _lib.STATUS_OK)
    assert after(np.zeros(6), _lib.STATUS_OK)
    assert not after(np.zeros(6), _lib.STATUS_TOO_FEW)
    mc, _ = _controller([])                                                        # a frame of another size: no hand-over
    for i in range(3):
        mc.image_callback_rgb(i, np.zeros((48, 64, 3), np.uint8))
    mc.rig_velocity_raw, mc.rig_status = np.zeros(6), _lib.STATUS_OK
    mc._watch_handover([0, 1, 2])
    assert mc.photometric_active is False


def test_a_photometric_round_calls_the_rig_law_on_the_live_cameras():
    depth = np.full((3, 24, 32), 600, np.uint16)
    depth[1, :, :16] = 0                                                           # camera 1: holes over its left half
    calls = []
    mc, p = _controller(calls, goal_depth=depth, photometric_illumination=True, photometric_robust_iterations=3,
                        photometric_sigma_min=0.5, photometric_level=1, ema_alpha=0.5)
    mc.image_callback_rgb(0, np.full((24, 32, 3), 5, np.uint8))
    mc.image_callback_rgb(2, np.full((24, 32, 3), 7, np.uint8))                    # camera 1 has no image: not live
    mc.photometric_active = True
    assert mc.ibvs() is None and len(calls) == 1 and mc.photometric_active
    cur, goal, z, Kc, W, live = calls[0][:6]
    assert cur.shape == (2, 24, 32, 3) and cur[0, 0, 0, 0] == 5 and cur[1, 0, 0, 0] == 7
    assert np.array_equal(np.asarray(goal)[:, 0, 0, 0], [0, 2]) and np.array_equal(np.asarray(z), depth[[0, 2]])
    assert Kc == p.intrinsics() and np.array_equal(W, mc.rig_W[[0, 2]]) and live is None
    assert calls[0][6:] == (1, "desired", 0.01, 0.03, 0.0, True, 3, 0.5)
    lp = mc.last_photometric
    assert lp["status"] == 0 and lp["cost"] == 2.0 and lp["n"] == 14 and lp["cameras"] == [0, 2] and lp["sigma"] == 1.5
    assert lp["gain"] == [1.1, 1.1] and lp["bias"] == [3.0, 3.0]
    assert np.allclose(lp["rejected"], [1 - 35.0 / (10 * 14)] * 2)                # 12 x 16 pooled, 10 x 14 inside the border
    assert np.array_equal(mc.rig_velocity_raw, [0.01, 0, 0, 0, 0, 0.02]) and np.array_equal(mc.v_rig, mc.rig_velocity_raw)
    assert all(c.v_c is None and c.photometric_active is False for c in mc.cameras)
    mc.ibvs()                                                                      # the same EMA as the rig laws'
    assert np.array_equal(mc.v_rig, mc.rig_velocity_raw) and len(calls) == 2
    mc.image_callback_rgb(1, np.zeros((24, 32, 3), np.uint8))                      # camera 1 joins: its goal depth and its holes
    mc.ibvs()
    assert np.array_equal(np.asarray(calls[2][2]), depth) and np.allclose(mc.last_photometric["rejected"][1], 1 - 35.0 / (10 * 7))


def test_the_scalar_depth_and_the_current_depths():
    calls = []
    mc, p = _controller(calls)
    for i in range(3):
        mc.image_callback_rgb(i, np.zeros((24, 32, 3), np.uint8))
    mc.photometric_active = True
    mc.ibvs()
    assert calls[0][2] is None and calls[0][10] == 0.6                             # no goal depth: homography_depth everywhere
    calls = []
    mc, p = _controller(calls, photometric_interaction="current")
    for i in range(3):
        mc.image_callback_rgb(i, np.zeros((24, 32, 3), np.uint8))
        mc.image_callback_depth(i, np.full((24, 32), 500 + i, np.uint16))
    mc.photometric_active = True
    mc.ibvs()
    assert np.array_equal(calls[0][2][:, 0, 0], [500, 501, 502]) and calls[0][10] == 0.0 and calls[0][7] == "current"


def test_a_status_that_is_not_ok_hands_back():
    calls = []
    mc, _ = _controller(calls, status=_lib.STATUS_TOO_FEW)
    for i in range(3):
        mc.image_callback_rgb(i, np.zeros((24, 32, 3), np.uint8))
    mc.photometric_active = True
    assert mc._photometric_round([0, 1, 2]) is False
    assert mc.photometric_active is False and mc.last_photometric["status"] == _lib.STATUS_TOO_FEW and mc.v_rig is None


def test_engine_checks_its_arguments_before_the_device():
    from vitvs_amd.engine import Engine, VitvsError
    eng = Engine.__new__(Engine)                               # no handle, no device: the checks come first
    f = np.zeros((2, 24, 32, 3), np.uint8)
    W = np.stack([np.eye(6)] * 2)
    Kc = (30.0, 30.0, 16.0, 12.0)
    with pytest.raises(VitvsError, match="uint8"):
        eng.photometric_rig_velocity_host(f.astype(np.float32), f, None, Kc, W, depth_scale=1.0)
    with pytest.raises(VitvsError, match="one shape"):
        eng.photometric_rig_velocity_host(f, f[:, :, :30], None, Kc, W, depth_scale=1.0)
    with pytest.raises(VitvsError, match="uint16"):
        eng.photometric_rig_velocity_host(f, f, np.zeros((2, 24, 32), np.int32), Kc, W)
    with pytest.raises(VitvsError, match="per camera"):
        eng.photometric_rig_velocity_host(f, f, None, np.zeros((3, 4)), W, depth_scale=1.0)
    for bad in (np.eye(6), np.zeros((3, 6, 6)), np.zeros((2, 36))):
        with pytest.raises(VitvsError, match="cVr"):
            eng.photometric_rig_velocity_host(f, f, None, Kc, bad, depth_scale=1.0)
    with pytest.raises(VitvsError, match="live"):
        eng.photometric_rig_velocity_host(f, f, None, Kc, W, [1, 1, 1], depth_scale=1.0)
    with pytest.raises(VitvsError, match="illumination"):
        eng.photometric_rig_velocity_host(f, f, None, Kc, W, depth_scale=1.0, illumination=2)
    with pytest.raises(VitvsError, match="robust_iterations"):
        eng.photometric_rig_velocity_host(f, f, None, Kc, W, depth_scale=1.0, robust_iterations=5)
    with pytest.raises(VitvsError, match="sigma_min"):
        eng.photometric_rig_velocity_host(f, f, None, Kc, W, depth_scale=1.0, sigma_min=0.0)
    with pytest.raises(VitvsError, match="interaction"):
        eng.photometric_rig_velocity_host(f, f, None, Kc, W, interaction="mean", depth_scale=1.0)


# ---------------------------------------------------------------------------------------------- (b) symbols
def test_the_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "vitvs.h")).read()
    lib = _lib.load()
    for name, count in (("vitvs_photometric_rig_velocity_dev", 25), ("vitvs_photometric_rig_velocity", 24)):
        assert f"VITVS_API int {name}(" in header, name
        assert name in _lib.PROTOTYPES and getattr(lib, name) is not None, name
        assert len(_lib.PROTOTYPES[name][1]) == count
        declared = header.split(f"VITVS_API int {name}(")[1].split(");")[0]
        assert declared.count(",") + 1 == count, name
    assert len(_lib.PROTOTYPES["vitvs_photometric_robust_velocity_dev"][1]) == 22  # the robust law's prototypes stand
    assert _lib.ABI_VERSION == 2 and lib.vitvs_abi_version() == 2
    from vitvs_amd.engine import Engine
    assert callable(Engine.photometric_rig_velocity) and callable(Engine.photometric_rig_velocity_host)


# ---------------------------------------------------------------------------------------------- (c) the reference itself
@pytest.fixture(scope="module")
def scene():
    sc = PlanarScene(synth.texture(128, 11), rs.SPAN / 128, PARAMS, plane_z=rs.PLANE_Z, device="cpu")
    ext = rs.rig()
    goal_rgb, goal_depth = rs.goals(sc, ext)
    return sc, ext, goal_rgb, goal_depth


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def test_one_camera_and_the_identity_is_the_robust_reference_bit_for_bit(scene):
    sc, ext, goal_rgb, goal_depth = scene
    Rr, tr = rs.start()
    cur = rs.frames(sc, ext, Rr, tr)
    _, depth = sc.render(*cl.camera_pose(Rr, tr, ext[0]))
    for i, z, scalar, inter in ((0, goal_depth[0], 0.0, 1), (1, depth, 0.0, 0), (2, None, 0.61, 1)):
        for illum, N in ((1, 4), (0, 2), (1, 0), (0, 0)):
            for reverse in (False, True):
                want = rr.velocity(cur[i], goal_rgb[i], z, scalar, K, rs.LEVEL, inter, rs.MU, rs.LAM, illum, N, 1.0, reverse=reverse)
                got = rg.velocity([cur[i]], [goal_rgb[i]], None if z is None else [z], scalar, [K], [np.eye(6)], None, rs.LEVEL, inter,
                                  rs.MU, rs.LAM, illum, N, 1.0, reverse=reverse)
                assert got["status"] == want["status"] == pr.OK
                assert np.array_equal(_bits(got["v"]), _bits(want["v"]))
                assert np.array_equal(_bits(got["normal"][0]), _bits(want["normal"]))
                assert np.array_equal(_bits(got["robust"][0]), _bits(want["robust"]))
                assert list(got["info"]) == [1, want["info"][0], want["info"][6], want["info"][7], want["info"][4], 0, 120, 160]
                assert got["margin_m"] == want["margin_m"] and got["margin_t"] == want["margin_t"]


def test_reference_statuses_dead_and_empty_cameras(scene):
    sc, ext, goal_rgb, goal_depth = scene
    Rr, tr = rs.start()
    cur = rs.frames(sc, ext, Rr, tr)
    W = [servo.twist_matrix(*e) for e in ext]
    args = (rs.LEVEL, rs.INTER, rs.MU, rs.LAM, 1, 4, 1.0)
    full = rg.velocity(cur, goal_rgb, goal_depth, 0.0, [K] * 3, W, None, *args)
    assert full["status"] == pr.OK and list(full["info"][[0, 1, 3, 4, 5, 6, 7]]) == [3, 3 * 118 * 158, 4, 0, 0, 120, 160]
    # a dead camera leaves no trace: the call equals the call without it, whatever its frames hold
    two = rg.velocity(cur[1:], goal_rgb[1:], goal_depth[1:], 0.0, [K] * 2, W[1:], None, *args)
    dead = rg.velocity(cur, goal_rgb, goal_depth, 0.0, [K] * 3, W, [0, 1, 1], *args)
    assert np.array_equal(_bits(dead["v"]), _bits(two["v"])) and np.array_equal(_bits(dead["normal"][1:]), _bits(two["normal"]))
    assert list(dead["info"]) == list(two["info"]) and not dead["normal"][0].any() and not dead["robust"][0].any()
    # a live camera without a row adds nothing and fails nothing
    holes = [np.zeros_like(goal_depth[0])] + goal_depth[1:]
    empty = rg.velocity(cur, goal_rgb, holes, 0.0, [K] * 3, W, None, *args)
    assert empty["status"] == pr.OK and np.array_equal(_bits(empty["v"]), _bits(two["v"]))
    assert list(empty["info"][[0, 1, 4]]) == [3, 2 * 118 * 158, 118 * 158] and not empty["robust"][0].any()
    none = rg.velocity(cur, goal_rgb, [np.zeros_like(goal_depth[0])] * 3, 0.0, [K] * 3, W, None, *args)
    assert none["status"] == pr.TOO_FEW and list(none["info"][[1, 4, 5]]) == [0, 3 * 118 * 158, 0] and not none["v"].any()
    nod = rg.velocity(cur, goal_rgb, None, 0.0, [K] * 3, W, None, *args)
    assert nod["status"] == pr.NO_DEPTH and not nod["v"].any()
    # a live camera whose 2 x 2 pivot fails (a flat goal: D is constant) fails the call
    flat = [np.full_like(goal_rgb[0], 90)] + goal_rgb[1:]
    out = rg.velocity([flat[0]] + cur[1:], flat, goal_depth, 0.0, [K] * 3, W, None, *args)
    assert out["status"] == pr.TOO_FEW and out["info"][5] == 1 and not out["v"].any() and not out["robust"].any()
    assert rg.velocity([flat[0]] + cur[1:], flat, goal_depth, 0.0, [K] * 3, W, None, rs.LEVEL, rs.INTER, rs.MU, rs.LAM, 0, 4,
                       1.0)["status"] == pr.OK                                      # (without the lighting model it adds zeros)


def test_no_run_of_the_device_test_is_left_out():
    """tests/test_gpu_photometric_rig_op.py compares the median bin and the rows of weight 0 exactly; its crops were chosen so that
    the reference keeps every row clear of the boundaries in every run."""
    import photometric_rig_cases as pc
    out = [run for run in pc.RUNS if pc.left_out(pc.reference(*run))]
    assert len(pc.RUNS) == 42 and not out, out
    for run in pc.RUNS:
        ref = pc.reference(*run)
        assert ref["status"] == pr.OK, run
        if run[2]:
            print(f"{run}: the half count lies {ref['margin_m']} rows inside its bin, the nearest row {ref['margin_e']:.2e} bins from an edge, "
                  f"|t - 1| >= {ref['margin_t']:.2e}; rows of weight 0 per camera {ref['zeros'].tolist()} of {ref['n'].tolist()}")


def _stacked(scale, illum, N):
    def law(cur, goal_rgb, goal_depth, W):
        return rg.velocity(cur, goal_rgb, goal_depth, 0.0, [K] * len(cur), W, None, rs.LEVEL, rs.INTER, rs.MU, rs.LAM, illum, N, 1.0,
                           scale=scale)
    return law


def _averaged(cur, goal_rgb, goal_depth, W):
    """The robust one-camera law per camera, each twist carried into the rig frame, the mean of them."""
    outs = [rr.velocity(c, g, z, 0.0, K, rs.LEVEL, rs.INTER, rs.MU, rs.LAM, 1, 4, 1.0) for c, g, z in zip(cur, goal_rgb, goal_depth)]
    ok = [i for i, o in enumerate(outs) if o["status"] == pr.OK]
    v = np.mean([np.linalg.solve(W[i], outs[i]["v"]) for i in ok], axis=0) if ok else np.zeros(6)
    return dict(v=v, status=pr.OK if ok else pr.TOO_FEW, robust=np.array([o["robust"] for o in outs]),
                zeros=np.array([o["info"][6] for o in outs]), n=np.array([o["info"][0] for o in outs]))


def _loop(scene, law, covered=rs.COVERED):
    sc, ext, goal_rgb, goal_depth = scene
    W = [servo.twist_matrix(*e) for e in ext]
    Rr, tr = rs.start()
    track, out = [cl.rig_pose_error(Rr, tr)], None
    for _ in range(rs.UPDATES):
        out = law(rs.frames(sc, ext, Rr, tr, covered), goal_rgb, goal_depth, W)
        if out["status"] == pr.OK:
            Rr, tr = rs.step(Rr, tr, out["v"])
        track.append(cl.rig_pose_error(Rr, tr))
    return track, out


def _show(name, track, out):
    print(f"photometric rig reference, {name}: pose error (cm / deg) at updates 0, 5, .., 30: "
          + "  ".join(f"{p:.4f}/{r:.4f}" for p, r in track[::5]))
    if out is not None and "robust" in out:
        with np.errstate(divide="ignore", invalid="ignore"):
            print(f"    gains {np.round(1 + out['robust'][:, 0], 4)}, biases {np.round(out['robust'][:, 1], 3)}, rows of weight 0 per "
                  f"camera {np.round(out['zeros'] / np.maximum(out['n'], 1), 3)}")


def test_the_one_median_stacked_law_reaches_the_goal(scene):
    track, out = _loop(scene, _stacked("stack", 1, 4))
    _show("stacked, one median, N = 4", track, out)
    p0, r0 = track[0]
    assert abs(p0 - 1.5) < 1e-9 and abs(r0 - 2.2) < 1e-6
    assert track[-1][0] < 0.1 and track[-1][1] < 0.1
    assert max(p for p, _ in track) <= p0 and max(r for _, r in track) <= r0
    assert out["status"] == pr.OK and out["zeros"][0] / out["n"][0] > 0.7           # camera 0 sets its covered rows aside
    assert abs(1 + out["robust"][1, 0] - 0.90) < 0.01 and abs(1 + out["robust"][2, 0] - 1.05) < 0.01


@pytest.mark.parametrize("name,law", [("stacked, each camera's own median, N = 4", _stacked("camera", 1, 4)),
                                      ("the one-camera robust laws averaged", _averaged),
                                      ("stacked, no illumination, N = 0", _stacked("stack", 0, 0))])
def test_the_other_laws_leave_the_goal(scene, name, law):
    track, out = _loop(scene, law)
    _show(name, track, out)
    assert track[-1][0] > 1.5


def test_on_clean_frames_both_laws_reach_the_goal(scene):
    """No occluder (the lightings stay): the stacked law and the average both pass the bar of the covered loop."""
    stacked, out = _loop(scene, _stacked("stack", 1, 4), covered=0)
    averaged, _ = _loop(scene, _averaged, covered=0)
    _show("clean frames, stacked, one median", stacked, out)
    _show("clean frames, the one-camera robust laws averaged", averaged, None)
    assert stacked[-1][0] < 0.1 and stacked[-1][1] < 0.1 and averaged[-1][0] < 0.1 and averaged[-1][1] < 0.1
