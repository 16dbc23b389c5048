"""The surface photometric law away from the GPU: the configuration, the YAML key, the refusals, the controller on
fake engines, the new symbols, the plan against its restatement, and tests/photometric_surface_ref.py itself, the fp64 reference the
device tests compare with.

The closed loops are test_photometric_tile_host.py's (640 x 480, level 2, the desired interaction matrix with the goal's depth image,
mu 0.01, lambda 0.5, dt 0.5, from 1.5 cm / 2.2 degrees; N = 4, sigma_min 1), every current frame under "ramp" (gain 0.9 .. 1.1 across
the width) or "spot" (a Gaussian lamp, gain 0.9 .. 1.2) of photometric_surface_cases.  The bars of the ramp and the undisturbed run
are ten times what this reference measures (the convention of test_photometric_host.py); the spot runs end below half of the start.
The tests assert the reference's behaviour, not a tolerance of the device.  The loop tests' docstrings have what this reference
measures."""
import ctypes as C
import os
import types

import numpy as np
import pytest

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib, config, servo, synth
import photometric_ref as pr
import photometric_robust_ref as rr
import photometric_tile_ref as tr
import photometric_surface_ref as sr
import photometric_surface_cases as sc
from planar_sim import PlanarScene, quat_xyzw, rodrigues
from solve_ref import THRESHOLD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ON = dict(photometric_illumination=True, photometric_robust_iterations=4)


# ---------------------------------------------------------------------------------------------- (a) configuration and refusals
def test_servo_params_validation():
    assert config.ServoParams().photometric_surface is None
    assert config.ServoParams(photometric_surface=(4, 8), **ON).photometric_surface == (4, 8)
    assert config.ServoParams(photometric_surface=[2, 3], **ON).photometric_surface == (2, 3)      # a YAML sequence
    assert config.ServoParams(photometric_surface=(1, 1), photometric_illumination=True).photometric_surface == (1, 1)   # a bilinear plane
    for bad in ((0, 4), (4, 9), (4,), (2, 2, 2), 4, "4x4", (2.0, 2), (True, 2)):
        with pytest.raises(ValueError, match="photometric_surface"):
            config.ServoParams(photometric_surface=bad, **ON)
    with pytest.raises(ValueError, match="photometric_illumination"):
        config.ServoParams(photometric_surface=(4, 4))
    with pytest.raises(ValueError, match="photometric_illumination"):
        config.ServoParams(photometric_surface=(4, 4), photometric_robust_iterations=4)
    with pytest.raises(ValueError, match="exclude each other"):
        config.ServoParams(photometric_surface=(4, 4), photometric_tiles=(4, 4), **ON)
    assert config.ServoParams(photometric_surface=(4, 4), photometric_tiles=(1, 1), **ON).photometric_tiles == (1, 1)
    assert config.ServoParams(photometric_surface=(2, 2), photometric_handback_rejected=0.25, **ON).photometric_handback_rejected == 0.25


def test_yaml_key():
    cfg = {k: 1 for k in config._REQUIRED_KEYS}
    cfg["image_path"] = "goal.png"
    assert config.load_reference_config(cfg).servo.photometric_surface is None
    cfg.update(photometric_illumination=True, photometric_robust_iterations=3, photometric_surface=[4, 2])
    ref = config.load_reference_config(cfg)
    assert ref.servo.photometric_surface == (4, 2) and ref.servo.photometric_tiles == (1, 1)
    assert not {k for k in ref.extras if k.startswith("photometric")}
    for key, bad, match in (("photometric_surface", [4, 16], "photometric_surface"), ("photometric_surface", 4, "photometric_surface"),
                            ("photometric_illumination", False, "photometric_illumination"),
                            ("photometric_tiles", [2, 2], "exclude each other")):
        with pytest.raises(ValueError, match=match):
            config.load_reference_config(dict(cfg, **{key: bad}))


class _FakeTwist:
    def __getitem__(self, i):
        return self

    def cpu(self):
        return self

    def numpy(self):
        return np.zeros(6)


def _fake_engine(params, calls, rejected=0.0625, status=0):
    base = dict(status=np.array([status]), cost=np.array([2.0]), n=np.array([7]))

    def plain(*a):
        calls.append(("plain", a))
        return _FakeTwist(), dict(base)

    def robust(*a):
        calls.append(("robust", a))
        return _FakeTwist(), dict(base, gain=np.array([1.15]), bias=np.array([8.0]), sigma=np.array([1.5]), rejected=np.array([rejected]))

    def tile(*a):
        calls.append(("tile", a))
        gy, gx = a[9]
        return _FakeTwist(), dict(base, sigma=np.array([1.5]), rejected=np.array([rejected]), tile_gain=np.ones((1, gy, gx)),
                                  tile_live=np.ones((1, gy, gx), bool), dead_tiles=np.array([0]))

    def surface(*a):
        calls.append(("surface", a))
        gy, gx = a[9]
        gain = np.linspace(0.9, 1.1, (gy + 1) * (gx + 1)).reshape(1, gy + 1, gx + 1)
        live = np.ones((1, gy + 1, gx + 1), bool)
        live[0, 0, 0] = False                                    # the dead unknown's gain of 1 is not in the range
        return _FakeTwist(), dict(base, sigma=np.array([1.5]), rejected=np.array([rejected]), node_gain=np.where(live, gain, 1.0),
                                  node_live=live, dead=np.array([3]))
    return types.SimpleNamespace(params=params, cfg=types.SimpleNamespace(img_size=224), apply_law_params=lambda p: None, max_pairs=4,
                                 set_goal_depth=lambda z: None, device="cpu", photometric_velocity=plain,
                                 photometric_robust_velocity=robust, photometric_tile_velocity=tile,
                                 photometric_surface_velocity=surface)


def _controller(calls, rejected=0.0625, status=0, **extra):
    p = config.ServoParams(photometric_handover=0.02, lambda_=0.03, u_max=32, v_max=24, homography_depth=0.6, **extra)
    ctl = servo.Controller(_fake_engine(p, calls, rejected, status), goal_image=np.zeros((24, 32, 3), np.uint8), params=p)
    ctl.image_callback_rgb(np.zeros((24, 32, 3), np.uint8))
    ctl.photometric_active = True
    return ctl, p


@pytest.mark.parametrize("extra,which", [({}, "plain"), (dict(ON), "robust"), (dict(ON, photometric_surface=None), "robust"),
                                         (dict(ON, photometric_tiles=(4, 4)), "tile"), (dict(ON, photometric_surface=(4, 4)), "surface"),
                                         (dict(photometric_illumination=True, photometric_surface=(1, 1)), "surface"),
                                         (dict(ON, photometric_surface=(8, 3), photometric_sigma_min=0.5), "surface")])
def test_the_controller_calls_the_surface_law_exactly_when_it_is_set(extra, which):
    calls = []
    ctl, p = _controller(calls, **extra)
    assert ctl._photometric_step() is True and ctl.photometric_active
    assert [c[0] for c in calls] == [which]
    args = calls[0][1]
    assert args[4:8] == (2, "desired", 0.01, 0.03)
    if which == "surface":
        assert args[9:] == (p.photometric_surface, p.photometric_robust_iterations, p.photometric_sigma_min) and len(args) == 12
        Q = (p.photometric_surface[0] + 1) * (p.photometric_surface[1] + 1)
        lo = 0.9 + 0.2 / (Q - 1)                                 # the second node's: the first is dead
        assert ctl.last_photometric == dict(status=0, cost=2.0, n=7, sigma=1.5, rejected=0.0625, dead=3, gain_min=pytest.approx(lo),
                                            gain_max=pytest.approx(1.1))
    elif which == "tile":
        assert args[9:] == (p.photometric_tiles, p.photometric_robust_iterations, p.photometric_sigma_min)
    elif which == "robust":
        assert args[9:] == (p.photometric_illumination, p.photometric_robust_iterations, p.photometric_sigma_min)
        assert ctl.last_photometric == dict(status=0, cost=2.0, n=7, gain=1.15, bias=8.0, sigma=1.5, rejected=0.0625)
    else:
        assert len(args) == 9 and ctl.last_photometric == dict(status=0, cost=2.0, n=7)


def test_the_hand_back_rule_covers_the_surface_law():
    for share, rejected, kept in ((0.25, 0.2501, False), (0.25, 0.25, True), (0.25, 0.1, True), (0.0, 0.99, True), (1.0, 1.0, True)):
        calls = []
        ctl, _ = _controller(calls, rejected=rejected, photometric_surface=(4, 4), photometric_handback_rejected=share, **ON)
        assert ctl._photometric_step() is kept and ctl.photometric_active is kept, (share, rejected)
        assert [c[0] for c in calls] == ["surface"] and ctl.last_photometric["rejected"] == rejected
    calls = []                                                   # a status that is not OK hands back as before
    ctl, _ = _controller(calls, status=_lib.STATUS_TOO_FEW, photometric_surface=(4, 4), photometric_handback_rejected=0.25, **ON)
    assert ctl._photometric_step() is False and ctl.photometric_active is False


def test_the_multi_controller_refuses_the_surface():
    goal = np.zeros((24, 32, 3), np.uint8)
    rig = [(np.eye(3), np.array([-0.1, 0.0, 0.0])), (np.eye(3), np.array([0.1, 0.0, 0.0]))]
    for extra in (dict(photometric_handover=0.02, homography_depth=0.6), {}):       # with the hand-over off too
        p = config.ServoParams(photometric_surface=(2, 2), lambda_=0.03, u_max=32, v_max=24, **extra, **ON)
        eng = types.SimpleNamespace(params=p, cfg=types.SimpleNamespace(img_size=224), apply_law_params=lambda q: None, max_pairs=4,
                                    set_goal_depth=lambda z: None, device="cpu", photometric_rig_velocity=lambda *a: None)
        with pytest.raises(ValueError, match="photometric_surface"):
            servo.MultiController(eng, [goal, goal], params=p, rig=rig)


def test_engine_checks_its_arguments_before_the_device():
    from vitvs_amd.engine import Engine, VitvsError
    eng = Engine.__new__(Engine)                               # no handle, no device: the checks come first
    f = np.zeros((24, 32, 3), np.uint8)
    K = (30.0, 30.0, 16.0, 12.0)
    with pytest.raises(VitvsError, match="uint8"):
        eng.photometric_surface_velocity_host(f.astype(np.float32), f, None, K, depth_scale=1.0)
    with pytest.raises(VitvsError, match="one shape"):
        eng.photometric_surface_velocity_host(f, f[:, :30], None, K, depth_scale=1.0)
    for bad in ((0, 2), (2, 9), (2,), 4, (2.5, 2), (True, 2), None, "22"):
        with pytest.raises(VitvsError, match="cells"):
            eng.photometric_surface_velocity_host(f, f, None, K, depth_scale=1.0, cells=bad)
    for bad in (-1, 5, 2.5, True):
        with pytest.raises(VitvsError, match="robust_iterations"):
            eng.photometric_surface_velocity_host(f, f, None, K, depth_scale=1.0, robust_iterations=bad)
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(VitvsError, match="sigma_min"):
            eng.photometric_surface_velocity_host(f, f, None, K, depth_scale=1.0, sigma_min=bad)


# ---------------------------------------------------------------------------------------------- (b) symbols and the plan
def test_the_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "vitvs.h")).read()
    lib = _lib.load()
    for name, count in (("vitvs_photometric_surface_velocity_dev", 24), ("vitvs_photometric_surface_velocity", 23),
                        ("vitvs_op_photometric_surface_plan", 6)):
        assert f"VITVS_API int {name}(" in header, name
        assert name in _lib.PROTOTYPES and getattr(lib, name) is not None, name
        assert len(_lib.PROTOTYPES[name][1]) == count
        declared = header.split(f"VITVS_API int {name}(")[1].split(");")[0]
        assert declared.count(",") + 1 == count, name
    assert len(_lib.PROTOTYPES["vitvs_photometric_tile_velocity_dev"][1]) == 24       # the tile law's prototypes stand
    assert _lib.ABI_VERSION == 2 and lib.vitvs_abi_version() == 2
    from vitvs_amd.engine import Engine
    assert callable(Engine.photometric_surface_velocity) and callable(Engine.photometric_surface_velocity_host)
    io = open(os.path.join(ROOT, "vit-vs_amd", "csrc", "io_layout.h")).read()
    check = open(os.path.join(ROOT, "tools", "io_layout_check.cpp")).read()
    assert "struct PhotometricSurfaceIo" in io and "photometric_surface_io(" in check


def _plan(H, W, level, gy, gx, which="surface"):
    out = np.full(8, -7, np.int32)
    rc = getattr(_lib.load(), f"vitvs_op_photometric_{which}_plan")(H, W, level, gy, gx, out.ctypes.data_as(C.c_void_p))
    return rc, tuple(int(x) for x in out)


def test_the_plan_equals_its_restatement():
    shapes = [(480, 640, 2, 4, 4), (480, 640, 0, 8, 8), (224, 224, 0, 2, 2), (24, 32, 0, 3, 5), (23, 29, 0, 4, 4), (70, 32, 0, 8, 2),
              (1042, 16, 1, 3, 1), (1042, 16, 1, 4, 1), (521, 16, 0, 1, 1), (4096, 4096, 0, 8, 8), (4096, 8, 0, 8, 8), (2048, 64, 1, 5, 7),
              (24, 8, 0, 2, 8), (4096, 4096, 3, 8, 8), (3, 3, 0, 3, 3)]
    for H, W, level, gy, gx in shapes:
        rc, out = _plan(H, W, level, gy, gx)
        assert rc == 0 and out == sr.plan(H, W, level, gy, gx), (H, W, level, gy, gx, out)
        rc, tile = _plan(H, W, level, gy, gx, "tile")
        assert rc == 0 and out[:7] == tile[:7] and out[7] * 48 == tile[7] * 128            # the tile law's bands, slots and LDS
        assert out[3] * out[4] <= 4096 and out[7] <= 4096 * 8 * 128                        # inside the 32 MiB per pair
    assert sr.plan(480, 640, 2, 4, 4)[7] == 120 * 4 * 128
    for bad in ((480, 640, 2, 0, 4), (480, 640, 2, 4, 9), (24, 32, 2, 7, 2), (24, 28, 2, 2, 8), (20, 32, 2, 6, 8), (4097, 32, 0, 2, 2),
                (24, 32, 4, 1, 1), (8, 8, 2, 1, 1)):
        rc, out = _plan(*bad)
        assert rc == -2 and out == (0,) * 8, bad
    assert _lib.load().vitvs_op_photometric_surface_plan(480, 640, 2, 4, 4, None) == -1


# ---------------------------------------------------------------------------------------------- (c) the reference itself
PARAMS = config.ServoParams(dino_input_size=224, use_feature_binning=False)
PLANE_Z, SPAN, DT = 0.61, 1.6, 0.5
LEVEL, INTER, MU, LAM = 2, 1, 0.01, 0.5
BARS_GLOBAL = ((1.62e-14, 1.93e-12, 7.80e-14), (1.78e-13, 1.82e-11, 8.56e-14), (1.97e-12, 3.25e-10, 6.11e-13))     # measured gaps of the global gain / bias test (its docstring)


def gain_bias(rgb, gain=1.15, bias=8.0):
    return np.clip(np.round(gain * rgb.astype(np.float64) + bias), 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def scene():
    scn = PlanarScene(synth.texture(128, 11), SPAN / 128, PARAMS, plane_z=PLANE_Z, device="cpu")
    goal_rgb, goal_depth = scn.render(np.eye(3), np.zeros(3))
    return scn, goal_rgb, goal_depth


def _pose_error(R, t):
    q = quat_xyzw(R)
    return float(np.linalg.norm(t) * 100), float(np.rad2deg(2 * np.arccos(min(1.0, abs(q[3])))))


def _start():
    axis = np.array([0.3, -0.4, 0.85])
    direction = np.array([0.6, -0.5, 0.6])
    return rodrigues(axis / np.linalg.norm(axis) * np.deg2rad(2.2)), direction / np.linalg.norm(direction) * 0.015


def _loop(scene, disturb, law, updates):
    """(track of (cm, deg), the last law output)."""
    scn, goal_rgb, goal_depth = scene
    R, t = _start()
    track, out = [_pose_error(R, t)], None
    for _ in range(updates):
        rgb, _ = scn.render(R, t)
        out = law(disturb(rgb), goal_rgb, goal_depth)
        assert out["status"] == pr.OK
        v, w = out["v"][:3], out["v"][3:]
        t = t + R @ v * DT
        R = R @ rodrigues(w * DT)
        track.append(_pose_error(R, t))
    print("closed loop: pose error (cm / deg) at updates 0, 10, ..: " + "  ".join(f"{p:.4f}/{r:.4f}" for p, r in track[::10])
          + f"; the last ({len(track) - 1}) {track[-1][0]:.4f}/{track[-1][1]:.4f}")
    return track, out


def _tiles(gy, gx):
    return lambda cur, goal, depth: tr.velocity(cur, goal, depth, 0.0, PARAMS.intrinsics(), LEVEL, INTER, MU, LAM, gy, gx, 4, 1.0)


def _surface(gy, gx):
    return lambda cur, goal, depth: sr.velocity(cur, goal, depth, 0.0, PARAMS.intrinsics(), LEVEL, INTER, MU, LAM, gy, gx, 4, 1.0)


DISTURB = dict(ramp=sc.ramp, spot=sc.spot, none=lambda rgb: rgb)


def _first_frame(scene, disturb):
    scn, goal_rgb, goal_depth = scene
    R, t = _start()
    rgb, _ = scn.render(R, t)
    return disturb(rgb), goal_rgb, goal_depth


def test_the_cell_and_the_weights_of_a_row():
    """cell = the tile law's tile; phi sums to 1 and is the bilinear weight of the pixel in its cell, exact at the cell's first row
    and column."""
    Z = np.full((24, 32), 600, np.uint16)
    Z[5, 7] = 0
    cell, phi = sr.weights_of_rows((24, 32), Z, 0, 3, 5)
    assert np.array_equal(cell, tr.tile_of_rows((24, 32), Z, 0, 3, 5)) and phi.shape == (22 * 30 - 1, 4)
    assert np.all(phi >= 0) and np.max(np.abs(phi.sum(axis=1) - 1.0)) < 4e-16
    r, c = np.mgrid[1:23, 1:31]
    keep = ~((r == 5) & (c == 7))
    at = {(int(a), int(b)): k for k, (a, b) in enumerate(zip(r[keep], c[keep]))}
    assert np.array_equal(phi[at[(8, 13)]], [1.0 - 1 / 32, 1 / 32, 0.0, 0.0])        # 8 * 3 = 24 and 13 * 5 = 65 = 2 * 32 + 1: v = 0
    assert list(sr.weights_of_rows((24, 32), None, 0, 3, 4)[1][7 * 30 + 7]) == [1.0, 0.0, 0.0, 0.0]    # pixel (8, 8): a cell's first corner
    assert np.array_equal(phi[at[(16, 26)]], [1.0 - 2 / 32, 2 / 32, 0.0, 0.0])       # 26 * 5 = 130 = 4 * 32 + 2
    v, u = (9 * 3 - 24) / 24, (14 * 5 - 64) / 32
    assert np.array_equal(phi[at[(9, 14)]], [(1 - v) * (1 - u), (1 - v) * u, v * (1 - u), v * u])
    assert sr.cell_nodes(7, 5) == [7 + 1, 7 + 2, 7 + 7, 7 + 8] and sr.cell_nodes(0, 1) == [0, 1, 2, 3]


@pytest.mark.parametrize("grid", [(2, 2), (4, 4), (8, 8)])
def test_the_banded_elimination_equals_a_dense_solve(scene, grid):
    """The bordered right-looking elimination against numpy.linalg.solve of the assembled live system: H', g' and q.  Measured
    (relative, the largest over the grids, at 8 x 8): H' 1.7e-13, g' 1.8e-13, q 2.9e-12 at a condition number of 2.2e9 (3.1e7 at
    2 x 2, 1.5e8 at 4 x 4); asserted at ten times."""
    gy, gx = grid
    cur, goal, depth = _first_frame(scene, sc.ramp)
    out = sr.velocity(cur, goal, depth, 0.0, PARAMS.intrinsics(), LEVEL, INTER, MU, LAM, gy, gx, 0, 1.0)
    assert out["status"] == pr.OK
    Cg, R, S = sr.assemble(out["normal"], gy, gx)
    assert np.array_equal(Cg, Cg.T)
    el = sr.eliminate(Cg, R, S, gx)
    live = el["live"]
    assert live.all()
    # nothing outside the band: nodes that share no cell
    i, j = np.nonzero(Cg)
    assert np.max(np.abs(i - j)) == 2 * gx + 5
    sol = np.linalg.solve(Cg, R.T)                                 # C_g^-1 [B_g^T, d_g]
    want = S - R @ sol
    rel = lambda a, b: float(np.max(np.abs(a - b)) / np.max(np.abs(b)))  # noqa: E731
    gaps = [rel(el["S"][:6, :6], want[:6, :6]), rel(el["S"][:6, 6], want[:6, 6])]
    x = out["passes"][0]["x"]
    q = np.linalg.solve(Cg, R[6] + R[:6].T @ x)
    gaps.append(rel(out["passes"][0]["q"], q))
    print(f"{grid}: cond {np.linalg.cond(Cg):.2e}, relative gaps of H', g', q to the dense solve: " + " ".join(f"{g:.2e}" for g in gaps))
    assert gaps[0] < 1.7e-12 and gaps[1] < 1.8e-12 and gaps[2] < 2.9e-11


def test_the_bias_block_sums_to_the_weights(scene):
    """sum phi = 1: the beta-beta block of C_g sums to sum w, and the beta columns of B_g to sum w L.  Measured: 2.1e-16 and 7.9e-15
    relative; asserted at ten times."""
    cur, goal, depth = _first_frame(scene, sc.ramp)
    for N in (0, 4):
        out = sr.velocity(cur, goal, depth, 0.0, PARAMS.intrinsics(), LEVEL, INTER, MU, LAM, 4, 4, N, 1.0)
        Cg, R, _ = sr.assemble(out["normal"], 4, 4)
        sw = out["robust"][3]
        assert sw == (118.0 * 158.0 if N == 0 else sw) and sw > 0
        gap = abs(Cg[1::2, 1::2].sum() - sw) / sw
        got = rr.rows(cur, goal, depth, 0.0, PARAMS.intrinsics(), LEVEL, INTER)
        wl = (out["weights"][:, None] * got[0]).sum(axis=0)
        gap_b = float(np.max(np.abs(R[:6, 1::2].sum(axis=1) - wl) / np.abs(wl).max()))
        print(f"N = {N}: beta-beta block against sum w {gap:.2e}, beta columns of B_g against sum w L {gap_b:.2e}")
        assert gap < 2.1e-15 and gap_b < 7.9e-14


def test_a_global_gain_and_bias_is_the_robust_reference(scene):
    """Under a global gain 1.15 and bias 8 the constant surface is the exact minimiser: every live node's pair equals the robust
    reference's (gamma, beta) = (0.15, 8) and the twist its twist.  The rows are the scene's; e = 0.15 D + 8 - L x0 is formed in fp64,
    since a uint8 frame under that gain clips and rounds (the frames' own fit is gamma 0.046, beta 20.7, and a surface fits the
    clipped regions better than a constant can: 0.07 .. 2 away), and mu = 0, since the damped step leaves a residual L (x - x0) that
    a surface absorbs in part.  Measured against the robust reference (gamma_a, beta_a in grey levels, v relative): 1 x 1 1.6e-14, 1.9e-12,
    7.8e-14; 4 x 4 1.8e-13, 1.8e-11, 8.6e-14; 8 x 8 2.0e-12, 3.3e-10, 6.1e-13 (BARS_GLOBAL); the robust reference itself is 1e-15 and
    1.4e-13 from (0.15, 8).  Asserted at ten times."""
    cur, goal, depth = _first_frame(scene, lambda rgb: rgb)
    L, _, D, _, _, _ = rr.rows(cur, goal, depth, 0.0, PARAMS.intrinsics(), LEVEL, INTER)
    x0 = np.array([0.004, -0.003, 0.005, 0.01, -0.008, 0.02])
    e = (0.15 * D + 8.0) - L @ x0
    w = np.ones(L.shape[0])
    v_r, x_r, gamma, beta, solved = rr.solve45(rr.weighted_sums(L, e, D, w)[0], 0.0, LAM, 1)
    assert solved
    print(f"the robust reference: gamma - 0.15 = {gamma - 0.15:.2e}, beta - 8 = {beta - 8:.2e}, |x - x0| = {np.max(np.abs(x_r - x0)):.2e}")
    assert abs(gamma - 0.15) < 1e-9 and abs(beta - 8.0) < 1e-7
    for grid, bars in (((1, 1), BARS_GLOBAL[0]), ((4, 4), BARS_GLOBAL[1]), ((8, 8), BARS_GLOBAL[2])):
        cell, phi = sr.weights_of_rows(cur.shape[:2], depth, LEVEL, *grid)
        normal, _, _ = sr.cell_sums(L, e, D, phi, w, cell, grid[0] * grid[1])
        v, x, q, live, _, solved = sr.solve_cells(normal, *grid, 0.0, LAM)
        assert solved and live.all()
        gaps = (float(np.max(np.abs(q[0::2] - gamma))), float(np.max(np.abs(q[1::2] - beta))),
                float(np.linalg.norm(v - v_r) / np.linalg.norm(v_r)))
        print(f"{grid}: gaps of gamma_a, beta_a, v to the robust reference: " + " ".join(f"{g:.2e}" for g in gaps))
        assert gaps[0] < 10 * bars[0] and gaps[1] < 10 * bars[1] and gaps[2] < 10 * bars[2]


def test_a_flat_region_gives_dead_unknowns(scene):
    """Goal and current frame flat over the pixel block of cells (1 .. 2, 1 .. 2) of a 4 x 4 grid: D is constant over the support
    of node (2, 2), so its beta is collinear with its gamma and dead; status OK, its value 0, and the other unknowns are the solution
    of the system without that row and column."""
    cur, goal, depth = _first_frame(scene, sc.ramp)
    cur, goal = cur.copy(), goal.copy()
    cur[120:360, 160:480] = 90
    goal[120:360, 160:480] = 90
    for N in (0, 4):
        out = sr.velocity(cur, goal, depth, 0.0, PARAMS.intrinsics(), LEVEL, INTER, MU, LAM, 4, 4, N, 1.0)
        dead = 2 * (2 * 5 + 2) + 1
        assert out["status"] == pr.OK and list(out["robust"][:2]) == [49.0, 1.0]
        p = out["passes"][-1]
        assert np.array_equal(np.nonzero(~p["live"])[0], [dead]) and p["q"][dead] == 0.0 and abs(p["ratio"][dead]) < 1e-9
        assert out["nodes"][12, 3] == 0.0 and out["nodes"][12, 2] == 1.0 and out["nodes"][12, 1] == 0.0
        Cg, R, _ = sr.assemble(out["normal"], 4, 4)
        keep = p["live"]
        q = np.linalg.solve(Cg[np.ix_(keep, keep)], (R[6] + R[:6].T @ p["x"])[keep])
        assert np.max(np.abs(p["q"][keep] - q)) < 1e-7 * np.max(np.abs(q))


def test_every_unknown_dead_is_too_few(scene):
    _, goal_rgb, goal_depth = scene
    black = np.zeros_like(goal_rgb)                                # D = 0: no gain column; no bias column either without a row
    out = sr.velocity(black, black, goal_depth, 0.0, PARAMS.intrinsics(), LEVEL, INTER, MU, LAM, 4, 4, 4, 1.0)
    assert out["status"] == pr.TOO_FEW and list(out["info"][5:]) == [1, 0, 0] and np.array_equal(out["v"], np.zeros(6))
    assert np.array_equal(out["robust"], np.zeros(4)) and np.array_equal(out["nodes"], np.zeros((25, 4)))
    normal = np.zeros((16, sr.NS))
    assert sr.solve_cells(normal, 4, 4, MU, LAM)[5] is False
    out = sr.velocity(goal_rgb, goal_rgb, None, 0.0, PARAMS.intrinsics(), LEVEL, INTER, MU, LAM, 4, 4, 4, 1.0)
    assert out["status"] == pr.NO_DEPTH
    same = sr.velocity(goal_rgb, goal_rgb, goal_depth, 0.0, PARAMS.intrinsics(), LEVEL, INTER, MU, LAM, 4, 4, 4, 1.0)
    assert same["status"] == pr.OK and np.max(np.abs(same["v"])) < 1e-12 and list(same["info"][6:]) == [0, 4]
    assert list(same["robust"]) == [50.0, 0.0, 1.0, 118.0 * 158.0]


def test_the_device_tests_cases_are_clean_and_reach_the_paths_they_name():
    """No device result: every crop's reference, for every N of 0, 1 and 4, has status OK, margin_m >= 3 in every re-weighting, no row
    within 1e-9 of Tukey's cut and every pivot ratio outside [THRESHOLD / 2, 2 THRESHOLD]: no case is left out of any exact
    comparison.  And the special cases are what their names say."""
    for name in sc.CASES:
        for N in sc.NS:
            ref = sc.reference(name, N)
            assert ref["status"] == pr.OK and ref["near_t"] == 0, (name, N)
            assert N == 0 or ref["margin_m"] >= 3, (name, N, ref["margin_m"])
            assert len(ref["passes"]) == N + 1
            for p in ref["passes"]:
                r = p["ratio"][np.isfinite(p["ratio"])]
                assert not np.any((r >= THRESHOLD / 2) & (r <= 2 * THRESHOLD)), (name, N)
            assert sc.clean(ref, N)
    plans = {name: sr.plan(c[0], c[1], c[2], *c[3]) for name, c in sc.CASES.items()}
    assert plans["1042x16-l1-3x1"][:5] == (521, 8, 2, 261, 2) and plans["70x32-l0-8x2"][:5] == (70, 32, 1, 70, 1)
    cut = {}
    for name, c in sc.CASES.items():
        h, _, rows, bands = plans[name][:4]
        first = np.arange(bands) * rows
        last = np.minimum(first + rows, h) - 1
        cut[name] = [int(b) for b in np.nonzero(first * c[3][0] // h != last * c[3][0] // h)[0]]
    assert cut["1042x16-l1-4x1"] == [65, 130, 195] and all(not b for name, b in cut.items() if name != "1042x16-l1-4x1")
    for name in ("1042x16-l1-3x1", "1042x16-l1-4x1"):
        ref = sc.reference(name, 4)
        assert ref["robust"][1] == 0 and np.all(ref["cell_n"] > 0) and ref["info"][6] > 0     # every unknown live, rows rejected
    full = sc.reference("48x64-l2-8x8", 4)
    assert full["nodes"].shape == (81, 4) and plans["48x64-l2-8x8"][:2] == (12, 16) and full["robust"][0] + full["robust"][1] == 162
    Cg = sr.assemble(full["normal"], 8, 8)[0]
    i, j = np.nonzero(Cg)
    assert np.max(np.abs(i - j)) == 21                            # the full bandwidth
    flat = sc.reference("48x64-l2-4x4-flat", 4)
    assert flat["nodes"][12, 3] == 0.0 and flat["nodes"][12, 2] == 1.0      # node (2, 2): the gain lives, the bias is dead
    edge = sc.reference("24x8-l0-2x8", 4)
    assert np.all(edge["cell_n"][[0, 7, 8, 15]] == 0)
    assert np.all(edge["nodes"].reshape(3, 9, 4)[:, [0, 7, 8], 2:] == 0)    # the border columns' nodes: no row has a weight on them
    holes = sc.reference("48x64-l2-4x4-holes", 0)
    assert holes["info"][4] == 9 and holes["info"][0] == 140 - 9


# ---------------------------------------------------------------------------------------------- (d) the need and the remedy
@pytest.mark.parametrize("disturb", ["ramp", "spot"])
def test_the_tile_reference_drifts_away_under_a_smooth_field(scene, disturb):
    """The need: 4 x 4 tiles under a smooth lighting field end farther away than they started after 60 updates, with every status
    OK.  DESIGN.md 5n: 2.12 cm / 1.86 degrees under the ramp, 2.03 / 1.73 under the spot; this run measures 2.1230 / 1.8584 and 2.0324 / 1.7293."""
    track, _ = _loop(scene, DISTURB[disturb], _tiles(4, 4), 60)
    assert track[-1][0] > track[0][0]


@pytest.mark.parametrize("grid,disturb,bar", [((4, 4), "ramp", (0.585, 0.534)), ((4, 4), "none", (0.184, 0.154)), ((4, 4), "spot", None),
                                              ((8, 8), "spot", None)])
def test_the_surface_reference_loop_ends_at_the_goal(scene, grid, disturb, bar):
    """The remedy: 40 updates; no track point lies above the start; the ramp run and the undisturbed run end below ten times what
    this reference measures, the spot runs below one half of the start (ten times the measured 0.27 cm would say nothing).
    Measured with this reference (cm / degrees): 4 x 4 under "ramp" 0.0585 / 0.0534 (0.0492 / 0.0440 at update 30), 4 x 4
    undisturbed 0.0184 / 0.0154, 4 x 4 under "spot" 0.2727 / 0.1266, 8 x 8 under "spot" 0.1973 / 0.1712; no unknown is dead at the end of any."""
    track, out = _loop(scene, DISTURB[disturb], _surface(*grid), 40)
    assert max(p for p, _ in track) <= track[0][0] and max(r for _, r in track) <= track[0][1]
    if bar is None:
        assert track[-1][0] < 0.5 * track[0][0] and track[-1][1] < 0.5 * track[0][1]
    else:
        assert track[-1][0] < bar[0] and track[-1][1] < bar[1]
    gains = 1.0 + out["nodes"][:, 0].reshape(grid[0] + 1, grid[1] + 1)
    print(f"{grid} {disturb}: live {int(out['robust'][0])}, dead {int(out['robust'][1])}, sigma {out['robust'][2]:.3f}, rows of weight 0: "
          f"{out['info'][6]} of {out['info'][0]}; node gains\n{np.round(gains, 3)}")
    if disturb == "ramp":
        x_node = np.arange(grid[1] + 1) * 640.0 / grid[1]
        assert out["robust"][1] == 0 and np.max(np.abs(gains - (0.9 + 0.2 * x_node / 639.0)[None, :])) < 0.05
