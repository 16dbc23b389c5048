"""The control law away from 640 x 480 (GPU): the map from a token to a camera pixel, the bounds of the depth image, the depth a
zero-padded row reads, the patch pitches behind sigma_min, and the host-pointer calls' depth staging, at the geometries of
tests/geometry_cases.py.

The code states the token-to-pixel map five times: servo.hip's token_pixel (on the prefetched depth path, T <= 256, and the direct
one), refined_pixel and goal_depth_kernel, api.hip's host-side depth sites (which pixels of the caller's image a host-pointer call
hands over), and the pitches that feed sigma_min in the robust, pose, homography and rig laws.  Every other GPU test of the law
runs at 640 x 480, where no product centre * scale is a rounding tie, nothing lies outside the image and pixel (0, 0) is no patch
centre.  tests/test_geometry_host.py pins, on the reference alone, what each geometry here adds: every token a tie (ties14,
ties17), the order of the fp64 operations (near308), pixels ON the image's edge, shared pixels and the origin (tiny, tiny17),
pitch_v > pitch_u (portrait), linear pixel indices above 2^20 (hd).

The bars are the plain law's (tests/test_gpu_servo_cover.py): s_uv, Z and Z* exact, L / e within 1e-13, v_c within 1e-9 (relative
L2); robust weights within 1e-9; host-pointer calls equal to device-pointer calls bit for bit."""
import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib, servo, synth, weights
from vitvs_amd.engine import Engine, VitvsError
import geometry_cases as gc
import homography_ref as hr
import interaction_ref as ir
import pose_ref as pr
import robust_ref as rr
import law_support as ls
from law_support import close_engines  # noqa: F401

pytestmark = pytest.mark.gpu

LDLT = -1
VC_BAR, L_BAR, W_BAR = 1e-9, 1e-13, 1e-9
MARGIN = 1e-6
K_PAIRS = gc.PAIRS


class GeometryEngines:
    """This module's weight-less handles (the law alone), one per geometry, with room for every token as a row."""

    def __init__(self):
        self.engines = {}

    def fetch(self, name):
        """The geometry's handle with every follow-on option off."""
        if name not in self.engines:
            geo = gc.geometry(name)
            self.engines[name] = Engine(geo.vit_config(), geo.params(), precision="fp32", max_pairs=1, max_rows=geo.tokens)
        eng = self.engines[name]
        for option in ls.LAW_OPTIONS:
            eng.set_option(option, 0)
        return eng

    def close(self):
        for eng in self.engines.values():
            eng.close()
        self.engines.clear()


ENGINES = GeometryEngines()       # close_engines closes them at the module's teardown


def _check_law(det, v, st, ref, s_star, s_, rows, what, z_column=None):
    """One pair's law against the reference's: pixels and Z exact, L / e within 1e-13, v_c within 1e-9, solved by LDL^T (every
    case's L passes the pivot test: tests/test_geometry_host.py)."""
    assert int(st) == _lib.STATUS_OK, (what, int(st))
    info = det["info"][0]
    assert int(info[5]) == 2 * rows and int(info[4]) == LDLT, (what, info)
    suv = det["s_uv"][0, :rows]
    assert np.array_equal(suv[:, 0:2], s_star), (what, "goal pixels", np.nonzero(np.any(suv[:, 0:2] != s_star, axis=1))[0])
    assert np.array_equal(suv[:, 2:4], s_), (what, "current pixels", np.nonzero(np.any(suv[:, 2:4] != s_, axis=1))[0])
    assert np.array_equal(det["feat"][0, :rows, 0:1], ref["Z"] if z_column is None else z_column), (what, "Z")
    lerr = float(np.max(np.abs(det["L"][0, :6, :2 * rows].T - ref["L"])))
    eerr = float(np.max(np.abs(det["L"][0, 6, :2 * rows] - ref["e"][:, 0])))
    err = rr.rel_l2(v, ref["v_c"])
    print(f"{what}: L max abs error {lerr:.2e}, e {eerr:.2e}, v_c rel L2 {err:.2e}")
    assert lerr <= L_BAR and eerr <= L_BAR, (what, lerr, eerr)
    assert err <= VC_BAR, (what, err)


# ----------------------------------------------------------------------------- 1. the law on tables, every geometry
@pytest.mark.parametrize("mode", gc.TABLE_MODES)
@pytest.mark.parametrize("name", list(gc.GEOMETRIES))
def test_law_on_tables(name, mode):
    """ORDER, DENSE, EXPLICIT with 24 ids, EXPLICIT with 6 of 24 ids (18 zero-padded rows, which read depth[0, 0], a depth) and
    EXPLICIT with 3 ids (TOO_FEW).  ties14 / ties17: every pixel is a rounding tie, on the prefetched and on the direct depth path;
    near308: the order of the fp64 operations; tiny / tiny17: rows on the image's edge read 100 m."""
    c = gc.table_case(name, mode)
    eng = ENGINES.fetch(name)
    tabs = (c["nn_1"], c["nn_2"], c["sim_1"], c["depth"], c["K"])
    if mode == "order":
        v, st = eng.servo_from_nn(*tabs, mode=_lib.SELECT_ORDER, selection=c["order"], num_pairs=K_PAIRS)
    elif mode == "dense":
        v, st = eng.servo_from_nn(*tabs, mode=_lib.SELECT_DENSE, num_pairs=K_PAIRS)
    else:
        v, st = eng.servo_from_nn(*tabs, mode=_lib.SELECT_EXPLICIT, selection=[c["ids"]], num_pairs=K_PAIRS)
    v, det = v.cpu().numpy(), eng.last_details(1)
    rows, n = c["rows"], len(c["ids"])
    assert int(det["info"][0, 0]) == len(c["mutual"])
    if mode == "too_few":
        assert int(st) == _lib.STATUS_TOO_FEW and not v.any() and not det["s_uv"][0, :K_PAIRS].any()
        return
    assert int(det["info"][0, 3]) == n and det["selected"][0, :n].tolist() == c["ids"].tolist()
    _check_law(det, v, st, c["ref"], c["s_star"], c["s_uv"], rows, (name, mode))
    if mode == "padded":
        assert np.all(det["feat"][0, n:rows, 0] == c["depth"][0, 0] / 1000.0) and c["depth"][0, 0] != 0
    if name.startswith("tiny"):
        out = gc.outside(c["geo"], det["s_uv"][0, :n, 2:4])
        assert out.any() and np.all(det["feat"][0, :n, 0][out] == 100.0)


# ----------------------------------------------------------------------------- 2. the goal-depth table
@pytest.mark.parametrize("interaction", ir.MODES[1:])
@pytest.mark.parametrize("name", list(gc.GEOMETRIES))
def test_goal_depth_table(name, interaction):
    """set_goal_depth at every geometry: an EXPLICIT selection of every token reads every entry of the table below T (0, read as
    100 m, for the tokens outside the image in tiny), one of 6 of 24 ids reads entry T for its padded rows (pixel (0, 0), a depth)."""
    c = gc.goal_case(name, interaction)
    geo, params, zg = c["geo"], c["params"], c["goal_depth"]
    eng = ENGINES.fetch(name)
    eng.set_option("interaction", ir.MODES.index(interaction))
    eng.set_goal_depth(zg)
    table = ls.goal_table(zg, geo.grid, geo.img, params)
    metres = np.where(table != 0, table / 1000.0, 100.0)
    out = gc.outside(geo, gc.token_pixels(geo))
    assert not table[:-1][out].any() and out.any() == name.startswith("tiny") and table[-1] == zg[0, 0] != 0
    for what, ids, rows in (("every token", c["every"], geo.tokens), ("padded", c["few"], K_PAIRS)):
        v, st = eng.servo_from_nn(c["nn_1"], c["nn_2"], c["sim_1"], c["depth"], c["K"], mode=_lib.SELECT_EXPLICIT, selection=[ids],
                                  num_pairs=rows)
        v, det = v.cpu().numpy(), eng.last_details(1)
        s_star, s_ = gc.features(geo, c["nn_1"], ids, rows)
        ref = ir.law(s_star, s_, c["depth"], zg, c["K"], params.lambda_, interaction)
        z_goal = eng.last_goal_depth(1)[0]
        assert np.array_equal(z_goal[:len(ids)], metres[ids]), (name, interaction, what)
        assert np.all(z_goal[len(ids):rows] == metres[-1]) and not z_goal[rows:].any(), (name, interaction, what)
        assert np.array_equal(z_goal[:rows, None], ref["Z_goal"]), (name, interaction, what)
        _check_law(det, v, st, ref, s_star, s_, rows, (name, interaction, what), ref["Z"] if interaction == "mean" else ref["Z_goal"])
    eng.set_goal_depth(None)


# ----------------------------------------------------------------------------- 3. sigma_min
@pytest.mark.parametrize("name", list(gc.ROBUST_CASES))
def test_robust_law_floor(name):
    """robust_law with N = 2 where the floor sigma_min = 0.5 max(pitch_u / f_x, pitch_v / f_y) decides the twist (tests/test_geometry_host.py):
    portrait (the pitch_v term is the larger one), tiny, hd with f_x = f_y, and portrait with f_x != f_y, where exchanging the
    pitches gives another twist."""
    c = gc.robust_case(name)
    geo, params, sc, ref, rob = c["geo"], c["params"], c["sc"], c["ref"], c["rob"]
    rows = len(sc["ids"])
    assert rob["margin"] >= MARGIN, ("the case sits on the rejection point: choose other inputs", rob["margin"])
    if name == "portrait":
        pu, pv = ls.pitches(params, geo.patch, geo.img)
        assert sc["K"][0] == sc["K"][1] and pv / sc["K"][1] > pu / sc["K"][0]
    eng = ENGINES.fetch(geo.name)
    eng.set_option("robust_law", gc.ROBUST_ITERATIONS)
    v, st = ls.servo_law(eng, sc)
    det = eng.last_details(1)
    assert st == _lib.STATUS_OK
    suv = det["s_uv"][0, :rows]
    assert np.array_equal(suv[:, 0:2], c["s_star"]) and np.array_equal(suv[:, 2:4], c["s_uv"])
    assert np.array_equal(det["feat"][0, :rows, 0:1], ref["Z"])
    np.testing.assert_allclose(det["L"][0, :6, :2 * rows].T, ref["L"], rtol=0, atol=L_BAR)
    np.testing.assert_allclose(det["L"][0, 6, :2 * rows], ref["e"][:, 0], rtol=0, atol=L_BAR)
    werr = float(np.max(np.abs(det["weights"][0, :rows] - rob["w"])))
    err = rr.rel_l2(v, rob["v_c"])
    print(f"{name}: weights max abs error {werr:.2e}, v_c rel L2 {err:.2e}, against the exchanged pitches {rr.rel_l2(v, c['swapped']['v_c']):.2e}")
    assert werr <= W_BAR and not det["weights"][0, rows:].any()
    assert err <= VC_BAR
    assert int(det["info"][0, 6]) == gc.ROBUST_ITERATIONS and int(det["info"][0, 7]) == rob["n_zero"]


def _plain_law_then(c):
    """The plain law on a case's scenario with its goal depth set: (handle, last_details + v_c, status, pitches, goal table), the
    rows checked against the oracle's (gc.oracle_details: what the host test chose the case on)."""
    geo, params, sc, zg = c["geo"], c["params"], c["sc"], c["goal_depth"]
    eng = ENGINES.fetch(geo.name)
    eng.set_goal_depth(zg)
    v_c, st = ls.servo_law(eng, sc)
    assert st == _lib.STATUS_OK
    before = ls.snapshot(eng, v_c)
    want, n = gc.oracle_details(c, geo.tokens), len(sc["ids"])
    assert np.array_equal(before["selected"][0, :n], want["selected"][0, :n]) and np.array_equal(before["s_uv"][0, :n], want["s_uv"][0, :n])
    assert np.array_equal(before["feat"][0, :n, :3], want["feat"][0, :n, :3])
    pitches = ls.pitches(params, geo.patch, geo.img)
    assert pitches[1] > pitches[0]
    return eng, before, st, pitches, ls.goal_table(zg, geo.grid, geo.img, params)


def test_pose_and_homography_laws_on_portrait():
    """One case each of the two follow-on laws that take their floor from the pitches, with N = 4 re-weightings, against
    tests/pose_ref.py and tests/homography_ref.py with law_support.pitches of the portrait geometry.  In both cases the floor is
    reached and exchanging pitch_u and pitch_v gives another twist (asserted here on the device's own rows, chosen on the oracle's
    in tests/test_geometry_host.py)."""
    N = gc.LAW_ITERATIONS
    # the pose law: the goal depth is the scenario's plane, so the residuals are of the floor's size
    c = gc.pose_case()
    sc, params = c["sc"], c["params"]
    eng, before, st, pitches, table = _plain_law_then(c)
    v, info = eng.pose_velocity(sc["K"], [st], N)
    v, info = v.cpu().numpy(), ls.host(info)
    with np.errstate(all="ignore"):
        ref = pr.pose_from_details(before, 0, st, sc["K"], table, params.lambda_, N, *pitches)
        other = pr.pose_from_details(before, 0, st, sc["K"], table, params.lambda_, N, *gc.swapped_pitches(pitches))
    assert all(g >= 1e-6 for g in ref["gaps"]) and ref["edge"] >= 1e-6, ("choose other inputs", ref["gaps"], ref["edge"])
    assert np.abs(ref["v"] - other["v"]).max() > 1e-6                      # the pitches do decide this twist
    assert int(info["status"][0]) == ref["status"] == pr.OK
    assert [int(info[f][0]) for f in Engine.POSE_INFO_FIELDS] == list(ref["info"][:6])
    errs = dict(v=np.abs(v[0] - ref["v"]).max(), R=np.abs(info["R"][0] - ref["R"]).max(), t=np.abs(info["t"][0] - ref["t"]).max(),
                weights=np.abs(info["weights"][0] - ref["weights"]).max())
    print("pose law on portrait: " + ", ".join(f"{k} {e:.1e}" for k, e in errs.items()))
    assert all(e <= 1e-9 for e in errs.values()), errs
    assert abs(float(info["sigma"][0]) - ref["sigma"]) <= 1e-12
    eng.set_goal_depth(None)
    # the homography law
    c = gc.law_case()
    sc, params = c["sc"], c["params"]
    eng, before, st, pitches, table = _plain_law_then(c)
    zhat = 0.61
    v, info = eng.homography_velocity(sc["K"], [st], zhat, N)
    v, info = v.cpu().numpy(), ls.host(info)
    ref = hr.homography_from_details(before, 0, st, sc["K"], params.lambda_, zhat, N, *pitches)
    other = hr.homography_from_details(before, 0, st, sc["K"], params.lambda_, zhat, N, *gc.swapped_pitches(pitches))
    assert all(g >= 1e-4 for g in ref["ratios"]) and all(g >= 1e-6 for g in ref["gaps"]) and ref["edge"] >= 1e-6, \
        ("choose other inputs", ref["ratios"], ref["gaps"], ref["edge"])
    assert np.abs(ref["v"] - other["v"]).max() > 1e-6                      # the pitches do decide this twist
    assert int(info["status"][0]) == ref["status"] == hr.OK
    assert [int(info[f][0]) for f in Engine.HOMOGRAPHY_INFO_FIELDS] == list(ref["info"][:6])
    errs = dict(v=np.abs(v[0] - ref["v"]).max(), H=np.abs(info["H"][0] - ref["H"]).max() / max(1.0, np.abs(ref["H"]).max()),
                weights=np.abs(info["weights"][0] - ref["weights"]).max())
    print("homography law on portrait: " + ", ".join(f"{k} {e:.1e}" for k, e in errs.items()))
    assert all(e <= 1e-9 for e in errs.values()), errs
    assert abs(float(info["sigma"][0]) - ref["sigma"]) <= 1e-12
    eng.set_goal_depth(None)


# ----------------------------------------------------------------------------- 4. sub-patch offsets at the border
@pytest.mark.parametrize("name", gc.BORDER_GEOMETRIES)
def test_subpatch_offsets_at_the_border(name):
    """A given offset table moves the matches in the last column and row half a pitch outwards, onto u == u_max and v == v_max:
    outside the image, 100 m, not the first pixel of the next row (a depth in these images); those in the first column and row
    onto u == 0 and v == 0.  The pixels are tests/refine_ref.py's, rounded as the reference rounds."""
    c = gc.border_case(name)
    geo = c["geo"]
    eng = ENGINES.fetch(name)
    v, st = eng.servo_from_nn(c["nn_1"], c["nn_2"], c["sim_1"], c["depth"], c["K"], mode=_lib.SELECT_EXPLICIT, selection=[c["ids"]],
                              num_pairs=K_PAIRS, offsets=c["offsets"])
    v, det = v.cpu().numpy(), eng.last_details(1)
    _check_law(det, v, st, c["ref"], c["s_star"], c["s_uv"], K_PAIRS, (name, "border offsets"))
    assert np.array_equal(det["offsets"][0, :K_PAIRS], c["offsets"][c["ids"]])
    edge = (det["s_uv"][0, :K_PAIRS, 2] == geo.u_max) | (det["s_uv"][0, :K_PAIRS, 3] == geo.v_max)
    assert edge.sum() >= 6 and np.all(det["feat"][0, :K_PAIRS, 0][edge] == 100.0)


# ----------------------------------------------------------------------------- 5. the host-pointer path
HOST_GEOMETRIES = ("base", "ties14", "tiny", "near308")


def _law_rows(det, rows):
    """What a law of ``rows`` pairs wrote of ``Engine.last_details``' arrays (the rows behind them belong to earlier calls)."""
    cut = dict(selected=rows, s_uv=rows, feat=rows, weights=rows, offsets=rows, Z_goal=rows)
    out = {k: (v[:, :cut[k]] if k in cut else v) for k, v in det.items()}
    out["L"] = det["L"][:, :, :2 * rows]
    return out


@pytest.mark.parametrize("name", HOST_GEOMETRIES)
def test_host_pointer_calls_equal_device_pointer_calls(name):
    """A 2-block model with synthetic weights at the geometry.  vitvs_compute_velocity hands over only the depth pixels the law can
    read (the host's restatement of the token-to-pixel map, plus pixel (0, 0) for zero-padded rows): DENSE and ORDER calls, a
    reselect with 6 of 24 ids (18 padded rows), the same after a whole-image copy of ANOTHER depth image (subpatch on, then off:
    nothing stale may be read), and servo._reference_update with more pairs than candidates, on host arrays and on tensors, must
    equal the device-pointer calls bit for bit."""
    geo = gc.geometry(name)
    cfg, params = geo.vit_config(), geo.params(use_feature_binning=False)
    rng = np.random.default_rng(9900 + list(gc.GEOMETRIES).index(name))
    depth, other_depth, K = gc.depth_image(geo, rng), gc.depth_image(geo, rng, level=137), gc.intrinsics(geo, rng)
    assert depth[0, 0] != 0 and other_depth[0, 0] not in (0, depth[0, 0])
    des, cur = synth.frame_pair(cfg.img_size, 20250705)
    order = rng.permutation(geo.tokens).astype(np.int32)
    eng = Engine(cfg, params, precision="fp32", max_pairs=1, max_rows=geo.tokens).load_state_dict(weights.synthetic_state_dict(cfg, 3))
    try:
        for mode, sel in ((_lib.SELECT_DENSE, None), (_lib.SELECT_ORDER, order)):
            v_d, st_d = eng.compute_velocity(cur, des, depth, K, mode=mode, selection=sel, num_pairs=K_PAIRS)
            det_d = eng.last_details(1)
            v_h, st_h = eng.compute_velocity_host(cur, des, depth, K, mode=mode, selection=sel, num_pairs=K_PAIRS)
            det_h = eng.last_details(1)
            assert int(st_d[0]) == _lib.STATUS_OK == int(st_h[0]), (name, mode, int(st_d[0]), int(st_h[0]))
            assert np.array_equal(v_h[0], v_d.cpu().numpy()[0]), (name, mode)
            assert ls.same_values(det_h, det_d), (name, mode, [k for k in det_d if not np.array_equal(det_d[k], det_h[k], equal_nan=True)])
        mutual = np.nonzero(det_d["nn_2"][0][det_d["nn_1"][0]] == np.arange(geo.tokens))[0]
        assert gc.LIVE <= len(mutual) < geo.tokens
        ids = mutual[:: len(mutual) // gc.LIVE][:gc.LIVE].astype(np.int32)
        v_e, st_e = eng.compute_velocity(cur, des, depth, K, mode=_lib.SELECT_EXPLICIT, selection=[ids], num_pairs=K_PAIRS)
        v_e, det_e = v_e.cpu().numpy()[0], eng.last_details(1)
        assert int(st_e[0]) == _lib.STATUS_OK and int(det_e["info"][0, 3]) == gc.LIVE
        assert np.all(det_e["feat"][0, gc.LIVE:K_PAIRS, 0] == depth[0, 0] / 1000.0)          # the padded rows read depth[0, 0]

        def reselected(what):
            eng.compute_velocity_host(cur, des, depth, K, mode=_lib.SELECT_ORDER, selection=order, num_pairs=K_PAIRS)
            v_r, st_r = eng.reselect_host(_lib.SELECT_EXPLICIT, [ids], num_pairs=K_PAIRS)
            det_r = eng.last_details(1)
            assert int(st_r[0]) == int(st_e[0]), (name, what)
            assert np.array_equal(det_r["feat"][0, :K_PAIRS], det_e["feat"][0, :K_PAIRS]), \
                (name, what, "Z of the padded rows", det_r["feat"][0, gc.LIVE, 0], "for", depth[0, 0] / 1000.0)
            assert np.array_equal(v_r[0], v_e), (name, what)
            assert ls.same_values(_law_rows(det_r, K_PAIRS), _law_rows(det_e, K_PAIRS)), (name, what)
        reselected("reselect")
        eng.set_option("subpatch", 1)                         # a refined match can lie on any pixel: the whole image is copied
        eng.compute_velocity_host(cur, des, other_depth, K, mode=_lib.SELECT_ORDER, selection=order, num_pairs=K_PAIRS)
        eng.set_option("subpatch", 0)
        reselected("reselect after a whole-image copy of another depth image")
        # the production seam: the reference's draw between the correspondence and the law, more pairs than candidates
        k = geo.tokens
        v_host, st_host = servo._reference_update(eng, cur[None], des[None], depth[None], K, torch.Generator().manual_seed(5), k)
        tab = eng.last_tables(1)
        candidates = int(np.count_nonzero(tab["nn_2"][0][tab["nn_1"][0]] == np.arange(geo.tokens)))
        assert 4 <= candidates < k
        v_dev, st_dev = servo._reference_update(eng, torch.from_numpy(cur[None]), torch.from_numpy(des[None]), torch.from_numpy(depth[None]),
                                                K, torch.Generator().manual_seed(5), k)
        assert int(st_host[0]) == int(st_dev[0]) == _lib.STATUS_OK
        assert np.array_equal(v_host, v_dev), (name, v_host, v_dev)
    finally:
        eng.close()


# ----------------------------------------------------------------------------- 6. shapes
def test_a_transposed_depth_image_is_refused():
    """[u_max, v_max] has the right number of pixels and the wrong rows: every call that takes a depth image says so, by its shape
    message, on a handle WITH weights, where nothing else stands in the call's way: the same calls with the image transposed back,
    [v_max, u_max], run and return a twist."""
    geo = gc.geometry("portrait")
    cfg, params = geo.vit_config(), geo.params(use_feature_binning=False)
    good = gc.depth_image(geo, np.random.default_rng(9990))
    wrong = np.ascontiguousarray(good.T)
    assert wrong.shape == (geo.u_max, geo.v_max) != good.shape and wrong.size == good.size
    K = gc.intrinsics(geo)
    des, cur = synth.frame_pair(cfg.img_size, 20250705)
    says_shape = r"\[v_max, u_max\]"
    eng = Engine(cfg, params, precision="fp32", max_pairs=1, max_rows=geo.tokens).load_state_dict(weights.synthetic_state_dict(cfg, 3))
    try:
        for z in (wrong, wrong[None]):
            with pytest.raises(VitvsError, match=says_shape):
                eng.compute_velocity(cur, des, z, K, num_pairs=K_PAIRS)
            with pytest.raises(VitvsError, match=says_shape):
                eng.compute_velocity_host(cur, des, z, K, num_pairs=K_PAIRS)
            with pytest.raises(VitvsError, match=says_shape):
                eng.set_goal_depth(z)
        for z in (good, good[None]):
            v_d, st_d = eng.compute_velocity(cur, des, z, K, num_pairs=K_PAIRS)
            v_h, st_h = eng.compute_velocity_host(cur, des, z, K, num_pairs=K_PAIRS)
            assert int(st_d[0]) == _lib.STATUS_OK == int(st_h[0])
            assert v_h[0].any() and np.array_equal(v_h[0], v_d.cpu().numpy()[0])
            eng.set_goal_depth(z)
        eng.set_goal_depth(None)
    finally:
        eng.close()
