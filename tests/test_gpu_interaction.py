"""The desired and mean interaction matrices of the control law (option ``interaction``: servo_kernel<., ., GOALZ>) on the GPU
against their fp64 numpy statement (tests/interaction_ref.py).

Tiny weight-less handles through ``vitvs_servo_from_nn[_ex]_dev`` in EXPLICIT mode, in the style of tests/test_gpu_robust_law.py
(shared helpers: tests/law_support.py): both modes on both sides of the LDS / global-workspace edge (R = 2 * pairs <= 128
keeps L in LDS), both solvers, zero padding, the same-image shortcut, the statuses that skip the law, a DENSE selection at
T = 1024, the quarter turn about the optical axis, the depth requirements and error returns of each mode, composition with ``robust_law`` and with a
given offset table, "off means off", and every entry point of a ViT-S/16 handle.  The bars are the plain law's: s_uv, Z and Z*
exact, L / e within 1e-13, v_c within 1e-9 (relative L2)."""
import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib, config, synth, weights
from vitvs_amd.engine import Engine, VitvsError
from oracle import servo_ref as sr
import interaction_ref as ir
import refine_ref as rf
import robust_ref as rr
import law_support as ls
from law_support import TinyEngines, close_engines  # noqa: F401

pytestmark = pytest.mark.gpu

ENGINES = TinyEngines()           # this module's tiny handles: close_engines closes them at its teardown

LDLT = -1
MAX_SWEEPS = 40
VC_BAR, L_BAR, W_BAR = 1e-9, 1e-13, 1e-9
MARGIN = 1e-6
OPTION = {"current": 0, "desired": 1, "mean": 2}
GOAL_MODES = ("desired", "mean")


def _features(g, img, params, nn1, ids, rows):
    ids = np.asarray(ids, np.int64)
    p1 = torch.from_numpy(np.stack([ids // g, ids % g], 1))
    p2 = torch.from_numpy(np.stack([nn1[ids] // g, nn1[ids] % g], 1))
    s_star, s_ = sr.calculate_uv(sr.patch_centres(p1, img, g), sr.patch_centres(p2, img, g), rows, params.u_max, params.v_max, img)
    return np.asarray(s_star), np.asarray(s_)


def _check_law(det, b, v, st, ref, s_star, s_, rows, mode, what, solver=None):
    """One pair's law against the reference's: pixels, Z and Z* exact, L / e within 1e-13, v_c within 1e-9; the solver it names."""
    assert int(st) == _lib.STATUS_OK, (what, int(st))
    info = det["info"][b]
    assert int(info[5]) == 2 * rows, (what, info)
    suv = det["s_uv"][b, :rows]
    assert np.array_equal(suv[:, 0:2], s_star) and np.array_equal(suv[:, 2:4], s_), what
    assert np.array_equal(det["Z_goal"][b, :rows, None], ref["Z_goal"]), what
    assert not det["Z_goal"][b, rows:].any(), what
    # feat[..][0]: Z in the mean mode, Z* in the desired mode (which never reads the current depth)
    assert np.array_equal(det["feat"][b, :rows, 0:1], ref["Z"] if mode == "mean" else ref["Z_goal"]), what
    assert np.array_equal(det["feat"][b, :rows, 1:3], ref["s_xy"]), what
    lerr = float(np.max(np.abs(det["L"][b, :6, :2 * rows].T - ref["L"])))
    eerr = float(np.max(np.abs(det["L"][b, 6, :2 * rows] - ref["e"][:, 0])))
    err = rr.rel_l2(v, ref["v_c"])
    print(f"{what}: L max abs error {lerr:.2e}, e {eerr:.2e}, v_c rel L2 {err:.2e}, solver {int(info[4])}")
    assert lerr <= L_BAR and eerr <= L_BAR, (what, lerr, eerr)
    assert err <= VC_BAR, (what, err)
    if solver is not None:
        Lw = ref["L"] if "rob" not in ref else np.sqrt(np.repeat(ref["rob"]["w"], 2))[:, None] * ref["L"]
        assert (ls.ldlt_passes(Lw) == (solver == "ldlt")), (what, "the case does not reach the solver it names")
        if solver == "ldlt":
            assert int(info[4]) == LDLT, (what, "expected LDL^T", info)
        else:
            assert 0 <= int(info[4]) <= MAX_SWEEPS, (what, "expected Jacobi", info)


def _run(eng, mode, sc, goal_depth, num_pairs=None, ids=None, depth="scenario", offsets=None, select=_lib.SELECT_EXPLICIT):
    eng.set_option("interaction", OPTION[mode])
    if goal_depth is not None:
        eng.set_goal_depth(goal_depth)
    ids = sc["ids"] if ids is None else ids
    k = len(sc["ids"]) if num_pairs is None else num_pairs
    z = sc["depth"] if isinstance(depth, str) else depth
    v, st = eng.servo_from_nn(sc["nn_1"], sc["nn_2"], sc["sim_1"], z, sc["K"], mode=select,
                              selection=[ids] if select == _lib.SELECT_EXPLICIT else ids, num_pairs=k, offsets=offsets)
    return v.cpu().numpy(), st, eng.last_details(1)


def _scenario(seed, num_pairs, g=14, max_rows=130, share=0.125):
    eng, params = ENGINES.fetch(g, max(max_rows, 130), reset=("robust_law",))
    rng = np.random.default_rng(seed)
    sc = rr.planted_scenario(rng, num_pairs, share, params, K=ls.intrinsics(rng, params), g=g, holes=True)
    return eng, params, sc, ls.goal_depth(rng)


# ----------------------------------------------------------------------------- equality with the reference
@pytest.mark.parametrize("mode", GOAL_MODES)
@pytest.mark.parametrize("num_pairs", [8, 24, 64, 65, 130])
def test_modes_equal_the_reference(num_pairs, mode):
    """8 .. 64 pairs: L in LDS; 65 and 130: in the global workspace.  Holes in both depth images, random intrinsics."""
    eng, params, sc, zg = _scenario(51000 + 10 * num_pairs + OPTION[mode], num_pairs)
    s_star, s_, _ = rr.oracle_law(sc, params)
    ref = ir.law(s_star, s_, sc["depth"], zg, sc["K"], params.lambda_, mode)
    assert np.any(ref["Z_goal"] == 100.0) or num_pairs < 24                       # holes do occur under the goal features
    v, st, det = _run(eng, mode, sc, zg)
    _check_law(det, 0, v, st, ref, s_star, s_, num_pairs, mode, (mode, num_pairs), "ldlt")
    cur = ir.law(s_star, s_, sc["depth"], zg, sc["K"], params.lambda_, "current")
    assert rr.rel_l2(v, cur["v_c"]) > 1e-3                                        # and it is not the current law


# ----------------------------------------------------------------------------- both solvers
@pytest.mark.parametrize("mode", GOAL_MODES)
@pytest.mark.parametrize("num_pairs,solver", [(24, "jacobi"), (65, "jacobi"), (24, "ldlt"), (65, "ldlt")])
def test_both_solvers(num_pairs, solver, mode):
    """A rank-deficient L in every mode: the selection names two goal tokens only (the first over and over, the second in the last
    four rows) and each has one match, so L(s, Z), L(s*, Z*) and their mean all have two distinct pairs of rows (rank 4), in LDS
    (24 pairs) and in the global workspace (65).  Distinct mutual tokens are LDL^T."""
    g, max_rows = 17, 80
    t = g * g
    rng = np.random.default_rng(300 * num_pairs + 7 * OPTION[mode] + (solver == "jacobi"))
    eng, params = ENGINES.fetch(g, max_rows, reset=("robust_law",))
    nn1, nn2, sim1, mutual = ls.tables(rng, t, 200)
    depth, zg, K = ls.depth(rng), ls.goal_depth(rng), ls.intrinsics(rng, params)
    if solver == "ldlt":
        ids = rng.choice(mutual, size=num_pairs, replace=False)
    else:
        a, b = rng.choice(t, size=2, replace=False)
        ids = np.full(num_pairs, a)
        ids[-4:] = b
    ids = ids.astype(np.int32)
    sc = dict(nn_1=nn1, nn_2=nn2, sim_1=sim1, depth=depth, K=K, ids=ids)
    v, st, det = _run(eng, mode, sc, zg)
    s_star, s_ = _features(g, 16 * g, params, nn1, ids, num_pairs)
    ref = ir.law(s_star, s_, depth, zg, K, params.lambda_, mode)
    assert solver == "ldlt" or np.linalg.matrix_rank(ref["L"]) == 4
    _check_law(det, 0, v, st, ref, s_star, s_, num_pairs, mode, (mode, num_pairs, solver), solver)


# ----------------------------------------------------------------------------- zero padding, same image, skipped laws
@pytest.mark.parametrize("mode", GOAL_MODES)
def test_zero_padded_rows(mode):
    """10 live pairs of 24: the padded rows are pairs at pixel (0, 0) on both sides, Z* read at pixel (0, 0) — once a depth, once a hole."""
    eng, params, sc, zg = _scenario(52000 + OPTION[mode], 24)
    n_live = 10
    s_star, s_, _ = rr.oracle_law(sc, params, n_live=n_live, rows=24)
    assert not s_star[n_live:].any() and not s_[n_live:].any()
    for corner in (1234, 0):
        zg[0, 0] = corner
        ref = ir.law(s_star, s_, sc["depth"], zg, sc["K"], params.lambda_, mode)
        assert np.all(ref["Z_goal"][n_live:] == (corner / 1000.0 if corner else 100.0))
        v, st, det = _run(eng, mode, sc, zg, num_pairs=24, ids=sc["ids"][:n_live])
        assert int(det["info"][0, 3]) == n_live and int(det["info"][0, 1]) == 24
        _check_law(det, 0, v, st, ref, s_star, s_, 24, mode, (mode, "padded", corner))


@pytest.mark.parametrize("mode", GOAL_MODES)
def test_same_image_and_skipped_laws(mode):
    g, k = 14, 24
    t = g * g
    eng, params = ENGINES.fetch(g, 130, reset=("robust_law",))
    rng = np.random.default_rng(53 + OPTION[mode])
    nn1, nn2, sim1, mutual = ls.tables(rng, t, t // 3)
    depth, zg, K = ls.depth(rng), ls.goal_depth(rng), params.intrinsics()
    order = rng.permutation(t).astype(np.int32)
    sc = dict(nn_1=nn1, nn_2=nn2, sim_1=np.ones(t, np.float32), depth=depth, K=K, ids=order)
    v, st, det = _run(eng, mode, sc, zg, num_pairs=k, select=_lib.SELECT_ORDER)
    assert int(st) == _lib.STATUS_OK and int(det["info"][0, 2]) == 1 and np.all(v == 0)          # exact zeros
    assert np.array_equal(det["s_uv"][0, :k, 0:2], det["s_uv"][0, :k, 2:4]) and not det["L"][0, 6].any()
    assert np.array_equal(det["Z_goal"][0, :k, None], sr.get_depth(zg, det["s_uv"][0, :k, 0:2]))
    # fewer than 4 matches of a short selection
    sc["sim_1"] = sim1
    few = rng.choice(mutual, size=3, replace=False).astype(np.int32)
    v, st, det = _run(eng, mode, sc, None, num_pairs=k, ids=few)
    assert int(st) == _lib.STATUS_TOO_FEW and np.all(v == 0) and not det["s_uv"][0].any()
    # every token mutual: the reference's filter returns nothing
    ident = dict(sc, nn_1=np.arange(t), nn_2=np.arange(t), sim_1=np.full(t, 0.5, np.float32))
    v, st, det = _run(eng, mode, ident, None, num_pairs=k, ids=order, select=_lib.SELECT_ORDER)
    assert int(st) == _lib.STATUS_NO_CORRESPONDENCE and np.all(v == 0)
    # the statuses are the current law's
    for name, s, sel, ids in (("few", sc, _lib.SELECT_EXPLICIT, few), ("none", ident, _lib.SELECT_ORDER, order)):
        v0, st0, d0 = _run(eng, "current", s, None, num_pairs=k, ids=ids, select=sel)
        v1, st1, d1 = _run(eng, mode, s, None, num_pairs=k, ids=ids, select=sel)
        assert int(st0) == int(st1) and np.array_equal(v0, v1) and np.array_equal(d0["info"], d1["info"]), name


def test_depth_requirements_of_each_mode():
    """desired: the current depth is never read, none is needed; mean: NO_DEPTH without it, as the current law."""
    eng, params, sc, zg = _scenario(54000, 24)
    s_star, s_, _ = rr.oracle_law(sc, params)
    ref = ir.law(s_star, s_, None, zg, sc["K"], params.lambda_, "desired")
    v, st, det = _run(eng, "desired", sc, zg, depth=None)
    _check_law(det, 0, v, st, ref, s_star, s_, 24, "desired", "desired without Z", "ldlt")
    v_with, st_with, det_with = _run(eng, "desired", sc, zg)
    assert np.array_equal(v, v_with) and np.array_equal(det["L"], det_with["L"]) and np.array_equal(det["feat"], det_with["feat"])
    v, st, det = _run(eng, "mean", sc, zg, depth=None)
    assert int(st) == _lib.STATUS_NO_DEPTH and np.all(v == 0)
    v, st, det = _run(eng, "current", sc, zg, depth=None)
    assert int(st) == _lib.STATUS_NO_DEPTH and np.all(v == 0)


def test_error_returns():
    img = 224
    params = config.ServoParams(dino_input_size=img)
    eng = Engine(ls.tiny_cfg(img), params, precision="fp32", max_pairs=2, max_rows=48)
    rng = np.random.default_rng(55)
    sc = rr.planted_scenario(rng, 24, 0.0, params, holes=True)
    zg = ls.goal_depth(rng)
    for mode in GOAL_MODES:                                  # no goal depth in the handle
        with pytest.raises(VitvsError, match=r"\(-5\)"):
            _run(eng, mode, sc, None)
    v, st, _ = _run(eng, "current", sc, None)               # the current law needs none
    assert int(st) == _lib.STATUS_OK
    eng.set_goal_depth(np.stack([zg, zg]))                   # two images for a call of one pair
    for mode in GOAL_MODES:
        with pytest.raises(VitvsError, match=r"\(-5\)"):
            _run(eng, mode, sc, None)
    v1, st1, _ = _run(eng, "mean", sc, zg)                   # one image pairs with it
    assert int(st1) == _lib.STATUS_OK
    eng.set_goal_depth(None)                                 # cleared: as if never set
    with pytest.raises(VitvsError, match=r"\(-5\)"):
        _run(eng, "mean", sc, None)
    with pytest.raises(VitvsError, match=r"\(-3\)"):
        eng.set_goal_depth(np.stack([zg, zg, zg]))           # more than max_pairs
    with pytest.raises(VitvsError):
        eng.set_goal_depth(zg[:100])                         # not a depth image of this camera
    for bad in (3, -1):
        with pytest.raises(VitvsError, match=r"\(-5\)"):
            eng.set_option("interaction", bad)
    eng.close()


# ----------------------------------------------------------------------------- DENSE
@pytest.mark.parametrize("mode", GOAL_MODES)
def test_dense_selection_at_1024_tokens(mode):
    """Every mutual token (a few hundred) enters the law: L in the global workspace, Z* from a table of 1025 entries."""
    g = 32
    t = g * g
    eng, params = ENGINES.fetch(g, t, reset=("robust_law",))
    rng = np.random.default_rng(4300 + OPTION[mode])
    nn1, nn2, sim1, mutual = ls.tables(rng, t, 300)
    depth, zg, K = ls.depth(rng), ls.goal_depth(rng), ls.intrinsics(rng, params)
    sc = dict(nn_1=nn1, nn_2=nn2, sim_1=sim1, depth=depth, K=K, ids=None)
    v, st, det = _run(eng, mode, sc, zg, num_pairs=24, select=_lib.SELECT_DENSE)
    rows = int(det["info"][0, 3])
    ids = det["selected"][0, :rows]
    assert rows == len(mutual) > 128 and ids.tolist() == mutual.tolist()
    s_star, s_ = _features(g, 16 * g, params, nn1, ids, rows)
    ref = ir.law(s_star, s_, depth, zg, K, params.lambda_, mode)
    _check_law(det, 0, v, st, ref, s_star, s_, rows, mode, (mode, "dense", rows), "ldlt")


# ----------------------------------------------------------------------------- the quarter turn
def test_quarter_turn_about_the_optical_axis():
    """tests/test_interaction_host.py's case on the device: nn_1 is the rotation permutation of the 14 x 14 grid, nn_2 its inverse
    except at three unselected tokens; the device equals the reference and the properties hold on the device's own values."""
    case = ir.quarter_turn_case()
    eng, params = ENGINES.fetch(case["g"], 130, lam=case["lam"], reset=("robust_law",))
    laws = ir.quarter_turn_laws(case)
    vz = {}
    for mode in ir.MODES:
        v, st, det = _run(eng, mode, case, case["goal_depth"])
        assert int(det["info"][0, 0]) == case["g"] ** 2 - 3                      # n_mutual < T
        if mode == "current":
            assert int(st) == _lib.STATUS_OK and rr.rel_l2(v, laws[mode]["v_c"]) <= VC_BAR and not det["Z_goal"].any()
            assert np.max(np.abs(det["L"][0, :6, :48].T - laws[mode]["L"])) <= L_BAR
        else:
            _check_law(det, 0, v, st, laws[mode], case["s_uv_star"], case["s_uv"], 24, mode, ("quarter turn", mode), "ldlt")
        print(f"device, quarter turn, {mode:8s}: v_z = {v[2]:+.4f}  w_z = {v[5]:+.4f}")
        vz[mode] = v
    ir.quarter_turn_properties(vz["current"][2], vz["desired"][2], vz["mean"][2])
    assert vz["current"][2] < 0 < vz["desired"][2] and abs(vz["mean"][5]) > 1.5 * abs(vz["current"][5])


# ----------------------------------------------------------------------------- composition
@pytest.mark.parametrize("mode", GOAL_MODES)
@pytest.mark.parametrize("num_pairs", [24, 65])
def test_with_the_robust_law(num_pairs, mode):
    """robust_law = 4 on the mode's L: the residuals e_k - L_k x use the matrix the mode built."""
    eng, params, sc, zg = _scenario(56000 + 10 * num_pairs + OPTION[mode], num_pairs, share=0.25 if num_pairs >= 48 else 0.125)
    s_star, s_, _ = rr.oracle_law(sc, params)
    ref = ir.law(s_star, s_, sc["depth"], zg, sc["K"], params.lambda_, mode, robust=4, s_min=ls.s_min(params, sc["img"], sc["K"]))
    rob = ref["rob"]
    assert rob["margin"] >= MARGIN, ("the case sits on the rejection point: choose other inputs", rob["margin"])
    eng.set_option("interaction", OPTION[mode])                                   # (_servo_engine reset robust_law to 0)
    eng.set_option("robust_law", 4)
    eng.set_goal_depth(zg)
    v, st = eng.servo_from_nn(sc["nn_1"], sc["nn_2"], sc["sim_1"], sc["depth"], sc["K"], mode=_lib.SELECT_EXPLICIT,
                              selection=[sc["ids"]], num_pairs=num_pairs)
    det = eng.last_details(1)
    eng.set_option("robust_law", 0)
    _check_law(det, 0, v.cpu().numpy(), st, ref, s_star, s_, num_pairs, mode, (mode, "robust", num_pairs), "ldlt")
    werr = float(np.max(np.abs(det["weights"][0, :num_pairs] - rob["w"])))
    assert werr <= W_BAR and int(det["info"][0, 6]) == 4 and int(det["info"][0, 7]) == rob["n_zero"], (werr, det["info"][0], rob["n_zero"])
    plain = ir.law(s_star, s_, sc["depth"], zg, sc["K"], params.lambda_, mode)
    assert rr.rel_l2(v.cpu().numpy(), plain["v_c"]) > 1e-3                        # the weights do change the twist


@pytest.mark.parametrize("mode", GOAL_MODES)
@pytest.mark.parametrize("num_pairs", [24, 65])
def test_with_a_given_offset_table(num_pairs, mode):
    """Sub-patch offsets move the CURRENT side only: the goal side, and with it Z*, stay at the patch centres."""
    eng, params, sc, zg = _scenario(57000 + 10 * num_pairs + OPTION[mode], num_pairs, share=0.0)
    rng = np.random.default_rng(num_pairs)
    table = rng.uniform(-0.5, 0.5, size=(sc["g"] ** 2, 2)).astype(np.float32)
    s_star, s_ = rf.refined_features(sc["ids"], sc["nn_1"], table, sc["img"], sc["g"], params.u_max, params.v_max, rows=num_pairs)
    s_star, s_ = np.asarray(s_star), np.asarray(s_)
    s_star_plain, s_plain, _ = rr.oracle_law(sc, params)
    assert np.array_equal(s_star, s_star_plain) and np.count_nonzero(np.any(s_ != s_plain, axis=1)) >= num_pairs // 2
    ref = ir.law(s_star, s_, sc["depth"], zg, sc["K"], params.lambda_, mode)
    v, st, det = _run(eng, mode, sc, zg, offsets=table)
    _check_law(det, 0, v, st, ref, s_star, s_, num_pairs, mode, (mode, "offsets", num_pairs), "ldlt")
    assert np.array_equal(det["offsets"][0, :num_pairs], table[sc["ids"]])


# ----------------------------------------------------------------------------- off means off
def test_off_means_off():
    """Option 0 with a goal depth in the handle: v_c, every detail and the weights are those of a handle that never saw the feature,
    bit for bit; Z_goal is all zero."""
    img = 224
    params = config.ServoParams(dino_input_size=img)
    rng = np.random.default_rng(58)
    sc = rr.planted_scenario(rng, 24, 0.125, params, holes=True)
    zg = ls.goal_depth(rng)

    def run(eng):
        v, st = eng.servo_from_nn(sc["nn_1"], sc["nn_2"], sc["sim_1"], sc["depth"], sc["K"], mode=_lib.SELECT_EXPLICIT,
                                  selection=[sc["ids"]], num_pairs=24)
        return v.cpu().numpy(), int(st), eng.last_details(1)
    fresh = Engine(ls.tiny_cfg(img), params, precision="fp32", max_pairs=1, max_rows=48)      # never saw the feature
    v0, st0, d0 = run(fresh)
    fresh.close()
    eng = Engine(ls.tiny_cfg(img), params, precision="fp32", max_pairs=1, max_rows=48)
    eng.set_goal_depth(zg)
    v1, st1, d1 = run(eng)                                                                  # a goal depth, option never set
    eng.set_option("interaction", 2)
    v2, st2, d2 = run(eng)
    eng.set_option("interaction", 0)
    v3, st3, d3 = run(eng)                                                                  # switched on and off again
    assert st0 == st1 == st2 == st3 == _lib.STATUS_OK
    for v, d in ((v1, d1), (v3, d3)):
        assert np.array_equal(v, v0)
        assert sorted(d) == sorted(d0)
        for key in d0:
            assert np.array_equal(d[key], d0[key]), key
        assert not d["Z_goal"].any() and np.all(d["weights"][0, :24] == 1.0)
    assert not np.array_equal(v2, v0) and d2["Z_goal"][0, :24].all() and not np.array_equal(d2["L"], d0["L"])
    _, _, ref = rr.oracle_law(sc, params)
    assert rr.rel_l2(v0, ref["v_c"]) <= VC_BAR
    eng.close()


# ----------------------------------------------------------------------------- every entry point (ViT-S/16)
def _vits16(interaction, max_pairs=1):
    cfg = config.baseline_config("vits16_224")
    params = config.ServoParams(dino_input_size=cfg.img_size, use_feature_binning=False, interaction=interaction)
    return cfg, params, weights.synthetic_state_dict(cfg, 0)


@pytest.mark.parametrize("mode", GOAL_MODES)
def test_every_entry_point_evaluates_the_mode(mode):
    cfg, params, sd = _vits16(mode)
    eng = Engine(cfg, params, precision="fp32", max_pairs=2).load_state_dict(sd)           # the option comes from the params
    des, cur = synth.frame_pair(cfg.img_size, 20250705)
    rng = np.random.default_rng(59)
    depth, K = synth.depth_pattern(), params.intrinsics()
    zg, zg2 = ls.goal_depth(rng), ls.goal_depth(rng)
    k, g = params.num_pairs, cfg.grid
    identity = np.arange(cfg.tokens, dtype=np.int32)
    with pytest.raises(VitvsError, match=r"\(-5\)"):                                       # no goal depth yet: every entry point refuses
        eng.compute_velocity(cur, des, depth, K, mode=_lib.SELECT_ORDER, selection=identity)
    with pytest.raises(VitvsError, match=r"\(-5\)"):
        eng.compute_velocity_host(cur, des, depth, K, mode=_lib.SELECT_ORDER, selection=identity)
    eng.set_goal_depth(zg)
    eng.compute_velocity(cur, des, depth, K, mode=_lib.SELECT_ORDER, selection=identity)
    tabs = eng.last_details(1)
    nn1 = tabs["nn_1"][0].astype(np.int64)
    mutual = np.nonzero(tabs["nn_2"][0][nn1] == np.arange(cfg.tokens))[0]
    ids = mutual[:: max(1, len(mutual) // k)][:k].astype(np.int32)

    def reference(goal):
        s_star, s_ = _features(g, cfg.img_size, params, nn1, ids, k)
        return s_star, s_, ir.law(s_star, s_, depth, goal, K, params.lambda_, mode)
    s_star, s_, ref = reference(zg)
    # the device-pointer call
    v_dev, st_dev = eng.compute_velocity(cur, des, depth, K, mode=_lib.SELECT_EXPLICIT, selection=[ids])
    det = eng.last_details(1)
    v_dev = v_dev.cpu().numpy()[0]
    _check_law(det, 0, v_dev, st_dev[0], ref, s_star, s_, k, mode, (mode, "compute_velocity_dev"), "ldlt")
    # the host-pointer call and the reselect seam
    v_host, st_host = eng.compute_velocity_host(cur, des, depth, K, mode=_lib.SELECT_EXPLICIT, selection=[ids])
    assert int(st_host[0]) == _lib.STATUS_OK and np.array_equal(v_host[0], v_dev)
    assert np.array_equal(eng.last_goal_depth(1), det["Z_goal"])
    eng.compute_velocity_host(cur, des, depth, K, mode=_lib.SELECT_ORDER, selection=identity)
    v_re, st_re = eng.reselect_host(_lib.SELECT_EXPLICIT, [ids])
    assert int(st_re[0]) == _lib.STATUS_OK and np.array_equal(v_re[0], v_dev)
    # without a run-time depth image
    v_nz, st_nz = eng.compute_velocity_host(cur, des, None, K, mode=_lib.SELECT_EXPLICIT, selection=[ids])
    v_nd, st_nd = eng.compute_velocity(cur, des, None, K, mode=_lib.SELECT_EXPLICIT, selection=[ids])
    if mode == "desired":
        assert int(st_nz[0]) == int(st_nd[0]) == _lib.STATUS_OK and np.array_equal(v_nz[0], v_dev)
        assert np.array_equal(v_nd.cpu().numpy()[0], v_dev)
    else:
        assert int(st_nz[0]) == int(st_nd[0]) == _lib.STATUS_NO_DEPTH and not v_nz.any()
    # the tables' seam
    v_nn, st_nn = eng.servo_from_nn(tabs["nn_1"][0], tabs["nn_2"][0], tabs["sim_1"][0], depth, K, mode=_lib.SELECT_EXPLICIT,
                                    selection=[ids], num_pairs=k)
    assert int(st_nn) == _lib.STATUS_OK and np.array_equal(v_nn.cpu().numpy(), v_dev)
    # two pairs: one shared goal image serves both, as two copies of it do
    two = lambda a: np.stack([a, a])   # noqa: E731
    v_sh, st_sh = eng.compute_velocity(two(cur), two(des), two(depth), K, mode=_lib.SELECT_EXPLICIT, selection=[ids, ids])
    d_sh = eng.last_details(2)
    eng.set_goal_depth(two(zg))
    v_2, st_2 = eng.compute_velocity(two(cur), two(des), two(depth), K, mode=_lib.SELECT_EXPLICIT, selection=[ids, ids])
    d_2 = eng.last_details(2)
    assert np.array_equal(v_sh.cpu().numpy(), v_2.cpu().numpy()) and np.array_equal(d_sh["Z_goal"], d_2["Z_goal"])
    assert np.array_equal(d_sh["Z_goal"][0], d_sh["Z_goal"][1]) and np.array_equal(d_sh["Z_goal"][0], det["Z_goal"][0])
    for b in range(2):
        assert rr.rel_l2(v_sh.cpu().numpy()[b], ref["v_c"]) <= VC_BAR and int(st_sh[b]) == _lib.STATUS_OK
    eng.set_goal_depth(np.stack([zg, zg2]))                                                 # one image per pair
    v_pp, _ = eng.compute_velocity(two(cur), two(des), two(depth), K, mode=_lib.SELECT_EXPLICIT, selection=[ids, ids])
    ref2 = reference(zg2)[2]
    assert rr.rel_l2(v_pp.cpu().numpy()[0], ref["v_c"]) <= VC_BAR and rr.rel_l2(v_pp.cpu().numpy()[1], ref2["v_c"]) <= VC_BAR
    with pytest.raises(VitvsError, match=r"\(-5\)"):                                        # two images, one pair
        eng.compute_velocity(cur, des, depth, K, mode=_lib.SELECT_EXPLICIT, selection=[ids])
    # graph replay equals eager bit for bit, and again after the goal depth is rewritten in place (a device tensor, in stream order)
    eng.set_goal_depth(zg)
    eng.set_option("graph_replay", 1)
    cur_d, des_d = eng._frames(cur), eng._frames(des)
    z_d = torch.as_tensor(depth).reshape(1, params.v_max, params.u_max).to(eng.device).contiguous()
    k_d = torch.as_tensor(K, dtype=torch.float64).reshape(1, 4).to(eng.device)
    sel_d, cnt_d = eng._selection_args(_lib.SELECT_EXPLICIT, [ids], 1, cfg.tokens, k)
    out_v = torch.zeros((1, 6), dtype=torch.float64, device=eng.device)
    out_s = torch.zeros(1, dtype=torch.int32, device=eng.device)

    def replayed():
        eng.compute_velocity_dev(cur_d, des_d, z_d, k_d, _lib.SELECT_EXPLICIT, sel_d, cnt_d, out_v=out_v, out_status=out_s, num_pairs=k)
        torch.cuda.synchronize()
        return out_v.cpu().numpy()[0].copy()
    v_g = replayed()
    assert np.array_equal(replayed(), v_g) and np.array_equal(v_g, v_dev)
    eng.set_goal_depth(torch.as_tensor(zg2).to(eng.device))
    v_g2 = replayed()
    assert np.array_equal(eng.last_goal_depth(1)[0, :k, None], ref2["Z_goal"])
    eng.set_option("graph_replay", 0)
    v_e2, _ = eng.compute_velocity(cur, des, depth, K, mode=_lib.SELECT_EXPLICIT, selection=[ids])
    assert not np.array_equal(v_g2, v_g) and np.array_equal(v_g2, v_e2.cpu().numpy()[0]) and rr.rel_l2(v_g2, ref2["v_c"]) <= VC_BAR
    # a change of the option drops the captured update
    eng.set_option("graph_replay", 1)
    assert np.array_equal(replayed(), v_g2)
    eng.set_option("interaction", 0)
    v_g0 = replayed()
    cur_law = ir.law(s_star, s_, depth, zg2, K, params.lambda_, "current")
    assert rr.rel_l2(v_g0, cur_law["v_c"]) <= VC_BAR and not eng.last_goal_depth(1).any()
    eng.set_option("interaction", OPTION[mode])
    assert np.array_equal(replayed(), v_g2)
    eng.close()


@pytest.mark.parametrize("mode", GOAL_MODES)
def test_through_a_pipeline_slot_and_the_controllers(mode):
    """UpdatePipeline hands the option (from the params) and the goal depth to every slot; Controller and MultiController take
    ``goal_depth`` and, in the desired mode, update without a depth image."""
    from vitvs_amd.pipeline import UpdatePipeline
    from vitvs_amd.servo import Controller, MultiController
    cfg, params, sd = _vits16(mode)
    des, cur = synth.frame_pair(cfg.img_size, 20250705)
    rng = np.random.default_rng(60)
    depth, K, zg = synth.depth_pattern(), params.intrinsics(), ls.goal_depth(rng)
    order = rng.permutation(cfg.tokens).astype(np.int32)
    eng = Engine(cfg, params, precision="fp32", max_pairs=1).load_state_dict(sd)
    eng.set_goal_depth(zg)
    v_ref, st_ref = eng.compute_velocity(cur, des, depth, K, mode=_lib.SELECT_ORDER, selection=order)
    v_ref = v_ref.cpu().numpy()
    z_ref = eng.last_goal_depth(1)
    assert int(st_ref[0]) == _lib.STATUS_OK and v_ref.any()
    pipe = UpdatePipeline(cfg, params, sd, precision="fp32", depth=2, device=eng.device)
    dev = eng.device
    args = (torch.from_numpy(cur[None]).to(dev), torch.from_numpy(des[None]).to(dev), torch.from_numpy(depth[None]).to(dev),
            torch.tensor([K], dtype=torch.float64, device=dev), _lib.SELECT_ORDER, torch.from_numpy(order[None]).to(dev))
    with pytest.raises(VitvsError, match=r"\(-5\)"):
        pipe.submit(*args)
    pipe.set_goal_depth(zg)
    for _ in range(2):                                                                     # both slots, twice (the second time replayed)
        for t in [pipe.submit(*args) for _ in range(2)]:
            v, st = pipe.result(t)
            assert int(st[0]) == _lib.STATUS_OK and np.array_equal(v.cpu().numpy(), v_ref)
            assert np.array_equal(pipe.engines[t % 2].last_goal_depth(1), z_ref)
    # Controller: the goal depth through the constructor; no run-time depth image in the desired mode
    gen = lambda: torch.Generator().manual_seed(7)   # noqa: E731
    ctl = Controller(eng, des, params, selection="order", goal_depth=zg)
    ctl.generator = gen()
    ctl.image_callback_rgb(cur)
    ctl.ibvs()
    if mode == "desired":
        assert ctl.v_c is not None and ctl.last_status == _lib.STATUS_OK and ctl.v_c.any()
    else:
        assert ctl.v_c is None                                                             # the reference's "Failed to get depth - skipping"
    ctl.image_callback_depth(depth)
    ctl.generator = gen()
    ctl.ema_velocities = [None] * 6
    ctl.ibvs()
    first = ctl.v_c.copy()
    assert ctl.last_status == _lib.STATUS_OK and first.any()
    multi = MultiController(pipe, [des, des], params, selection="order", generator=gen(), goal_depth=zg)
    for i in range(2):
        multi.image_callback_rgb(i, cur)
        multi.image_callback_depth(i, depth)
    multi.ibvs()
    assert np.array_equal(multi.v_c[0], first) and multi.v_c[1] is not None
    pipe.close()
    eng.close()
