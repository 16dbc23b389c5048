"""The outlier-robust control law (option ``robust_law``: Tukey IRLS inside servo_kernel) on the GPU against its fp64 numpy
statement (tests/robust_ref.py).

Tiny handles through ``vitvs_servo_from_nn_dev`` in EXPLICIT mode, in the style of tests/test_gpu_servo_cover.py (shared
helpers: tests/law_support.py): planted-outlier scenarios on both sides of the LDS / global-workspace edge (R = 2 * pairs <= 128
keeps L and the weights in LDS), both solvers of the weighted system, the planted-outlier property on the device, zero padding, the same-image
shortcut, the statuses that skip the law, a DENSE selection at T = 1024, "off means off", and every entry point of a ViT-S/16
handle.  The bars are the plain law's: s_uv and Z exact, L / e within 1e-13, v_c within 1e-9 (relative L2); final weights
within 1e-9 absolute.  Every equality case is checked (on the reference, before the device is asked) to keep every pair's
t = rho / (c sigma) at least 1e-6 away from the rejection point 1, where the count of zero weights is not continuous."""
import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib, config, synth, weights
from vitvs_amd.engine import Engine, VitvsError
import robust_ref as rr
import law_support as ls
from law_support import TinyEngines, close_engines  # noqa: F401

pytestmark = pytest.mark.gpu

ENGINES = TinyEngines()           # this module's tiny handles: close_engines closes them at its teardown

LDLT = -1
MAX_SWEEPS = 40
VC_BAR, L_BAR, W_BAR = 1e-9, 1e-13, 1e-9
MARGIN = 1e-6


def _check_robust(det, b, v, st, ref, rob, s_star, s_, rows, n_iter, solver, what):
    """One pair's robust law against the reference's: the plain law's checks of L / e, then the weights, the twist, the
    counters and the solver of the FINAL weighted system."""
    assert int(st) == _lib.STATUS_OK, (what, int(st))
    info = det["info"][b]
    assert int(info[5]) == 2 * rows, (what, info)
    suv = det["s_uv"][b, :rows]
    assert np.array_equal(suv[:, 0:2], s_star) and np.array_equal(suv[:, 2:4], s_), what
    assert np.array_equal(det["feat"][b, :rows, 0:1], ref["Z"]), what
    np.testing.assert_allclose(det["L"][b, :6, :2 * rows].T, ref["L"], rtol=0, atol=L_BAR, err_msg=str(what))
    np.testing.assert_allclose(det["L"][b, 6, :2 * rows], ref["e"][:, 0], rtol=0, atol=L_BAR, err_msg=str(what))
    assert rob["margin"] >= MARGIN, (what, "the case sits on the rejection point: choose other inputs", rob["margin"])
    werr = float(np.max(np.abs(det["weights"][b, :rows] - rob["w"])))
    err = rr.rel_l2(v, rob["v_c"])
    print(f"{what}: weights max abs error {werr:.2e}, v_c rel L2 {err:.2e}, zero weights {rob['n_zero']}, solver {int(info[4])}")
    assert werr <= W_BAR, (what, werr)
    assert not det["weights"][b, rows:].any(), what
    assert err <= VC_BAR, (what, err)
    assert int(info[6]) == n_iter and int(info[7]) == rob["n_zero"], (what, info, rob["n_zero"])
    sw = np.sqrt(np.repeat(rob["w"], 2))[:, None]
    assert (ls.ldlt_passes(sw * ref["L"]) == (solver == "ldlt")), (what, "the case does not reach the solver it names")
    if solver == "ldlt":
        assert int(info[4]) == LDLT, (what, "expected LDL^T", info)
    else:
        assert 0 <= int(info[4]) <= MAX_SWEEPS, (what, "expected Jacobi", info)


def _run(eng, sc, n_iter, num_pairs=None, ids=None):
    eng.set_option("robust_law", n_iter)
    ids = sc["ids"] if ids is None else ids
    k = len(sc["ids"]) if num_pairs is None else num_pairs
    v, st = eng.servo_from_nn(sc["nn_1"], sc["nn_2"], sc["sim_1"], sc["depth"], sc["K"], mode=_lib.SELECT_EXPLICIT, selection=[ids],
                              num_pairs=k)
    return v.cpu().numpy(), st, eng.last_details(1)


# ----------------------------------------------------------------------------- equality with the reference
@pytest.mark.parametrize("n_iter", [1, 4, 16])
@pytest.mark.parametrize("num_pairs", [8, 24, 48, 64, 65, 130])
def test_planted_scenarios_equal_the_reference(num_pairs, n_iter):
    """8 .. 64 pairs: L and the weights in LDS; 65 and 130: in the global workspace.  Depth holes, random intrinsics."""
    eng, params = ENGINES.fetch(14, 130)
    rng = np.random.default_rng(9000 + 20 * num_pairs + n_iter)
    sc = rr.planted_scenario(rng, num_pairs, 0.25 if num_pairs >= 48 else 0.125, params, K=ls.intrinsics(rng, params), holes=True)
    s_star, s_, ref = rr.oracle_law(sc, params)
    rob = rr.robust_velocity(ref["L"], ref["e"], params.lambda_, n_iter, ls.s_min(params, sc["img"], sc["K"]))
    v, st, det = _run(eng, sc, n_iter)
    _check_robust(det, 0, v, st, ref, rob, s_star, s_, num_pairs, n_iter, "ldlt", ("planted", num_pairs, n_iter))


# ----------------------------------------------------------------------------- both solvers under weights
@pytest.mark.parametrize("num_pairs,solver", [(24, "jacobi"), (40, "jacobi"), (65, "jacobi"), (24, "ldlt"), (65, "ldlt")])
def test_both_solvers_under_weights(num_pairs, solver):
    """Rank-deficient selections (every goal token matched to one token below 32 pairs, to two tokens in two blocks from 32 on)
    fail the pivot test under any weights, so every solve — the final one included — is the Jacobi SVD on rows scaled by sqrt(w),
    in the LDS copy (24, 40 pairs) and in the global one (65); distinct mutual tokens are LDL^T."""
    g, max_rows = 17, 80
    t = g * g
    rng = np.random.default_rng(200 * num_pairs + (solver == "jacobi"))
    eng, params = ENGINES.fetch(g, max_rows)
    nn1, nn2, sim1, mutual = ls.tables(rng, t, 200)
    depth, K = ls.depth(rng), ls.intrinsics(rng, params)
    if solver == "ldlt":
        ids = rng.choice(mutual, size=num_pairs, replace=False)
    else:
        # distinct goal tokens that all have the SAME match: identical rows of L (rank 2; two matches in two blocks from 32
        # pairs on: rank 4), different errors — an inconsistent rank-deficient system, so the residuals and weights differ
        ids = rng.choice(t, size=num_pairs, replace=False)
        nn1 = nn1.copy()
        a, b = rng.choice(t, size=2, replace=False)
        nn1[ids] = a
        if num_pairs >= 32:
            nn1[ids[-4:]] = b
        n_mutual = int(np.count_nonzero(nn2[nn1] == np.arange(t)))
        assert 0 < n_mutual < t
    ids = ids.astype(np.int32)
    eng.set_option("robust_law", 4)
    v, st = eng.servo_from_nn(nn1, nn2, sim1, depth, K, mode=_lib.SELECT_EXPLICIT, selection=[ids], num_pairs=num_pairs)
    det = eng.last_details(1)
    s_star, s_, ref = ls.oracle(g, 16 * g, params, nn1, ids, num_pairs, depth, K)
    rob = rr.robust_velocity(ref["L"], ref["e"], params.lambda_, 4, ls.s_min(params, 16 * g, K))
    assert solver == "ldlt" or np.ptp(rob["w"]) > 0.05                     # the Jacobi SVD does run on unequal weights
    _check_robust(det, 0, v.cpu().numpy(), st, ref, rob, s_star, s_, num_pairs, 4, solver, (num_pairs, solver))


# ----------------------------------------------------------------------------- the property on the device
@pytest.mark.parametrize("n_pairs,share,seed0", rr.PROPERTY_CONFIGS)
def test_planted_outlier_property_on_the_device(n_pairs, share, seed0):
    """The scenarios of tests/test_robust_host.py: the device's robust twist (N = 4) is closer than half the device's plain
    twist's distance to the plain law on the un-corrupted matches, in every scenario."""
    eng, params = ENGINES.fetch(14, 130)
    errs = []
    for sc, clean in rr.property_scenarios(n_pairs, share, seed0, params):
        v_plain, st0, _ = _run(eng, sc, 0)
        v_rob, st1, _ = _run(eng, sc, 4)
        assert int(st0) == _lib.STATUS_OK and int(st1) == _lib.STATUS_OK
        errs.append((rr.rel_l2(v_plain, clean["v_c"]), rr.rel_l2(v_rob, clean["v_c"])))
    errs = np.array(errs)
    print(f"device, {n_pairs} pairs, {100 * share:.1f} % outliers: plain error median {np.median(errs[:, 0]):.3f}, robust median "
          f"{np.median(errs[:, 1]):.3f}, largest robust / plain {np.max(errs[:, 1] / errs[:, 0]):.3f}")
    assert len(errs) == rr.N_SCENARIOS and np.all(errs[:, 1] < 0.5 * errs[:, 0])


# ----------------------------------------------------------------------------- zero padding, same image, skipped laws
def test_zero_padded_pairs_have_weight_zero():
    eng, params = ENGINES.fetch(14, 130)
    rng = np.random.default_rng(77)
    sc = rr.planted_scenario(rng, 24, 0.125, params, K=ls.intrinsics(rng, params), holes=True)
    n_live = 10
    s_star, s_, ref = rr.oracle_law(sc, params, n_live=n_live, rows=24)
    s_min = ls.s_min(params, sc["img"], sc["K"])
    rob = rr.robust_velocity(ref["L"], ref["e"], params.lambda_, 4, s_min, n_live=n_live)
    v, st, det = _run(eng, sc, 4, num_pairs=24, ids=sc["ids"][:n_live])
    assert int(det["info"][0, 3]) == n_live and int(det["info"][0, 1]) == 24
    _check_robust(det, 0, v, st, ref, rob, s_star, s_, 24, 4, "ldlt", "padded")
    assert not det["weights"][0, n_live:].any()
    live = rr.robust_velocity(ref["L"][:2 * n_live], ref["e"][:2 * n_live], params.lambda_, 4, s_min)
    assert rr.rel_l2(v, live["v_c"]) <= VC_BAR                       # the law of the live pairs alone


def test_same_image_and_skipped_laws():
    g, k = 14, 24
    t = g * g
    eng, params = ENGINES.fetch(g, 130)
    rng = np.random.default_rng(78)
    nn1, nn2, sim1, mutual = ls.tables(rng, t, t // 3)
    depth, K = ls.depth(rng), params.intrinsics()
    eng.set_option("robust_law", 4)
    order = rng.permutation(t).astype(np.int32)
    v, st = eng.servo_from_nn(nn1, nn2, np.ones(t, np.float32), depth, K, mode=_lib.SELECT_ORDER, selection=order, num_pairs=k)
    det = eng.last_details(1)
    assert int(st) == _lib.STATUS_OK and int(det["info"][0, 2]) == 1 and np.all(v.cpu().numpy() == 0)
    assert int(det["info"][0, 6]) == 4 and int(det["info"][0, 7]) == 0 and np.all(det["weights"][0, :k] == 1.0)
    few = rng.choice(mutual, size=3, replace=False).astype(np.int32)
    results = {}
    for n_iter in (0, 4):
        eng.set_option("robust_law", n_iter)
        v, st = eng.servo_from_nn(nn1, nn2, sim1, depth, K, mode=_lib.SELECT_EXPLICIT, selection=[few], num_pairs=k)
        det = eng.last_details(1)
        assert int(st) == _lib.STATUS_TOO_FEW and np.all(v.cpu().numpy() == 0) and int(det["info"][0, 6]) == 0
        assert not det["weights"][0].any()
        results[("few", n_iter)] = (v.cpu().numpy(), det["info"][0, :6].copy())
        v, st = eng.servo_from_nn(nn1, nn2, sim1, None, K, mode=_lib.SELECT_EXPLICIT, selection=[mutual[:k].astype(np.int32)],
                                  num_pairs=k)
        det = eng.last_details(1)
        assert int(st) == _lib.STATUS_NO_DEPTH and np.all(v.cpu().numpy() == 0) and int(det["info"][0, 6]) == 0
        results[("nodepth", n_iter)] = (v.cpu().numpy(), det["info"][0, :6].copy())
    for what in ("few", "nodepth"):
        assert np.array_equal(results[(what, 0)][0], results[(what, 4)][0]) and np.array_equal(results[(what, 0)][1], results[(what, 4)][1])


# ----------------------------------------------------------------------------- DENSE
def test_dense_selection_at_1024_tokens():
    """Every mutual token (a few hundred) enters the law: L, the weights and the Jacobi copy in the global workspace, the
    residuals and the median over a few hundred values."""
    g = 32
    t = g * g
    eng, params = ENGINES.fetch(g, t)
    rng = np.random.default_rng(4242)
    nn1, nn2, sim1, mutual = ls.tables(rng, t, 300)
    depth, K = ls.depth(rng), ls.intrinsics(rng, params)
    eng.set_option("robust_law", 4)
    v, st = eng.servo_from_nn(nn1, nn2, sim1, depth, K, mode=_lib.SELECT_DENSE, num_pairs=24)
    det = eng.last_details(1)
    rows = int(det["info"][0, 3])
    ids = det["selected"][0, :rows]
    assert rows == len(mutual) > 128 and ids.tolist() == mutual.tolist()
    s_star, s_, ref = ls.oracle(g, 16 * g, params, nn1, ids, rows, depth, K)
    rob = rr.robust_velocity(ref["L"], ref["e"], params.lambda_, 4, ls.s_min(params, 16 * g, K))
    _check_robust(det, 0, v.cpu().numpy(), st, ref, rob, s_star, s_, rows, 4, "ldlt", ("dense", rows))


# ----------------------------------------------------------------------------- off means off
def test_off_means_off():
    img = 224
    params = config.ServoParams(dino_input_size=img)
    eng = Engine(ls.tiny_cfg(img), params, precision="fp32", max_pairs=1, max_rows=48)      # the option never set
    rng = np.random.default_rng(5)
    sc = rr.planted_scenario(rng, 24, 0.125, params, holes=True)
    runs = []
    for n_iter in (None, 4, 0):
        if n_iter is not None:
            eng.set_option("robust_law", n_iter)
        v, st = eng.servo_from_nn(sc["nn_1"], sc["nn_2"], sc["sim_1"], sc["depth"], sc["K"], mode=_lib.SELECT_EXPLICIT,
                                  selection=[sc["ids"]], num_pairs=24)
        runs.append((v.cpu().numpy(), int(st), eng.last_details(1)))
    (v0, st0, d0), (v4, st4, d4), (v2, st2, d2) = runs
    assert st0 == st2 == _lib.STATUS_OK and np.array_equal(v0, v2) and np.array_equal(d0["info"], d2["info"])
    assert np.array_equal(d0["L"], d2["L"]) and np.array_equal(d0["L"], d4["L"])          # L and e stay the unweighted ones
    assert not np.array_equal(v0, v4) and int(d4["info"][0, 6]) == 4 and int(d0["info"][0, 6]) == 0 and int(d0["info"][0, 7]) == 0
    for d in (d0, d2):
        assert np.all(d["weights"][0, :24] == 1.0) and not d["weights"][0, 24:].any()
    _, _, ref = rr.oracle_law(sc, params)
    assert rr.rel_l2(v0, ref["v_c"]) <= VC_BAR
    for bad in (17, -1):
        with pytest.raises(VitvsError, match=r"\(-5\)"):
            eng.set_option("robust_law", bad)
    eng.close()


# ----------------------------------------------------------------------------- every entry point (ViT-S/16)
def test_every_entry_point_evaluates_the_robust_law():
    cfg = config.baseline_config("vits16_224")
    params = config.ServoParams(dino_input_size=cfg.img_size, use_feature_binning=False, robust_iterations=4)
    eng = Engine(cfg, params, precision="fp32", max_pairs=1).load_state_dict(weights.synthetic_state_dict(cfg, 0))
    des, cur = synth.frame_pair(cfg.img_size, 20250705)
    depth, K = synth.depth_pattern(), params.intrinsics()
    k = params.num_pairs
    eng.compute_velocity(cur, des, depth, K, mode=_lib.SELECT_ORDER, selection=np.arange(cfg.tokens, dtype=np.int32))
    tabs = eng.last_details(1)
    mutual = np.nonzero(tabs["nn_2"][0][tabs["nn_1"][0]] == np.arange(cfg.tokens))[0]
    ids = mutual[:: max(1, len(mutual) // k)][:k].astype(np.int32)
    v_dev, st_dev = eng.compute_velocity(cur, des, depth, K, mode=_lib.SELECT_EXPLICIT, selection=[ids])
    det = eng.last_details(1)
    v_dev = v_dev.cpu().numpy()[0]
    assert int(st_dev[0]) == _lib.STATUS_OK and int(det["info"][0, 6]) == 4
    rob = rr.robust_velocity(det["L"][0, :6, :2 * k].T, det["L"][0, 6, :2 * k], params.lambda_, 4, ls.s_min(params, cfg.img_size, K))
    assert rob["margin"] >= MARGIN
    assert rr.rel_l2(v_dev, rob["v_c"]) <= VC_BAR and np.max(np.abs(det["weights"][0, :k] - rob["w"])) <= W_BAR
    v_host, st_host = eng.compute_velocity_host(cur, des, depth, K, mode=_lib.SELECT_EXPLICIT, selection=[ids])
    assert int(st_host[0]) == _lib.STATUS_OK and np.array_equal(v_host[0], v_dev)
    assert np.array_equal(eng.last_weights(1), det["weights"]) and int(eng.last_features(1)["info"][0, 6]) == 4
    eng.compute_velocity_host(cur, des, depth, K, mode=_lib.SELECT_ORDER, selection=np.arange(cfg.tokens, dtype=np.int32))
    v_re, st_re = eng.reselect_host(_lib.SELECT_EXPLICIT, [ids])
    assert int(st_re[0]) == _lib.STATUS_OK and np.array_equal(v_re[0], v_dev)
    # graph replay: a change of the option drops the captured update
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
    v_g4 = replayed()
    assert np.array_equal(replayed(), v_g4) and np.array_equal(v_g4, v_dev)
    eng.set_option("robust_law", 0)
    v_g0 = replayed()
    plain = -params.lambda_ * np.linalg.pinv(det["L"][0, :6, :2 * k].T) @ det["L"][0, 6, :2 * k]
    assert not np.array_equal(v_g0, v_g4) and rr.rel_l2(v_g0, plain) <= VC_BAR and np.all(eng.last_weights(1)[0, :k] == 1.0)
    eng.set_option("robust_law", 4)
    assert np.array_equal(replayed(), v_g4)
    eng.close()
