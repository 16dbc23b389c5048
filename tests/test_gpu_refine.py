"""Sub-patch refinement of matches (option ``subpatch``) on the GPU against its fp64 numpy statement
(tests/refine_ref.py).

  * ``vitvs_refine_dev`` (the arithmetic alone: one wave per token, refine.h) on smooth and random descriptors at T = 196, 484,
    1369 and Dp = 384, 768, 1024, 9 x 384.  Bar on an offset: 4 x the error of an fp32 numpy evaluation of the same formula
    against fp64 on the same inputs (measured per case on the reference alone, tests/test_refine_host.py: 7e-7 .. 2.6e-6 on the
    smooth cases, 4e-7 .. 1.2e-6 on the random ones; the device measured 1.1e-7 .. 4.6e-7); parabolas whose fp64 |den| is below
    1e-4 (none in these cases; at most 5 % allowed) are held to |error| <= 1/2 only.
  * the law on a GIVEN offset table (``vitvs_servo_from_nn_ex_dev``) against ``oracle.servo_ref.velocity`` on the refined integer
    pixels: pixel features and Z exact, L / e within 1e-13, v_c within 1e-9 relative L2 (the project's bars for the law).
  * end to end: the offsets of ``vitvs_last_offsets`` against the reference on the device's own descriptors and tables, to the
    bar of the first item; s_uv, Z and v_c against the oracle's law on the pixels those offsets give.
  * off means off, identical frames, graph replay.
Helpers follow tests/test_gpu_robust_law.py."""
import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib, config, synth, weights
from vitvs_amd.engine import Engine, VitvsError
import refine_ref as rf
import robust_ref as rr
import law_support as ls
from law_support import TinyEngines, close_engines  # noqa: F401

pytestmark = pytest.mark.gpu

ENGINES = TinyEngines()           # this module's tiny handles: close_engines closes them at its teardown

LDLT = -1
VC_BAR, L_BAR, W_BAR = 1e-9, 1e-13, 1e-9
BAR_FACTOR = 4.0


# ----------------------------------------------------------------------------- the seam: vitvs_refine_dev
@pytest.mark.parametrize("kind", ["smooth", "random"])
@pytest.mark.parametrize("Dp", rf.SEAM_WIDTHS)
@pytest.mark.parametrize("T", rf.SEAM_TOKENS)
def test_refine_dev_equals_the_reference(T, Dp, kind):
    # the handle's descriptor workspace holds 2 * max_pairs * T_handle * 128 floats: 28 pairs of 1369 tokens take 2 x 1369 x 3456
    eng, _ = ENGINES.fetch(37, 48, max_pairs=28)
    g = int(round(np.sqrt(T)))
    d1, d2 = rf.descriptor_case(T, Dp, kind)
    S = rf.cosine_similarity(d1, d2)
    nn1 = S.argmax(1)
    ref, den = rf.offsets_from_similarity(S, nn1, g, with_den=True)
    e32, _, share = rf.offset_errors(rf.offsets(d1, d2, nn1, g, dtype=np.float32), ref, den)
    assert share <= rf.SMALL_DEN_SHARE
    off = eng.refine(torch.from_numpy(d1), torch.from_numpy(d2), nn1).cpu().numpy()
    big, small, _ = rf.offset_errors(off, ref, den)
    print(f"refine_dev {kind} T={T} Dp={Dp}: device against fp64 {big:.2e} (fp32 numpy {e32:.2e}, bar {BAR_FACTOR * e32:.2e}); "
          f"|den| < 1e-4: share {share:.4f}, error {small:.2e}")
    assert np.all(np.isfinite(off)) and np.all(np.abs(off) <= 0.5)
    r, c = np.divmod(nn1, g)
    assert not off[(r == 0) | (r == g - 1), 0].any() and not off[(c == 0) | (c == g - 1), 1].any()     # borders
    assert small <= 0.5
    assert big <= BAR_FACTOR * e32, (kind, T, Dp, big, e32)
    again = eng.refine(torch.from_numpy(d1), torch.from_numpy(d2), nn1).cpu().numpy()
    assert np.array_equal(off, again)                                                                  # deterministic


def test_refine_dev_matches_outside_the_grid_and_bad_arguments():
    eng, _ = ENGINES.fetch(37, 48, max_pairs=28)
    d1, d2 = rf.descriptor_case(196, 384, "smooth")
    nn1 = rf.cosine_similarity(d1, d2).argmax(1)
    nn1[:3] = (-1, 196, 10 ** 6)
    off = eng.refine(torch.from_numpy(d1), torch.from_numpy(d2), nn1).cpu().numpy()
    assert not off[:3].any() and off[3:].any()
    with pytest.raises(VitvsError, match=r"\(-5\)"):                                                   # not a square grid
        eng.refine(torch.from_numpy(d1[:195]), torch.from_numpy(d2[:195]), nn1[:195])


# ----------------------------------------------------------------------------- the law on a given offset table
def _check_law(det, v, st, ref, s_star, s_, rows, what, off_rows=None):
    assert int(st) == _lib.STATUS_OK, (what, int(st))
    suv = det["s_uv"][0, :rows]
    assert np.array_equal(suv[:, 0:2], s_star) and np.array_equal(suv[:, 2:4], s_), what
    assert np.array_equal(det["feat"][0, :rows, 0:1], ref["Z"]), what
    assert np.array_equal(det["feat"][0, :rows, 1:3], ref["s_xy"]), what
    np.testing.assert_allclose(det["L"][0, :6, :2 * rows].T, ref["L"], rtol=0, atol=L_BAR, err_msg=str(what))
    np.testing.assert_allclose(det["L"][0, 6, :2 * rows], ref["e"][:, 0], rtol=0, atol=L_BAR, err_msg=str(what))
    if off_rows is not None:
        assert np.array_equal(det["offsets"][0, :rows], off_rows), what
    assert not det["offsets"][0, rows:].any(), what


def _scenario(seed, num_pairs, g=14, share=0.0):
    eng, params = ENGINES.fetch(g, max(130, g * g))
    rng = np.random.default_rng(seed)
    sc = rr.planted_scenario(rng, num_pairs, share, params, K=ls.intrinsics(rng, params), g=g, holes=True)
    table = rng.uniform(-0.5, 0.5, size=(g * g, 2)).astype(np.float32)
    table[rng.integers(0, g * g, size=g * g // 8)] = 0.0
    return eng, params, sc, table


def _refined_oracle(sc, params, table, ids, rows):
    s_star, s_ = rf.refined_features(ids, sc["nn_1"], table, sc["img"], sc["g"], params.u_max, params.v_max, rows=rows)
    return s_star, s_, rf.velocity(s_star, s_, sc["depth"], sc["K"], params.lambda_)


@pytest.mark.parametrize("num_pairs", [8, 24, 64, 65, 130])
def test_law_on_a_given_table_explicit(num_pairs):
    """8 .. 64 pairs: L in LDS; 65 and 130: in the global workspace.  Depth holes, random intrinsics; the refined pixels move
    by up to half a patch pitch (23 / 17 camera pixels), so nearly every feature and most depths differ from the plain law's."""
    eng, params, sc, table = _scenario(31000 + num_pairs, num_pairs)
    eng.set_option("robust_law", 0)
    v, st = eng.servo_from_nn(sc["nn_1"], sc["nn_2"], sc["sim_1"], sc["depth"], sc["K"], mode=_lib.SELECT_EXPLICIT,
                              selection=[sc["ids"]], num_pairs=num_pairs, offsets=table)
    det = eng.last_details(1)
    s_star, s_, ref = _refined_oracle(sc, params, table, sc["ids"], num_pairs)
    _, s_plain, _ = rr.oracle_law(sc, params)
    assert np.count_nonzero(np.any(s_ != s_plain, axis=1)) >= num_pairs // 2           # the case does move the features
    _check_law(det, v.cpu().numpy(), st, ref, s_star, s_, num_pairs, ("explicit", num_pairs), table[sc["ids"]])
    err = rr.rel_l2(v.cpu().numpy(), ref["v_c"])
    print(f"law on a table, EXPLICIT {num_pairs} pairs: v_c rel L2 {err:.2e}, solver {int(det['info'][0, 4])}")
    assert err <= VC_BAR and int(det["info"][0, 4]) == LDLT
    # NULL table = the plain entry point
    v0, st0 = eng.servo_from_nn(sc["nn_1"], sc["nn_2"], sc["sim_1"], sc["depth"], sc["K"], mode=_lib.SELECT_EXPLICIT,
                                selection=[sc["ids"]], num_pairs=num_pairs)
    d0 = eng.last_details(1)
    _, _, plain = rr.oracle_law(sc, params)
    assert np.array_equal(d0["s_uv"][0, :num_pairs, 2:4], s_plain) and rr.rel_l2(v0.cpu().numpy(), plain["v_c"]) <= VC_BAR
    assert not d0["offsets"].any()


def test_law_on_a_given_table_order_dense_and_padding():
    eng, params, sc, table = _scenario(32001, 24)
    eng.set_option("robust_law", 0)
    t, g = sc["g"] ** 2, sc["g"]
    nn1, nn2 = np.asarray(sc["nn_1"]), np.asarray(sc["nn_2"])
    mutual = nn2[nn1] == np.arange(t)
    rng = np.random.default_rng(5)
    # ORDER: the first 24 mutual tokens of a visiting order
    order = rng.permutation(t).astype(np.int32)
    ids = np.array([i for i in order if mutual[i]][:24])
    v, st = eng.servo_from_nn(nn1, nn2, sc["sim_1"], sc["depth"], sc["K"], mode=_lib.SELECT_ORDER, selection=order, num_pairs=24,
                              offsets=table)
    det = eng.last_details(1)
    assert det["selected"][0, :24].tolist() == ids.tolist()
    s_star, s_, ref = _refined_oracle(sc, params, table, ids, 24)
    _check_law(det, v.cpu().numpy(), st, ref, s_star, s_, 24, "order", table[ids])
    assert rr.rel_l2(v.cpu().numpy(), ref["v_c"]) <= VC_BAR
    # DENSE: every mutual token (L in the global workspace)
    ids = np.nonzero(mutual)[0]
    v, st = eng.servo_from_nn(nn1, nn2, sc["sim_1"], sc["depth"], sc["K"], mode=_lib.SELECT_DENSE, num_pairs=24, offsets=table)
    det = eng.last_details(1)
    rows = int(det["info"][0, 3])
    assert rows == len(ids) > 64 and det["selected"][0, :rows].tolist() == ids.tolist()
    s_star, s_, ref = _refined_oracle(sc, params, table, ids, rows)
    _check_law(det, v.cpu().numpy(), st, ref, s_star, s_, rows, "dense", table[ids])
    err = rr.rel_l2(v.cpu().numpy(), ref["v_c"])
    print(f"law on a table, DENSE {rows} pairs: v_c rel L2 {err:.2e}")
    assert err <= VC_BAR
    # a short selection: 10 live pairs of 24, zero padding behind them (padded rows: offset 0, pixel 0)
    live = sc["ids"][:10]
    v, st = eng.servo_from_nn(nn1, nn2, sc["sim_1"], sc["depth"], sc["K"], mode=_lib.SELECT_EXPLICIT, selection=[live], num_pairs=24,
                              offsets=table)
    det = eng.last_details(1)
    s_star, s_, ref = _refined_oracle(sc, params, table, live, 24)
    assert int(det["info"][0, 3]) == 10 and not s_[10:].any()
    _check_law(det, v.cpu().numpy(), st, ref, s_star, s_, 24, "padded", np.concatenate([table[live], np.zeros((14, 2), np.float32)]))
    assert rr.rel_l2(v.cpu().numpy(), ref["v_c"]) <= VC_BAR
    # fewer than 4 matches, no depth, same image: the statuses and shortcuts decided before the law are unchanged
    v, st = eng.servo_from_nn(nn1, nn2, sc["sim_1"], sc["depth"], sc["K"], mode=_lib.SELECT_EXPLICIT, selection=[live[:3]], num_pairs=24,
                              offsets=table)
    assert int(st) == _lib.STATUS_TOO_FEW and not v.cpu().numpy().any() and not eng.last_offsets(1).any()
    v, st = eng.servo_from_nn(nn1, nn2, sc["sim_1"], None, sc["K"], mode=_lib.SELECT_EXPLICIT, selection=[sc["ids"]], num_pairs=24,
                              offsets=table)
    assert int(st) == _lib.STATUS_NO_DEPTH and not v.cpu().numpy().any()
    v, st = eng.servo_from_nn(nn1, nn2, np.ones(t, np.float32), sc["depth"], sc["K"], mode=_lib.SELECT_ORDER, selection=order,
                              num_pairs=24, offsets=table)
    det = eng.last_details(1)
    assert int(st) == _lib.STATUS_OK and int(det["info"][0, 2]) == 1 and np.all(v.cpu().numpy() == 0) and not det["offsets"].any()
    assert np.array_equal(det["s_uv"][0, :24, 0:2], det["s_uv"][0, :24, 2:4])


@pytest.mark.parametrize("num_pairs", [24, 65])
def test_law_on_a_given_table_jacobi(num_pairs):
    """Every selected goal token has the same match AND the same offset: identical rows of L (rank 2), the pivot test fails and
    the Jacobi SVD solves, on L in LDS (24 pairs) and in the global workspace (65)."""
    eng, params, sc, table = _scenario(33000 + num_pairs, num_pairs)
    eng.set_option("robust_law", 0)
    t = sc["g"] ** 2
    nn1 = np.asarray(sc["nn_1"]).copy()
    nn1[sc["ids"]] = 5 * sc["g"] + 6
    table[sc["ids"]] = (0.31, -0.27)
    assert 0 < np.count_nonzero(np.asarray(sc["nn_2"])[nn1] == np.arange(t)) < t
    sc = dict(sc, nn_1=nn1)
    v, st = eng.servo_from_nn(nn1, sc["nn_2"], sc["sim_1"], sc["depth"], sc["K"], mode=_lib.SELECT_EXPLICIT, selection=[sc["ids"]],
                              num_pairs=num_pairs, offsets=table)
    det = eng.last_details(1)
    s_star, s_, ref = _refined_oracle(sc, params, table, sc["ids"], num_pairs)
    _check_law(det, v.cpu().numpy(), st, ref, s_star, s_, num_pairs, ("jacobi", num_pairs), table[sc["ids"]])
    err = rr.rel_l2(v.cpu().numpy(), ref["v_c"])
    print(f"law on a table, Jacobi {num_pairs} pairs: v_c rel L2 {err:.2e}, sweeps {int(det['info'][0, 4])}")
    assert err <= VC_BAR and 0 <= int(det["info"][0, 4]) <= 40


@pytest.mark.parametrize("num_pairs", [24, 48, 130])
def test_law_on_a_given_table_with_the_robust_law(num_pairs):
    """servo_kernel<true, true>: Tukey IRLS (N = 4) on the refined system against tests/robust_ref.py."""
    eng, params, sc, table = _scenario(34000 + num_pairs, num_pairs, share=0.25 if num_pairs >= 48 else 0.125)
    eng.set_option("robust_law", 4)
    v, st = eng.servo_from_nn(sc["nn_1"], sc["nn_2"], sc["sim_1"], sc["depth"], sc["K"], mode=_lib.SELECT_EXPLICIT,
                              selection=[sc["ids"]], num_pairs=num_pairs, offsets=table)
    det = eng.last_details(1)
    eng.set_option("robust_law", 0)
    s_star, s_, ref = _refined_oracle(sc, params, table, sc["ids"], num_pairs)
    rob = rr.robust_velocity(ref["L"], ref["e"], params.lambda_, 4, rr.sigma_min(16, params.u_max, params.v_max, sc["img"], sc["K"][0], sc["K"][1]))
    assert rob["margin"] >= 1e-6, "the case sits on the rejection point: choose other inputs"
    _check_law(det, v.cpu().numpy(), st, ref, s_star, s_, num_pairs, ("robust", num_pairs), table[sc["ids"]])
    werr = float(np.max(np.abs(det["weights"][0, :num_pairs] - rob["w"])))
    err = rr.rel_l2(v.cpu().numpy(), rob["v_c"])
    print(f"law on a table, robust_law 4, {num_pairs} pairs: weights {werr:.2e}, v_c rel L2 {err:.2e}, zero weights {rob['n_zero']}")
    assert werr <= W_BAR and err <= VC_BAR and int(det["info"][0, 6]) == 4 and int(det["info"][0, 7]) == rob["n_zero"]


# ----------------------------------------------------------------------------- end to end (ViT-S/16 224)
_SD = {}


def _vits16(precision, binned, **kw):
    cfg = config.baseline_config("vits16_224")
    if "sd" not in _SD:
        _SD["sd"] = weights.synthetic_state_dict(cfg, 0)
    params = config.ServoParams(dino_input_size=cfg.img_size, use_feature_binning=binned, **kw)
    eng = Engine(cfg, params, precision=precision, max_pairs=1, max_rows=cfg.tokens).load_state_dict(_SD["sd"])
    return cfg, params, eng


def _reference_offsets(eng, cfg, des, cur, nn1):
    """fp64 offsets, their denominators and the fp32-numpy error of the formula on the DEVICE's own descriptors of the two frames."""
    desc = eng.extract_descriptors(np.stack([des, cur]))[:, 0].cpu().numpy()
    S = rf.cosine_similarity(desc[0], desc[1])
    ref, den = rf.offsets_from_similarity(S, nn1, cfg.grid, with_den=True)
    e32, _, share = rf.offset_errors(rf.offsets(desc[0], desc[1], nn1, cfg.grid, dtype=np.float32), ref, den)
    return ref, den, e32, share


def _check_end_to_end(eng, cfg, params, det, v, st, depth, K, ref, den, e32, what):
    assert int(st) == _lib.STATUS_OK and int(det["info"][0, 2]) == 0, what
    rows = int(det["info"][0, 1])
    live = int(det["info"][0, 3])
    ids = det["selected"][0, :live].astype(np.int64)
    nn1 = det["nn_1"][0].astype(np.int64)
    off = det["offsets"][0]
    big, small, share = rf.offset_errors(off[:live], ref[ids], den[ids])
    print(f"{what}: {live} rows, offsets against fp64 {big:.2e} (fp32 numpy {e32:.2e}, bar {BAR_FACTOR * e32:.2e}), "
          f"|den| < 1e-4 share {share:.3f}, largest |offset| {np.abs(off).max():.3f}")
    assert np.abs(off[:live]).max() > 0.05 and np.all(np.abs(off) <= 0.5) and not off[live:].any(), what
    assert small <= 0.5 and big <= BAR_FACTOR * e32, (what, big, e32)
    # the law on the pixels the device's own offsets give
    table = np.zeros((cfg.tokens, 2), np.float32)
    table[ids] = off[:live]
    s_star, s_ = rf.refined_features(ids, nn1, table, cfg.img_size, cfg.grid, params.u_max, params.v_max, rows=rows)
    oracle = rf.velocity(s_star, s_, depth, K, params.lambda_)
    assert np.array_equal(det["s_uv"][0, :rows, 0:2], s_star) and np.array_equal(det["s_uv"][0, :rows, 2:4], s_), what
    assert np.array_equal(det["feat"][0, :rows, 0:1], oracle["Z"]) and np.array_equal(det["feat"][0, :rows, 1:3], oracle["s_xy"]), what
    err = rr.rel_l2(v, oracle["v_c"])
    print(f"{what}: v_c rel L2 against the oracle on the refined pixels {err:.2e}")
    assert err <= VC_BAR, (what, err)


@pytest.mark.parametrize("binned", [False, True])
@pytest.mark.parametrize("precision", ["fp32", "f16x2", "bf16"])
def test_end_to_end(precision, binned):
    """compute_velocity, compute_velocity_host and reselect with the option on: plain descriptors (the fused Gram: offsets from
    the fp32 normalised descriptors) and binned ones (the stencil form: offsets from the raw Gram)."""
    cfg, params, eng = _vits16(precision, binned, subpatch=True)
    des, cur = synth.frame_pair(cfg.img_size, 20250705)
    depth, K = synth.depth_pattern(), params.intrinsics()
    k = params.num_pairs
    order = np.random.default_rng(3).permutation(cfg.tokens).astype(np.int32)
    what = f"end to end {precision} {'binned' if binned else 'plain'}"
    # ORDER, 24 pairs
    v, st = eng.compute_velocity(cur, des, depth, K, mode=_lib.SELECT_ORDER, selection=order)
    det = eng.last_details(1)
    v = v.cpu().numpy()[0]
    ref, den, e32, share = _reference_offsets(eng, cfg, des, cur, det["nn_1"][0].astype(np.int64))
    assert share <= rf.SMALL_DEN_SHARE
    _check_end_to_end(eng, cfg, params, det, v, st[0], depth, K, ref, den, e32, what + " ORDER")
    # DENSE: every mutual token
    vd, std = eng.compute_velocity(cur, des, depth, K, mode=_lib.SELECT_DENSE)
    detd = eng.last_details(1)
    assert np.array_equal(detd["nn_1"], det["nn_1"]) and int(detd["info"][0, 3]) > k
    _check_end_to_end(eng, cfg, params, detd, vd.cpu().numpy()[0], std[0], depth, K, ref, den, e32, what + " DENSE")
    # the host-pointer entry point and the law again on its tables
    ids = det["selected"][0, :k].astype(np.int32)
    vh, sth = eng.compute_velocity_host(cur, des, depth, K, mode=_lib.SELECT_ORDER, selection=order)
    assert int(sth[0]) == _lib.STATUS_OK and np.array_equal(vh[0], v)
    assert np.array_equal(eng.last_offsets(1), det["offsets"]) and np.array_equal(eng.last_features(1)["s_uv"], det["s_uv"])
    vr, str_ = eng.reselect_host(_lib.SELECT_EXPLICIT, [ids])
    assert int(str_[0]) == _lib.STATUS_OK and np.array_equal(vr[0], v) and np.array_equal(eng.last_offsets(1), det["offsets"])
    # with robust_law on top: the robust reference on the device's own (refined) L and e
    eng.set_option("robust_law", 4)
    v4, st4 = eng.compute_velocity(cur, des, depth, K, mode=_lib.SELECT_ORDER, selection=order)
    det4 = eng.last_details(1)
    assert int(st4[0]) == _lib.STATUS_OK and np.array_equal(det4["s_uv"], det["s_uv"]) and np.array_equal(det4["offsets"], det["offsets"])
    rob = rr.robust_velocity(det4["L"][0, :6, :2 * k].T, det4["L"][0, 6, :2 * k], params.lambda_, 4,
                             rr.sigma_min(cfg.stride, params.u_max, params.v_max, cfg.img_size, K[0], K[1]))
    if rob["margin"] >= 1e-6:
        assert rr.rel_l2(v4.cpu().numpy()[0], rob["v_c"]) <= VC_BAR
    eng.close()


def test_end_to_end_split_gram_form():
    """ViT-B/8 448² in bf16: 3136 tokens, so the Gram runs on the f16 matrix cores from the hi / lo split of the descriptors
    (GRAM_SPLIT); the refinement still reads the fp32 rows."""
    cfg = config.baseline_config("vitb8_448")
    params = config.ServoParams(dino_input_size=cfg.img_size, use_feature_binning=False, subpatch=True)
    eng = Engine(cfg, params, precision="bf16", max_pairs=1, max_rows=48).load_state_dict(weights.synthetic_state_dict(cfg, 0))
    des, cur = synth.frame_pair(cfg.img_size, 20250705)
    depth, K = synth.depth_pattern(), params.intrinsics()
    order = np.random.default_rng(3).permutation(cfg.tokens).astype(np.int32)
    v, st = eng.compute_velocity(cur, des, depth, K, mode=_lib.SELECT_ORDER, selection=order)
    det = eng.last_details(1)
    ref, den, e32, share = _reference_offsets(eng, cfg, des, cur, det["nn_1"][0].astype(np.int64))
    assert share <= rf.SMALL_DEN_SHARE
    _check_end_to_end(eng, cfg, params, det, v.cpu().numpy()[0], st[0], depth, K, ref, den, e32, "end to end bf16 ViT-B/8 448 ORDER")
    eng.close()


# ----------------------------------------------------------------------------- off means off
@pytest.mark.parametrize("binned", [False, True])
def test_off_means_off(binned):
    cfg, params, eng0 = _vits16("fp32", binned)                 # never sees the option
    _, _, eng = _vits16("fp32", binned)
    des, cur = synth.frame_pair(cfg.img_size, 20250705)
    depth, K = synth.depth_pattern(), params.intrinsics()
    order = np.random.default_rng(3).permutation(cfg.tokens).astype(np.int32)

    def update(e, host=False):
        if host:
            v, st = e.compute_velocity_host(cur, des, depth, K, mode=_lib.SELECT_ORDER, selection=order)
            return v[0], int(st[0]), e.last_details(1)
        v, st = e.compute_velocity(cur, des, depth, K, mode=_lib.SELECT_ORDER, selection=order)
        return v.cpu().numpy()[0], int(st[0]), e.last_details(1)
    v0, st0, d0 = update(eng0)
    eng.set_option("subpatch", 0)
    v1, st1, d1 = update(eng)
    eng.set_option("subpatch", 1)
    v2, st2, d2 = update(eng)
    v2h, _, d2h = update(eng, host=True)
    eng.set_option("subpatch", 0)
    v3, st3, d3 = update(eng)
    v3h, _, d3h = update(eng, host=True)
    for v, st, d in ((v1, st1, d1), (v3, st3, d3), (v3h, st3, d3h)):
        assert st == st0 == _lib.STATUS_OK and np.array_equal(v, v0)
        assert np.array_equal(d["s_uv"], d0["s_uv"]) and np.array_equal(d["L"], d0["L"]) and np.array_equal(d["feat"], d0["feat"])
        assert not d["offsets"].any()
    assert st2 == _lib.STATUS_OK and not np.array_equal(v2, v0) and d2["offsets"].any() and np.array_equal(v2h, v2)
    assert np.array_equal(d2["s_uv"][..., 0:2], d0["s_uv"][..., 0:2]) and not np.array_equal(d2["s_uv"], d0["s_uv"])   # the goal side stays
    # identical frames: the same-image shortcut, offsets 0 and v_c = 0 exactly with the option on
    eng.set_option("subpatch", 1)
    v, st = eng.compute_velocity(des, des, depth, K, mode=_lib.SELECT_ORDER, selection=order)
    det = eng.last_details(1)
    assert int(st[0]) == _lib.STATUS_OK and int(det["info"][0, 2]) == 1 and np.all(v.cpu().numpy() == 0) and not det["offsets"].any()
    for bad in (2, -1):
        with pytest.raises(VitvsError, match=r"\(-5\)"):
            eng.set_option("subpatch", bad)
    eng.close()
    eng0.close()


# ----------------------------------------------------------------------------- graph replay
@pytest.mark.parametrize("binned", [False, True])
def test_graph_replay_equals_eager_and_the_option_recaptures(binned):
    cfg, params, eng = _vits16("fp32", binned, subpatch=True)
    des, cur = synth.frame_pair(cfg.img_size, 20250705)
    depth, K = synth.depth_pattern(), params.intrinsics()
    k = params.num_pairs
    order = np.random.default_rng(3).permutation(cfg.tokens).astype(np.int32)
    v_on, _ = eng.compute_velocity(cur, des, depth, K, mode=_lib.SELECT_ORDER, selection=order)
    v_on = v_on.cpu().numpy()[0]
    off_on = eng.last_offsets(1)
    eng.set_option("subpatch", 0)
    v_off, _ = eng.compute_velocity(cur, des, depth, K, mode=_lib.SELECT_ORDER, selection=order)
    v_off = v_off.cpu().numpy()[0]
    eng.set_option("subpatch", 1)
    eng.set_option("graph_replay", 1)
    cur_d, des_d = eng._frames(cur), eng._frames(des)
    z_d = torch.as_tensor(depth).reshape(1, params.v_max, params.u_max).to(eng.device).contiguous()
    k_d = torch.as_tensor(K, dtype=torch.float64).reshape(1, 4).to(eng.device)
    sel_d, cnt_d = eng._selection_args(_lib.SELECT_ORDER, order, 1, cfg.tokens, k)
    out_v = torch.zeros((1, 6), dtype=torch.float64, device=eng.device)
    out_s = torch.zeros(1, dtype=torch.int32, device=eng.device)

    def replayed():
        eng.compute_velocity_dev(cur_d, des_d, z_d, k_d, _lib.SELECT_ORDER, sel_d, cnt_d, out_v=out_v, out_status=out_s, num_pairs=k)
        torch.cuda.synchronize()
        return out_v.cpu().numpy()[0].copy()
    g_on = replayed()
    assert np.array_equal(g_on, v_on) and np.array_equal(replayed(), v_on) and np.array_equal(eng.last_offsets(1), off_on)
    eng.set_option("subpatch", 0)                  # drops the captured update: the replay is the plain law's
    assert np.array_equal(replayed(), v_off) and not eng.last_offsets(1).any() and not np.array_equal(v_off, v_on)
    eng.set_option("subpatch", 1)
    assert np.array_equal(replayed(), v_on) and np.array_equal(eng.last_offsets(1), off_on)
    eng.close()
