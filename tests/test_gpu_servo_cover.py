"""Every code path of the control law (servo.hip) against the oracle's numpy law (GPU).

servo_kernel picks among several paths: the depth prefetch (T <= 256) or direct depth reads; the one-position ballot scan
(T <= 256) or the shuffle scan over ceil(T / 256) positions per thread, with tail threads holding none (T = 289: threads from
145 on); L in LDS (R = 2 * rows <= 128) or in the global workspace with column stride 2 * max_rows; the LDL^T normal equations or,
when a pivot falls below 1e-4 of its diagonal, one-sided Jacobi SVD, whose lanes loop over several rows once R > 64.  Every case
asserts which solver ran through info[4] (-1: LDL^T, otherwise the Jacobi sweeps, <= 40) and R through info[5], and checks the
law against oracle/servo_ref (numpy pinv): s_uv exact, Z exact, L within 1e-13, v_c within 1e-9 (relative L2).  The tables go
in through vitvs_servo_from_nn_dev (tiny handles, T up to 1024) or come from velocity calls of the 2-block tiny model.
Also here: the three law options (robust_law, subpatch, interaction) together through the forward and every entry point, and the
reselect state of the host-pointer entry point, which ends with every call that rewrites the arg-max keys."""
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
VC_BAR, L_BAR = 1e-9, 1e-13


def _check_law(det, b, v, st, ref, s_star, s_, rows, solver, what):
    """One pair's law against the oracle's, and the solver that ran."""
    assert int(st) == _lib.STATUS_OK, (what, int(st))
    info = det["info"][b]
    assert int(info[5]) == 2 * rows, (what, info)
    assert (ls.ldlt_passes(ref["L"]) == (solver == "ldlt")), (what, "the case does not reach the solver it names")
    if solver == "ldlt":
        assert int(info[4]) == LDLT, (what, "expected LDL^T", info)
    else:
        assert 0 <= int(info[4]) <= MAX_SWEEPS, (what, "expected Jacobi", info)
    suv = det["s_uv"][b, :rows]
    assert np.array_equal(suv[:, 0:2], s_star) and np.array_equal(suv[:, 2:4], s_), what
    assert np.array_equal(det["feat"][b, :rows, 0:1], ref["Z"]), what
    np.testing.assert_allclose(det["L"][b, :6, :2 * rows].T, ref["L"], rtol=0, atol=L_BAR, err_msg=what)
    np.testing.assert_allclose(det["L"][b, 6, :2 * rows], ref["e"][:, 0], rtol=0, atol=L_BAR, err_msg=what)
    err = rr.rel_l2(v, ref["v_c"])
    assert err <= VC_BAR, (what, err)
    return int(info[4])


# ----------------------------------------------------------------------------- random tables, every selection mode
@pytest.mark.parametrize("mode", ["order", "explicit", "dense"])
@pytest.mark.parametrize("g", [14, 17, 22, 32])
def test_law_on_random_tables(g, mode):
    """T = 196 (prefetched depth, ballot scan), 289 (direct depth reads, shuffle scan, threads from 145 on without a position),
    484 and 1024 (4 positions per thread).  ORDER and EXPLICIT keep 24 pairs (L in LDS), DENSE all mutual tokens (L global)."""
    t, k = g * g, 24
    rng = np.random.default_rng(7000 + 10 * g + ["order", "explicit", "dense"].index(mode))
    eng, params = ENGINES.fetch(g, t)
    img = 16 * g
    nn1, nn2, sim1, mutual = ls.tables(rng, t, int(rng.integers(t // 4, t // 2)))
    depth, K = ls.depth(rng), ls.intrinsics(rng, params)
    if mode == "order":
        order = rng.permutation(t).astype(np.int32)
        mset = set(mutual.tolist())
        ids, rows = np.array([x for x in order if x in mset][:k]), k
        v, st = eng.servo_from_nn(nn1, nn2, sim1, depth, K, mode=_lib.SELECT_ORDER, selection=order, num_pairs=k)
    elif mode == "explicit":
        ids, rows = rng.choice(t, size=k, replace=False).astype(np.int32), k      # any tokens, mutual or not
        v, st = eng.servo_from_nn(nn1, nn2, sim1, depth, K, mode=_lib.SELECT_EXPLICIT, selection=[ids], num_pairs=k)
    else:
        ids, rows = mutual, len(mutual)
        v, st = eng.servo_from_nn(nn1, nn2, sim1, depth, K, mode=_lib.SELECT_DENSE, num_pairs=k)
    det = eng.last_details(1)
    assert int(det["info"][0, 0]) == len(mutual) and int(det["info"][0, 3]) == rows
    assert det["selected"][0, :rows].tolist() == [int(x) for x in ids]
    s_star, s_, ref = ls.oracle(g, img, params, nn1, ids, rows, depth, K)
    _check_law(det, 0, v.cpu().numpy(), st, ref, s_star, s_, rows, "ldlt", (g, mode))
    if mode == "dense":
        assert 2 * rows > 128                                 # L in the global workspace


# ----------------------------------------------------------------------------- both solvers across the LDS / global edge
@pytest.mark.parametrize("solver", ["ldlt", "jacobi"])
@pytest.mark.parametrize("num_pairs", [4, 24, 40, 64, 65])
def test_both_solvers_across_the_lds_edge(num_pairs, solver):
    """R = 8 .. 130: LDS up to 128 rows, the global workspace beyond with column stride 2 * max_rows = 160 != R.  Well conditioned
    (distinct mutual tokens: LDL^T) and rank-deficient (Jacobi, each lane over several rows from R = 65 on): one token repeated
    below 32 pairs; from 32 pairs on two tokens in two blocks, the second holding the last 4 pairs, so that rows past 64 are not
    a repeat of the first 64."""
    g, max_rows = 17, 80
    t = g * g
    rng = np.random.default_rng(100 * num_pairs + (solver == "jacobi"))
    eng, params = ENGINES.fetch(g, max_rows)
    nn1, nn2, sim1, mutual = ls.tables(rng, t, 200)
    depth, K = ls.depth(rng), ls.intrinsics(rng, params)
    if solver == "ldlt":
        ids = rng.choice(mutual, size=num_pairs, replace=False)
    else:
        moved = np.nonzero(nn1 != np.arange(t))[0]            # displaced matches: e != 0
        if num_pairs < 32:
            ids = np.full(num_pairs, rng.choice(moved))
        else:
            a, b = rng.choice(moved, size=2, replace=False)
            ids = np.where(np.arange(num_pairs) < num_pairs - 4, a, b)
    ids = ids.astype(np.int32)
    v, st = eng.servo_from_nn(nn1, nn2, sim1, depth, K, mode=_lib.SELECT_EXPLICIT, selection=[ids], num_pairs=num_pairs)
    det = eng.last_details(1)
    s_star, s_, ref = ls.oracle(g, 16 * g, params, nn1, ids, num_pairs, depth, K)
    _check_law(det, 0, v.cpu().numpy(), st, ref, s_star, s_, num_pairs, solver, (num_pairs, solver))


@pytest.mark.parametrize("seed", range(6))
def test_rank_four_selections_within_the_sweep_cap(seed):
    """Two distinct tokens (rank 4): the Jacobi sweeps converge slowly and may stop at the cap of 40; v_c still matches."""
    g, k = 14, 24
    t = g * g
    rng = np.random.default_rng(500 + seed)
    eng, params = ENGINES.fetch(g, 48)
    nn1, nn2, sim1, _ = ls.tables(rng, t, 80)
    depth, K = ls.depth(rng), ls.intrinsics(rng, params)
    moved = np.nonzero(nn1 != np.arange(t))[0]
    ids = np.resize(rng.choice(moved, size=2, replace=False), k).astype(np.int32)
    v, st = eng.servo_from_nn(nn1, nn2, sim1, depth, K, mode=_lib.SELECT_EXPLICIT, selection=[ids], num_pairs=k)
    det = eng.last_details(1)
    s_star, s_, ref = ls.oracle(g, 16 * g, params, nn1, ids, k, depth, K)
    assert np.linalg.matrix_rank(ref["L"]) == 4
    sweeps = _check_law(det, 0, v.cpu().numpy(), st, ref, s_star, s_, k, "jacobi", seed)
    print(f"rank-4 selection {seed}: {sweeps} sweeps")


# ----------------------------------------------------------------------------- statuses and the same-image shortcut
@pytest.mark.parametrize("g", [17, 32])
def test_statuses_at_many_tokens(g):
    t, k = g * g, 24
    rng = np.random.default_rng(300 + g)
    eng, params = ENGINES.fetch(g, t)
    nn1, nn2, sim1, mutual = ls.tables(rng, t, t // 3)
    depth, K = ls.depth(rng), params.intrinsics()
    few = rng.choice(mutual, size=3, replace=False).astype(np.int32)
    v, st = eng.servo_from_nn(nn1, nn2, sim1, depth, K, mode=_lib.SELECT_EXPLICIT, selection=[few], num_pairs=k)
    det = eng.last_details(1)
    assert int(st) == _lib.STATUS_TOO_FEW and np.all(v.cpu().numpy() == 0) and not det["s_uv"][0, :k].any()
    v, st = eng.servo_from_nn(nn1, nn2, sim1, None, K, mode=_lib.SELECT_DENSE, num_pairs=k)
    assert int(st) == _lib.STATUS_NO_DEPTH and np.all(v.cpu().numpy() == 0)
    ident = np.arange(t)
    for a, b in ((ident, ident), ((ident + 1) % t, (ident + 2) % t)):      # every token mutual; none
        v, st = eng.servo_from_nn(a, b, np.full(t, 0.5, np.float32), depth, K, mode=_lib.SELECT_ORDER,
                                  selection=rng.permutation(t).astype(np.int32), num_pairs=k)
        det = eng.last_details(1)
        assert int(st) == _lib.STATUS_NO_CORRESPONDENCE and np.all(v.cpu().numpy() == 0), int(st)
        assert int(det["info"][0, 0]) in (0, t)
    # identical frames (mean sim_1 > 0.99): every token is its own match, e = 0, v_c = 0 exactly
    order = rng.permutation(t).astype(np.int32)
    v, st = eng.servo_from_nn(nn1, nn2, np.ones(t, np.float32), depth, K, mode=_lib.SELECT_ORDER, selection=order, num_pairs=k)
    det = eng.last_details(1)
    assert int(det["info"][0, 2]) == 1 and det["selected"][0, :k].tolist() == order[:k].tolist()
    s_star, s_, ref = ls.oracle(g, 16 * g, params, ident, order[:k], k, depth, K)
    assert np.all(v.cpu().numpy() == 0) and np.array_equal(s_star, s_)
    _check_law(det, 0, v.cpu().numpy(), st, ref, s_star, s_, k, "ldlt" if ls.ldlt_passes(ref["L"]) else "jacobi", ("same", g))


# ----------------------------------------------------------------------------- several pairs in one velocity call
def _tiny_model(max_pairs, max_rows):
    cfg = ls.tiny_cfg(224)
    params = config.ServoParams(dino_input_size=224, use_feature_binning=False)
    eng = Engine(cfg, params, precision="fp32", max_pairs=max_pairs, max_rows=max_rows)
    return eng.load_state_dict(weights.synthetic_state_dict(cfg, 3)), cfg, params


def test_three_pairs_each_with_its_own_intrinsics_depth_and_selection():
    """One velocity call, three pairs: each its own frames, K, depth image and EXPLICIT ids; pair 1 rank-deficient (Jacobi)
    beside two LDL^T pairs.  Each pair must be the oracle's law on its own device tables."""
    eng, cfg, params = _tiny_model(3, 196)                   # (max_rows >= T: the DENSE call that draws the tables)
    g, t, k = cfg.grid, cfg.tokens, 24
    rng = np.random.default_rng(33)
    pairs = [synth.frame_pair(cfg.img_size, s) for s in (20250705, 20250715, 20250738)]
    des = np.stack([p[0] for p in pairs])
    cur = np.stack([p[1] for p in pairs])
    depth = np.stack([ls.depth(rng), np.roll(synth.depth_pattern(), 37, axis=1), (synth.depth_pattern() // 2 + 300).astype(np.uint16)])
    K = np.array([ls.intrinsics(rng, params) for _ in range(3)])
    eng.compute_velocity(cur, des, depth, K, mode=_lib.SELECT_DENSE, num_pairs=k)    # the tables, to draw from
    tabs = eng.last_details(3)
    ids = []
    for b in range(3):
        moved = np.nonzero(tabs["nn_1"][b] != np.arange(t))[0]
        if b == 1:
            ids.append(np.resize(rng.choice(moved, size=1), k).astype(np.int32))
        else:
            ids.append(rng.choice(t, size=k, replace=False).astype(np.int32))
    v, st = eng.compute_velocity(cur, des, depth, K, mode=_lib.SELECT_EXPLICIT, selection=ids, num_pairs=k)
    det = eng.last_details(3)
    v, st = v.cpu().numpy(), st.cpu().numpy()
    for b in range(3):
        assert np.array_equal(det["nn_1"][b], tabs["nn_1"][b]) and int(det["info"][b, 2]) == 0
        s_star, s_, ref = ls.oracle(g, cfg.img_size, params, det["nn_1"][b].astype(np.int64), ids[b], k, depth[b], K[b])
        _check_law(det, b, v[b], st[b], ref, s_star, s_, k, "jacobi" if b == 1 else "ldlt", ("pair", b))
    eng.close()


# ----------------------------------------------------------------------------- the three law options at once
@pytest.mark.parametrize("binned", [False, True])
def test_all_three_law_options_through_every_entry_point(binned):
    """robust_law, subpatch and interaction together on a ViT-S/16 forward (T = 196, fp32): the refinement reads the normalised
    descriptors (plain) or the raw Gram (binned).  The device call, the host call, the reselect seam and a captured update on a
    side stream give the same v_c and the same per-row outputs bit for bit; switching the options off one by one changes the
    replay and returns each getter to its "off" value."""
    cfg = config.baseline_config("vits16_224")
    params = config.ServoParams(dino_input_size=cfg.img_size, use_feature_binning=binned, robust_iterations=2, subpatch=True,
                                interaction="mean")
    eng = Engine(cfg, params, precision="fp32", max_pairs=1).load_state_dict(weights.synthetic_state_dict(cfg, 0))
    des, cur = synth.frame_pair(cfg.img_size, 20250705)
    depth, K, k = synth.depth_pattern(), params.intrinsics(), 24
    zg = (np.ascontiguousarray(depth[::-1, ::-1]).astype(np.int64) + 137).clip(1, 65535).astype(np.uint16)
    eng.set_goal_depth(zg)
    order = np.random.default_rng(11).permutation(cfg.tokens).astype(np.int32)

    def rows():
        return dict(weights=eng.last_weights(1), offsets=eng.last_offsets(1), Z_goal=eng.last_goal_depth(1), **eng.last_features(1))

    def same_rows(what):
        got = rows()
        for key, want in eager.items():
            assert np.array_equal(got[key], want), (what, key)
    v, st = eng.compute_velocity(cur, des, depth, K, mode=_lib.SELECT_ORDER, selection=order, num_pairs=k)
    assert int(st[0]) == _lib.STATUS_OK
    v, det, eager = v.cpu().numpy()[0], eng.last_details(1), rows()
    assert det["offsets"][0, :k].any() and det["Z_goal"][0, :k].all() and int(det["info"][0, 6]) == 2
    rob = rr.robust_velocity(det["L"][0, :6, :2 * k].T, det["L"][0, 6, :2 * k], params.lambda_, 2,
                             rr.sigma_min(cfg.stride, params.u_max, params.v_max, cfg.img_size, K[0], K[1]))
    if rob["margin"] >= 1e-6:
        assert rr.rel_l2(v, rob["v_c"]) <= VC_BAR
    vh, sth = eng.compute_velocity_host(cur, des, depth, K, mode=_lib.SELECT_ORDER, selection=order, num_pairs=k)
    assert int(sth[0]) == _lib.STATUS_OK and np.array_equal(vh[0], v)
    same_rows("host")
    vr, str_ = eng.reselect_host(_lib.SELECT_ORDER, order, num_pairs=k)
    assert int(str_[0]) == _lib.STATUS_OK and np.array_equal(vr[0], v)
    same_rows("reselect")
    # a captured update (a side stream: the default stream is never captured)
    eng.set_option("graph_replay", 1)
    cur_d, des_d = eng._frames(cur), eng._frames(des)
    z_d = torch.as_tensor(depth).reshape(1, params.v_max, params.u_max).to(eng.device).contiguous()
    k_d = torch.as_tensor(K, dtype=torch.float64).reshape(1, 4).to(eng.device)
    sel_d, cnt_d = eng._selection_args(_lib.SELECT_ORDER, order, 1, cfg.tokens, k)
    out_v = torch.zeros((1, 6), dtype=torch.float64, device=eng.device)
    out_s = torch.zeros(1, dtype=torch.int32, device=eng.device)
    side = torch.cuda.Stream(eng.device)
    torch.cuda.synchronize()

    def replayed():
        with torch.cuda.stream(side):
            eng.compute_velocity_dev(cur_d, des_d, z_d, k_d, _lib.SELECT_ORDER, sel_d, cnt_d, out_v=out_v, out_status=out_s, num_pairs=k)
        torch.cuda.synchronize()
        return out_v.cpu().numpy()[0].copy()
    for what in ("captured", "replayed"):
        assert np.array_equal(replayed(), v), what
        same_rows(what)
    eng.set_option("graph_replay", 0)
    ve, _ = eng.compute_velocity(cur, des, depth, K, mode=_lib.SELECT_ORDER, selection=order, num_pairs=k)
    assert np.array_equal(ve.cpu().numpy()[0], v)
    same_rows("eager again")
    # off, one by one
    eng.set_option("graph_replay", 1)
    prev = replayed()
    eng.set_option("robust_law", 0)
    now = replayed()
    assert not np.array_equal(now, prev) and np.all(eng.last_weights(1)[0, :k] == 1.0) and not eng.last_weights(1)[0, k:].any()
    assert eng.last_offsets(1).any() and eng.last_goal_depth(1).any()
    prev = now
    eng.set_option("subpatch", 0)
    now = replayed()
    assert not np.array_equal(now, prev) and not eng.last_offsets(1).any() and eng.last_goal_depth(1).any()
    prev = now
    eng.set_option("interaction", 0)
    now = replayed()
    assert not np.array_equal(now, prev) and not eng.last_goal_depth(1).any() and int(out_s[0]) == _lib.STATUS_OK
    eng.close()


# ----------------------------------------------------------------------------- reselect state
@pytest.mark.parametrize("between", ["set_goal", "extract_descriptors", "correspond"])
def test_reselect_ends_with_calls_that_rewrite_the_keys(between):
    """vitvs_reselect re-runs the law on the arg-max keys a host-pointer velocity call left.  set_goal and extract_descriptors
    (their forward clears or overwrites the keys) and correspond (overwrites them) end that state: reselect then fails with -5
    rather than returning a v_c of foreign keys."""
    eng, cfg, params = _tiny_model(1, 196)
    des, cur = synth.frame_pair(cfg.img_size, 20250705)
    depth = synth.depth_pattern()
    v0, st0 = eng.compute_velocity_host(cur, des, depth, params.intrinsics(), mode=_lib.SELECT_DENSE)
    v1, st1 = eng.reselect_host(_lib.SELECT_DENSE)
    assert np.array_equal(v0, v1) and np.array_equal(st0, st1)
    if between == "set_goal":
        eng.set_goal(des)
    elif between == "extract_descriptors":
        eng.extract_descriptors(np.stack([des, cur]))
    else:
        d = torch.randn(cfg.tokens, cfg.dim, generator=torch.Generator().manual_seed(1))
        eng.correspond(d, d.flip(0))
    torch.cuda.synchronize()
    with pytest.raises(VitvsError, match=r"\(-5\)"):
        eng.reselect_host(_lib.SELECT_DENSE)
    eng.close()
