"""Selection mode BEST through every entry point, by one identity (GPU): a BEST call returns v_c, status and every field of
vitvs_last_details bit for bit equal to the same call in ORDER mode given tests/select_ref.py's order of the tables the call
reports, and vitvs_last_order is that order.  The law behind the selection is the one ORDER runs (tests/test_gpu_servo_cover.py
holds it to the oracle), so nothing here has a tolerance."""
import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib, config, synth, weights
from vitvs_amd.engine import Engine, VitvsError
from vitvs_amd.pipeline import UpdatePipeline
import select_ref as sref
import law_support as ls
from law_support import TinyEngines, close_engines  # noqa: F401

pytestmark = pytest.mark.gpu

ENGINES = TinyEngines()           # this module's tiny handles: close_engines closes them at its teardown


def _reference_orders(det, n, cells):
    return np.stack([sref.best_order(det["nn_1"][b], det["nn_2"][b], det["sim_1"][b], cells) for b in range(n)])


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), what


def _same_details(det_b, det_o, what):
    assert set(det_b) == set(det_o)
    for key in det_b:
        _same_bits(det_b[key], det_o[key], (what, key))


def _identity(eng, n, run, cells=4, what=""):
    """run(mode, order) -> (v, st) as numpy; BEST against ORDER on the reference's order.  Returns the BEST call's details."""
    vb, sb = run(_lib.SELECT_BEST, None)
    det_b, order_dev = eng.last_details(n), eng.last_order(n)
    want = _reference_orders(det_b, n, cells)
    assert np.array_equal(order_dev, want), (what, "vitvs_last_order is not the reference's order")
    vo, so = run(_lib.SELECT_ORDER, want)
    _same_bits(vb, vo, (what, "v_c"))
    _same_bits(sb, so, (what, "status"))
    _same_details(det_b, eng.last_details(n), what)
    return det_b, vb, sb


@pytest.fixture(scope="module")
def model():
    """The 2-block tiny model at 224 (T = 196), three pairs of capacity, with its frames."""
    cfg = ls.tiny_cfg(224)
    params = config.ServoParams(dino_input_size=224, use_feature_binning=False)
    sd = weights.synthetic_state_dict(cfg, 3)
    eng = Engine(cfg, params, precision="fp32", max_pairs=3, max_rows=196).load_state_dict(sd)
    pairs = [synth.frame_pair(cfg.img_size, s) for s in (20250705, 20250715, 20250738)]
    rng = np.random.default_rng(5)
    depth = np.stack([ls.depth(rng), np.roll(synth.depth_pattern(), 37, axis=1), (synth.depth_pattern() // 2 + 300).astype(np.uint16)])
    yield dict(eng=eng, cfg=cfg, params=params, sd=sd, des=np.stack([p[0] for p in pairs]), cur=np.stack([p[1] for p in pairs]),
               depth=depth, K=params.intrinsics())
    eng.close()


def _np(v, st):
    return v.cpu().numpy(), st.cpu().numpy()


# ----------------------------------------------------------------------------- the law on given tables
@pytest.mark.parametrize("rows", [24, 130])
@pytest.mark.parametrize("g", [14, 17, 32])
def test_servo_from_nn(g, rows):
    t = g * g
    rng = np.random.default_rng(100 * g + rows)
    eng, params = ENGINES.fetch(g, 160)
    nn1, nn2, sim1, _ = ls.tables(rng, t, int(rng.integers(t // 4, t // 2)))
    depth, K = ls.depth(rng), params.intrinsics()

    def run(mode, order):
        return _np(*eng.servo_from_nn(nn1, nn2, sim1, depth, K, mode=mode, selection=order, num_pairs=rows))
    det, v, st = _identity(eng, 1, run, what=(g, rows))
    assert int(st) in (_lib.STATUS_OK, _lib.STATUS_TOO_FEW)
    n = int(det["info"][0, 3])
    assert det["selected"][0, :n].tolist() == sref.selected(nn1, nn2, sim1, rows).tolist()
    if int(st) == _lib.STATUS_OK:
        assert np.any(v != 0)


def test_servo_from_nn_with_other_cells_and_back():
    """select_cells between calls: `selected` follows the reference at every setting, and the orders differ."""
    g, rows = 17, 24
    t = g * g
    rng = np.random.default_rng(4)
    eng, params = ENGINES.fetch(g, 160)
    nn1, nn2, sim1, _ = ls.tables(rng, t, 140)
    depth, K = ls.depth(rng), params.intrinsics()

    def run(mode, order):
        return _np(*eng.servo_from_nn(nn1, nn2, sim1, depth, K, mode=mode, selection=order, num_pairs=rows))
    picked = {}
    try:
        for cells in (1, 4, 16, 4):
            eng.set_option("select_cells", cells)
            det, _, _ = _identity(eng, 1, run, cells=cells, what=("cells", cells))
            got = det["selected"][0, :rows].tolist()
            assert got == sref.selected(nn1, nn2, sim1, rows, cells).tolist()
            assert picked.setdefault(cells, got) == got
        assert picked[1] != picked[4] and picked[4] != picked[16]
        for bad in (0, 17):
            with pytest.raises(VitvsError, match=r"\(-5\)"):
                eng.set_option("select_cells", bad)
    finally:
        eng.set_option("select_cells", 4)


# ----------------------------------------------------------------------------- through the forward
def test_compute_velocity_dev_one_pair(model):
    eng, m = model["eng"], model

    def run(mode, order):
        return _np(*eng.compute_velocity(m["cur"][:1], m["des"][:1], m["depth"][:1], m["K"], mode=mode, selection=order, num_pairs=24))
    det, v, st = _identity(eng, 1, run, what="one pair")
    assert int(st[0]) == _lib.STATUS_OK and np.any(v != 0)


def test_compute_velocity_dev_three_pairs_sharing_a_goal(model):
    eng, m = model["eng"], model

    def run(mode, order):
        return _np(*eng.compute_velocity(m["cur"], m["des"][:1], m["depth"], m["K"], mode=mode, selection=order, des_shared=True,
                                         num_pairs=24))
    det, v, st = _identity(eng, 3, run, what="three pairs")
    assert not np.array_equal(eng.last_details(3)["selected"][0], eng.last_details(3)["selected"][1])
    # ... and three pairs of their own goals
    def run2(mode, order):
        return _np(*eng.compute_velocity(m["cur"], m["des"], m["depth"], m["K"], mode=mode, selection=order, num_pairs=24))
    _identity(eng, 3, run2, what="three pairs, three goals")


def test_host_call_and_reselect(model):
    eng, m = model["eng"], model

    def run(mode, order):
        return eng.compute_velocity_host(m["cur"][:1], m["des"][:1], m["depth"][:1], m["K"], mode, order, num_pairs=24)
    det, v, st = _identity(eng, 1, run, what="host")
    # the law again on what the host call left: BEST, then ORDER on the same order, and BEST after a DENSE host call
    def again(mode, order):
        return eng.reselect_host(mode, order, num_pairs=24)
    det_r, v_r, st_r = _identity(eng, 1, again, what="reselect")
    _same_bits(v_r, v, "reselect v_c")
    _same_details(det_r, det, "reselect details")
    eng.compute_velocity_host(m["cur"][:1], m["des"][:1], m["depth"][:1], m["K"], _lib.SELECT_DENSE, num_pairs=24)
    v_d, st_d = eng.reselect_host(_lib.SELECT_BEST, num_pairs=24)
    _same_bits(v_d, v, "reselect after DENSE")
    assert np.array_equal(eng.last_order(1), _reference_orders(det, 1, 4))


def test_graph_replay(model):
    """A captured update (a side stream: the default stream is never captured): the first call captures, the second replays."""
    eng, m = model["eng"], model
    p = m["params"]
    eng.set_option("graph_replay", 1)
    try:
        cur_d, des_d = eng._frames(m["cur"][:1]), eng._frames(m["des"][:1])
        z_d = torch.as_tensor(m["depth"][:1]).to(eng.device).contiguous()
        k_d = torch.as_tensor(m["K"], dtype=torch.float64).reshape(1, 4).to(eng.device)
        out_v = torch.zeros((1, 6), dtype=torch.float64, device=eng.device)
        out_s = torch.zeros(1, dtype=torch.int32, device=eng.device)
        side = torch.cuda.Stream(eng.device)
        torch.cuda.synchronize()

        def run(mode, order):
            sel = None if order is None else torch.from_numpy(np.ascontiguousarray(order)).to(eng.device)
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                eng.compute_velocity_dev(cur_d, des_d, z_d, k_d, mode, sel, None, out_v=out_v, out_status=out_s, num_pairs=24)
            torch.cuda.synchronize()
            return out_v.cpu().numpy().copy(), out_s.cpu().numpy().copy()
        det1, v1, st1 = _identity(eng, 1, run, what="captured")
        det2, v2, st2 = _identity(eng, 1, run, what="replayed")
        _same_bits(v1, v2, "replay v_c")
        _same_details(det1, det2, "replay details")
        # the option is part of what a captured update holds: changing it drops the graphs, the replay follows
        eng.set_option("select_cells", 1)
        det3, v3, _ = _identity(eng, 1, run, cells=1, what="replayed, one cell")
        assert det3["selected"][0, :24].tolist() != det1["selected"][0, :24].tolist()
    finally:
        eng.set_option("select_cells", 4)
        eng.set_option("graph_replay", 0)
    v_e, st_e = _np(*eng.compute_velocity(m["cur"][:1], m["des"][:1], m["depth"][:1], m["K"], mode=_lib.SELECT_BEST, num_pairs=24))
    _same_bits(v_e, v1, "eager against captured")


def test_update_pipeline_of_two_slots(model):
    m = model
    pipe = UpdatePipeline(m["cfg"], m["params"], m["sd"], precision="fp32", depth=2, max_rows=196)
    try:
        dev = pipe.engines[0].device
        Ic = [torch.from_numpy(m["cur"][b:b + 1]).to(dev) for b in range(2)]
        Id = [torch.from_numpy(m["des"][b:b + 1]).to(dev) for b in range(2)]
        Z = [torch.from_numpy(m["depth"][b:b + 1]).to(dev) for b in range(2)]
        K = torch.tensor([m["K"]], dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        tickets = [pipe.submit(Ic[b], Id[b], Z[b], K, _lib.SELECT_BEST, None, None, False, 24) for b in range(2)]
        best = [tuple(x.cpu().numpy().copy() for x in pipe.result(t)) for t in tickets]
        pipe.synchronize()
        dets = [pipe.engines[b].last_details(1) for b in range(2)]
        orders = [_reference_orders(dets[b], 1, 4) for b in range(2)]
        for b in range(2):
            assert np.array_equal(pipe.engines[b].last_order(1), orders[b]), b
        sel = [torch.from_numpy(orders[b]).to(dev) for b in range(2)]
        torch.cuda.synchronize()
        tickets = [pipe.submit(Ic[b], Id[b], Z[b], K, _lib.SELECT_ORDER, sel[b], None, False, 24) for b in range(2)]
        plain = [tuple(x.cpu().numpy().copy() for x in pipe.result(t)) for t in tickets]
        pipe.synchronize()
        for b in range(2):
            _same_bits(best[b][0], plain[b][0], ("slot", b, "v_c"))
            _same_bits(best[b][1], plain[b][1], ("slot", b, "status"))
            _same_details(dets[b], pipe.engines[b].last_details(1), ("slot", b))
        assert not np.array_equal(best[0][0], best[1][0])
    finally:
        pipe.close()


# ----------------------------------------------------------------------------- with the law's options, and the laws behind it
def test_with_the_three_law_options_on(model):
    eng, m = model["eng"], model
    zg = (np.ascontiguousarray(m["depth"][0][::-1, ::-1]).astype(np.int64) + 137).clip(1, 65535).astype(np.uint16)
    eng.set_goal_depth(zg)
    for name, value in (("robust_law", 4), ("subpatch", 1), ("interaction", 2)):
        eng.set_option(name, value)
    try:
        def run(mode, order):
            return _np(*eng.compute_velocity(m["cur"][:1], m["des"][:1], m["depth"][:1], m["K"], mode=mode, selection=order, num_pairs=24))
        det, v, st = _identity(eng, 1, run, what="options on")
        assert int(st[0]) == _lib.STATUS_OK and int(det["info"][0, 6]) == 4 and det["Z_goal"][0, :24].all()

        def host(mode, order):
            return eng.compute_velocity_host(m["cur"][:1], m["des"][:1], m["depth"][:1], m["K"], mode, order, num_pairs=24)
        det_h, v_h, _ = _identity(eng, 1, host, what="options on, host")
        _same_bits(v_h, v, "host against device")
    finally:
        for name in ("robust_law", "subpatch", "interaction"):
            eng.set_option(name, 0)
        eng.set_goal_depth(None)


def test_follow_on_laws_read_what_a_best_call_left(model):
    """One of each family behind a BEST call: the pose law, the homography law and the rig law give bit for bit what they give
    behind the ORDER call on the same order."""
    eng, m = model["eng"], model
    zg = (np.ascontiguousarray(m["depth"][0][::-1, ::-1]).astype(np.int64) + 137).clip(1, 65535).astype(np.uint16)
    eng.set_goal_depth(zg)
    W = np.stack([np.eye(6)] * 2)
    try:
        def behind(mode, order):
            v, st = eng.compute_velocity(m["cur"][:2], m["des"][:2], m["depth"][:2], m["K"], mode=mode, selection=order, num_pairs=24)
            out = {}
            vp, ip = eng.pose_velocity(m["K"], st, 2)
            out.update({"pose_v": vp, **{"pose_" + k: x for k, x in ip.items()}})
            vh, ih = eng.homography_velocity(m["K"], st, 0.6, 0)
            out.update({"hom_v": vh, **{"hom_" + k: x for k, x in ih.items()}})
            vr, rst, ir = eng.rig_velocity(W, st)
            out.update({"rig_v": vr, "rig_normal": ir["normal"]})
            torch.cuda.synchronize()
            return {k: (x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)) for k, x in out.items()}, int(rst)
        best, rst_b = behind(_lib.SELECT_BEST, None)
        order = _reference_orders(eng.last_details(2), 2, 4)
        plain, rst_o = behind(_lib.SELECT_ORDER, order)
        assert rst_b == rst_o == _lib.STATUS_OK and np.any(best["rig_v"] != 0)
        for key in best:
            _same_bits(best[key], plain[key], key)
        print("pose statuses", best["pose_status"], "homography statuses", best["hom_status"])
    finally:
        eng.set_goal_depth(None)


# ----------------------------------------------------------------------------- statuses, determinism, state
def test_same_image_pair(model):
    eng, m = model["eng"], model

    def run(mode, order):
        return _np(*eng.compute_velocity(m["des"][:1], m["des"][:1], m["depth"][:1], m["K"], mode=mode, selection=order, num_pairs=24))
    det, v, st = _identity(eng, 1, run, what="same image")
    assert int(det["info"][0, 2]) == 1 and int(st[0]) == _lib.STATUS_OK and np.all(v == 0)


def test_best_is_deterministic_where_order_jitters(model):
    eng, m = model["eng"], model

    def call(mode, order=None):
        v, st = _np(*eng.compute_velocity(m["cur"][:1], m["des"][:1], m["depth"][:1], m["K"], mode=mode, selection=order, num_pairs=24))
        return v, st, eng.last_details(1)
    v1, st1, det1 = call(_lib.SELECT_BEST)
    v2, st2, det2 = call(_lib.SELECT_BEST)
    _same_bits(v1, v2, "two BEST calls")
    _same_details(det1, det2, "two BEST calls")
    rng = np.random.default_rng(1)
    twists = [call(_lib.SELECT_ORDER, rng.permutation(196).astype(np.int32))[0].tobytes() for _ in range(8)]
    assert len(set(twists)) > 1                                  # the jitter the mode removes


def test_a_best_call_leaves_no_trace_in_an_order_call(model):
    eng, m = model["eng"], model
    order = np.random.default_rng(2).permutation(196).astype(np.int32)

    def call(mode, sel=None):
        v, st = _np(*eng.compute_velocity(m["cur"][:1], m["des"][:1], m["depth"][:1], m["K"], mode=mode, selection=sel, num_pairs=24))
        return v, st, eng.last_details(1)
    va, sa, da = call(_lib.SELECT_ORDER, order)
    with pytest.raises(VitvsError, match=r"\(-5\)"):             # the last law call was not BEST
        eng.last_order(1)
    call(_lib.SELECT_BEST)
    assert sorted(eng.last_order(1)[0].tolist()) == list(range(196))
    vb, sb, db = call(_lib.SELECT_ORDER, order)
    _same_bits(va, vb, "ORDER, BEST, ORDER")
    _same_details(da, db, "ORDER, BEST, ORDER")
    with pytest.raises(VitvsError, match=r"\(-5\)"):
        eng.last_order(1)
    # mode 4 is still refused, and BEST takes no arrays
    with pytest.raises(VitvsError, match=r"\(-5\)"):
        eng.compute_velocity(m["cur"][:1], m["des"][:1], m["depth"][:1], m["K"], mode=4, selection=order, num_pairs=24)
    assert eng._selection_args(_lib.SELECT_BEST, None, 1, 196, 24) == (None, None)
    assert eng._selection_arrays_host(_lib.SELECT_BEST, None, 1, 24) == (None, None)


def test_engine_takes_select_cells_from_its_params(model):
    m = model
    params = m["params"].replace(select_cells=2)
    eng = Engine(m["cfg"], params, precision="fp32", max_pairs=1, max_rows=196).load_state_dict(m["sd"])
    try:
        assert eng.params.select_cells == 2

        def run(mode, order):
            return _np(*eng.compute_velocity(m["cur"][:1], m["des"][:1], m["depth"][:1], m["K"], mode=mode, selection=order, num_pairs=24))
        det, _, _ = _identity(eng, 1, run, cells=2, what="select_cells=2")
        want = sref.selected(det["nn_1"][0], det["nn_2"][0], det["sim_1"][0], 24, 2)
        assert det["selected"][0, :len(want)].tolist() == want.tolist()
        run(_lib.SELECT_BEST, None)                               # (the identity ended with its ORDER call)
        assert not np.array_equal(eng.last_order(1)[0], sref.best_order(det["nn_1"][0], det["nn_2"][0], det["sim_1"][0], 4))
    finally:
        eng.close()
