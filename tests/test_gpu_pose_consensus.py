"""The pose law's consensus start through a handle (vitvs_pose_consensus_velocity[_dev], Engine.pose_velocity(..., consensus, seed);
DESIGN.md §5f): on a token grid through ``Engine.servo_from_nn`` (the tiny handle without weights and the planted scenario of
tests/test_gpu_pose.py at 24 and 130 rows, the goal depth that of the scenario's plane) and through a ViT-S/16 224² fp32 handle's
velocity call, three pairs sharing one goal depth image.

The reference is tests/pose_consensus_ref.py on what the velocity call left (``Engine.last_details``) and the goal-depth table
restated on the host.  Exact: status, the law's counters, the winner's id and the start weights at 1, and with N = 0 the weights;
v_pose, R, t and the weights <= 1e-9, sigma <= 1e-12.  Every comparison asserts on its CPU side that the reference keeps its margins
(the winner's cost >= 1e-6 below any other row set's, no residual within 1e-6 of the cut-off or of a rejection edge, eigen-gaps >=
1e-6), so that no winner, start weight or status can flip."""
import ctypes as C

import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib, config, synth, weights
from vitvs_amd.engine import Engine

import pose_consensus_ref as cr
import pose_ref as pr
import law_support as ls
from law_support import TinyEngines, close_engines  # noqa: F401

pytestmark = pytest.mark.gpu

ENGINES = TinyEngines()           # this module's tiny handles: close_engines closes them at its teardown

G = 14
IMG = 16 * G
M = 256
SEED = 5
FIELDS = Engine.POSE_INFO_FIELDS + ("winner", "start_weights")


def _scenario(seed, num_pairs, share=0.125):
    """(eng, params, scenario, goal depth): the planted scenario and the depth image of its plane at the goal pose, with holes."""
    eng, params, sc = ls.planted_case(ENGINES, G, seed, num_pairs, share)
    zg = np.full((params.v_max, params.u_max), 610, np.uint16)
    zg.reshape(-1)[np.random.default_rng(seed + 1).integers(0, zg.size, size=zg.size // 7)] = 0
    eng.set_goal_depth(zg)
    return eng, params, sc, zg


def _reference(det, b, cam_status, K, table, lam, n_iter, pitches, n_hyp=M, seed=SEED):
    with np.errstate(all="ignore"):
        ref = cr.pose_consensus_from_details(det, b, cam_status, K, table, lam, n_iter, *pitches, n_hyp, seed)
    assert ref["cgap"] >= 1e-6 and ref["edge_T"] >= 1e-6 and ref["edge"] >= 1e-6 and all(g >= 1e-6 for g in ref["gaps"]), \
        ("choose other inputs", ref["cgap"], ref["edge_T"], ref["edge"], ref["gaps"])
    return ref


def _compare(v, info, b, ref, what, n_iter):
    info = ls.host(info)
    v = v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
    assert int(info["status"][b]) == ref["status"], (what, info["status"][b], ref["status"])
    got_info = [int(info[name][b]) for name in FIELDS]
    assert got_info == list(ref["info"]), (what, got_info, ref["info"])
    if n_iter == 0:
        assert np.array_equal(info["weights"][b], ref["start"]), what
    errs = dict(v=np.abs(v[b] - ref["v"]).max(), R=np.abs(info["R"][b] - ref["R"]).max(), t=np.abs(info["t"][b] - ref["t"]).max(),
                weights=np.abs(info["weights"][b] - ref["weights"]).max())
    print(f"{what}: " + ", ".join(f"{k} {e:.1e}" for k, e in errs.items()) + f"; winner {ref['info'][6]}, start weights {ref['info'][7]} of "
          f"{ref['info'][0]}, cost gap {ref['cgap']:.1e}, edge_T {ref['edge_T']:.1e}")
    assert all(e <= 1e-9 for e in errs.values()), (what, errs)
    assert float(info["sigma"][b]) == ref["sigma"] or abs(float(info["sigma"][b]) - ref["sigma"]) <= 1e-12, what


def _c_entry(eng, K, st, n_iter, n_hyp, seed):
    """vitvs_pose_consensus_velocity_dev itself -> (return code, outputs)."""
    dev = eng.device
    kd = torch.tensor([K], dtype=torch.float64, device=dev)
    sd = torch.tensor([st], dtype=torch.int32, device=dev)
    v, ps = torch.zeros((1, 6), dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    pose, pi = torch.zeros((1, 12), dtype=torch.float64, device=dev), torch.full((1, 8), -1, dtype=torch.int32, device=dev)
    w, sg = torch.zeros((1, eng.max_rows), dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    rc = eng.lib.vitvs_pose_consensus_velocity_dev(eng.handle, 1, p(kd), p(sd), n_iter, n_hyp, seed, p(v), p(ps), p(pose), p(pi), p(w),
                                                   p(sg), None)
    torch.cuda.synchronize()
    return rc, dict(v=v.cpu().numpy(), status=ps.cpu().numpy(), pose=pose.cpu().numpy(), info=pi.cpu().numpy(), weights=w.cpu().numpy(),
                    sigma=sg.cpu().numpy())


@pytest.mark.parametrize("num_pairs", [24, 130])
def test_device_equals_the_reference_and_leaves_the_call_untouched(num_pairs):
    """Random intrinsics, holes in both depth images, 12 % wrong matches, N = 0 and 4 behind 256 hypotheses; the call changes nothing
    the velocity call left; the host-pointer form is the same launch; no hypotheses through the new entry point is pose_velocity bit
    for bit."""
    eng, params, sc, zg = _scenario(91000 + num_pairs, num_pairs)
    table, pitches = ls.goal_table(zg, G, IMG, params), ls.pitches(params, 16, IMG)
    v_c, st = ls.servo_law(eng, sc)
    assert st == _lib.STATUS_OK
    before = ls.snapshot(eng, v_c)
    for n_iter in (0, 4):
        v, info = eng.pose_velocity(sc["K"], [st], n_iter, M, SEED)
        ref = _reference(before, 0, st, sc["K"], table, params.lambda_, n_iter, pitches)
        assert ref["status"] == pr.OK and ref["info"][6] >= 1 and 3 <= ref["info"][7] < ref["info"][0]
        _compare(v, info, 0, ref, f"{num_pairs} pairs, N = {n_iter}", n_iter)
        v_h, info_h = eng.pose_velocity_host(sc["K"], [st], n_iter, M, SEED)
        assert np.array_equal(v_h, v.cpu().numpy()) and ls.same_values(ls.host(info), info_h)
        # no hypotheses: the law as it was, through the old and the new entry point
        v0, info0 = eng.pose_velocity(sc["K"], [st], n_iter)
        rc, got = _c_entry(eng, sc["K"], st, n_iter, 0, SEED)
        info0 = ls.host(info0)
        assert rc == 0 and np.array_equal(got["v"], v0.cpu().numpy())
        assert np.array_equal(got["pose"][:, :9], info0["R"].reshape(1, 9)) and np.array_equal(got["pose"][:, 9:], info0["t"])
        assert np.array_equal(got["weights"], info0["weights"]) and np.array_equal(got["sigma"], info0["sigma"])
        assert list(got["info"][0]) == [int(info0[name][0]) for name in Engine.POSE_INFO_FIELDS] + [0, 0]
        assert not info0["winner"].any() and not info0["start_weights"].any()
        plain = pr.pose_from_details(before, 0, st, sc["K"], table, params.lambda_, n_iter, *pitches)
        assert np.abs(v0.cpu().numpy()[0] - plain["v"]).max() <= 1e-9
    assert ls.same_values(ls.snapshot(eng, v_c), before)                   # v_c and every vitvs_last_* output as the velocity call left them


@pytest.mark.parametrize("option", ["subpatch", "robust_law"])
def test_with_the_other_law_options(option):
    """subpatch: the hypotheses are drawn from the moved matches (feat's x, y) and the depth under them; robust_law: the camera's own
    weights do not reach the pose law."""
    eng, params, sc, zg = _scenario(92000 + len(option), 24)
    offsets = None
    if option == "subpatch":
        offsets = np.random.default_rng(7).uniform(-0.5, 0.5, size=(G * G, 2)).astype(np.float32)
    else:
        eng.set_option("robust_law", 4)
    v_c, st = ls.servo_law(eng, sc, offsets=offsets)
    assert st == _lib.STATUS_OK
    before = ls.snapshot(eng, v_c)
    if option == "subpatch":
        assert before["offsets"][0, :24].any()
    table, pitches = ls.goal_table(zg, G, IMG, params), ls.pitches(params, 16, IMG)
    for n_iter in (0, 4):
        v, info = eng.pose_velocity(sc["K"], [st], n_iter, M, SEED)
        _compare(v, info, 0, _reference(before, 0, st, sc["K"], table, params.lambda_, n_iter, pitches), f"{option}, N = {n_iter}", n_iter)
    assert ls.same_values(ls.snapshot(eng, v_c), before)
    eng.set_option("robust_law", 0)


@pytest.mark.parametrize("num_pairs", [24, 130])
def test_a_third_of_the_matches_permuted_to_wrong_tokens(num_pairs):
    """No planted outlier but the first third of the selected goal tokens matched to each other's current tokens: the start weights
    drop exactly the rows the reference drops."""
    eng, params, sc, zg = _scenario(93000 + num_pairs, num_pairs, share=0.0)
    third = num_pairs // 3
    ids = np.asarray(sc["ids"], np.int64)
    nn1 = sc["nn_1"].copy()
    nn1[ids[:third]] = np.roll(sc["nn_1"][ids[:third]], third // 2)
    nn2 = np.zeros_like(sc["nn_2"])
    nn2[nn1] = np.arange(len(nn1))
    sc = dict(sc, nn_1=nn1, nn_2=nn2)
    v_c, st = ls.servo_law(eng, sc)
    assert st == _lib.STATUS_OK
    before = ls.snapshot(eng, v_c)
    table, pitches = ls.goal_table(zg, G, IMG, params), ls.pitches(params, 16, IMG)
    for n_iter in (0, 4):
        v, info = eng.pose_velocity(sc["K"], [st], n_iter, M, SEED)
        ref = _reference(before, 0, st, sc["K"], table, params.lambda_, n_iter, pitches)
        _compare(v, info, 0, ref, f"{num_pairs} pairs, a third permuted, N = {n_iter}", n_iter)
        if n_iter == 0:
            got = ls.host(info)["weights"][0]
            assert np.array_equal(got == 0.0, ref["start"] == 0.0)
            n_dropped = int(ref["info"][0] - ref["info"][7])
            assert n_dropped > 0 and n_dropped == ref["info"][3]                             # (a condition on the inputs)
            print(f"{num_pairs} pairs: {n_dropped} of {ref['info'][0]} usable rows start at weight 0 ({third} matches permuted; a "
                  f"permuted match within the cut-off of the right one stays)")


def test_error_returns():
    eng, params, sc, zg = _scenario(94000, 24)
    v_c, st = ls.servo_law(eng, sc)
    for bad in (-1, 4097):
        assert _c_entry(eng, sc["K"], st, 4, bad, 0)[0] == -2
    assert _c_entry(eng, sc["K"], st, 17, 256, 0)[0] == -2
    assert _c_entry(eng, sc["K"], st, 4, 4096, 0xFFFFFFFF)[0] == 0
    with pytest.raises(ValueError, match="0 .. 4096"):
        eng.pose_velocity(sc["K"], [st], 4, 5000)


def test_three_pairs_of_a_vits16_handle_share_one_goal_depth():
    """ViT-S/16 224², fp32, synthetic weights: three pairs with draws of their own through the forward's velocity call, one goal depth
    image (n_goal = 1) for the three."""
    cfg = config.baseline_config("vits16_224")
    params = config.ServoParams(dino_input_size=cfg.img_size, use_feature_binning=False)
    eng = Engine(cfg, params, precision="fp32", max_pairs=3).load_state_dict(weights.synthetic_state_dict(cfg, 0))
    des, cur = synth.frame_pair(cfg.img_size, 20250705)
    depth, K = synth.depth_pattern(), params.intrinsics()
    zg = ls.goal_depth(np.random.default_rng(65))
    n = 3
    three = lambda a: np.stack([a] * n)   # noqa: E731
    orders = np.stack([np.random.default_rng(70 + b).permutation(cfg.tokens) for b in range(n)]).astype(np.int32)
    eng.set_goal_depth(zg)
    pitches = ls.pitches(params, cfg.stride, cfg.img_size)
    v_c, st = eng.compute_velocity(three(cur), three(des), three(depth), K, mode=_lib.SELECT_ORDER, selection=orders)
    st_h = st.cpu().numpy()
    assert not st_h.any()
    before = dict(eng.last_details(n), v_c=v_c.cpu().numpy().copy())
    table = ls.goal_table(zg, cfg.grid, cfg.img_size, params)
    for n_iter in (0, 4):
        v, info = eng.pose_velocity(K, st, n_iter, M, SEED)
        for b in range(n):
            ref = _reference(before, b, st_h[b], K, table, params.lambda_, n_iter, pitches)
            _compare(v, info, b, ref, f"ViT-S/16, pair {b}, N = {n_iter}", n_iter)
        v_h, info_h = eng.pose_velocity_host(K, st_h, n_iter, M, SEED)
        assert np.array_equal(v_h, v.cpu().numpy()) and ls.same_values(ls.host(info), info_h)
        v0, info0 = eng.pose_velocity(K, st, n_iter)                    # consensus = 0: the law as it was
        v1, info1 = eng.pose_velocity(K, st, n_iter, 0, SEED)
        assert np.array_equal(v0.cpu().numpy(), v1.cpu().numpy()) and ls.same_values(ls.host(info0), ls.host(info1))
        assert not ls.host(info0)["winner"].any()
    assert ls.same_values(dict(eng.last_details(n), v_c=v_c.cpu().numpy()), before)
    eng.close()
