"""The homography law's consensus start through a handle (vitvs_homography_consensus_velocity[_dev], Engine.homography_velocity(...,
consensus, seed)), on a token grid through ``Engine.servo_from_nn``: the tiny handle without weights and the scenario
shapes of tests/test_gpu_homography.py, restated here, at 24 and 130 rows.

The reference is tests/homography_consensus_ref.py on what the velocity call left (``Engine.last_details``).  Exact: status, the
law's counters, the winner's id and the start weights at 1, and with N = 0 the weights; v_h, H and the weights <= 1e-9, sigma <=
1e-12.  Every comparison asserts on its CPU side that the reference keeps its margins (the winner's cost >= 1e-6 below any other
row set's, no residual within 1e-6 of the cut-off or of a rejection edge, second-smallest eigenvalues >= 1e-4 of the trace,
eigen-gaps >= 1e-6), so that no winner, start weight or status can flip."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib
from vitvs_amd.engine import Engine

import homography_consensus_ref as cr
import homography_ref as hr
import law_support as ls
from law_support import TinyEngines, close_engines  # noqa: F401

pytestmark = pytest.mark.gpu

ENGINES = TinyEngines()           # this module's tiny handles: close_engines closes them at its teardown

G = 14
IMG = 16 * G
_scenario = functools.partial(ls.planted_case, ENGINES, G)
ZHAT = 0.61
M = 256
SEED = 5
FIELDS = Engine.HOMOGRAPHY_INFO_FIELDS + ("winner", "start_weights")


def _reference(det, cam_status, K, lam, n_iter, pitches, n_hyp=M, seed=SEED):
    ref = cr.homography_consensus_from_details(det, 0, cam_status, K, lam, ZHAT, n_iter, *pitches, n_hyp, seed)
    assert ref["gap"] >= 1e-6 and ref["edge_T"] >= 1e-6 and ref["edge"] >= 1e-6 and all(g >= 1e-4 for g in ref["ratios"]) and \
        all(g >= 1e-6 for g in ref["gaps"]), ("choose other inputs", ref["gap"], ref["edge_T"], ref["edge"], ref["ratios"], ref["gaps"])
    return ref


def _compare(v, info, ref, what, n_iter):
    info = ls.host(info)
    v = v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
    assert int(info["status"][0]) == ref["status"], (what, info["status"][0], ref["status"])
    got_info = [int(info[name][0]) for name in FIELDS]
    assert got_info == list(ref["info"]), (what, got_info, ref["info"])
    if n_iter == 0:
        assert np.array_equal(info["weights"][0], ref["start"]), what
    errs = dict(v=np.abs(v[0] - ref["v"]).max(), H=np.abs(info["H"][0] - ref["H"]).max() / max(1.0, np.abs(ref["H"]).max()),
                weights=np.abs(info["weights"][0] - ref["weights"]).max())
    print(f"{what}: " + ", ".join(f"{k} {e:.1e}" for k, e in errs.items()) + f"; winner {ref['info'][6]}, start weights {ref['info'][7]} of "
          f"{ref['info'][0]}, gap {ref['gap']:.1e}, edge_T {ref['edge_T']:.1e}")
    assert all(e <= 1e-9 for e in errs.values()), (what, errs)
    assert float(info["sigma"][0]) == ref["sigma"] or abs(float(info["sigma"][0]) - ref["sigma"]) <= 1e-12, what


def _snapshot(eng, v):
    return dict(eng.last_details(1), v_c=np.array(v, copy=True))


def _c_entry(eng, K, st, n_iter, n_hyp, seed):
    """vitvs_homography_consensus_velocity_dev itself -> (return code, v, h_info, weights)."""
    dev = eng.device
    kd = torch.tensor([K], dtype=torch.float64, device=dev)
    sd = torch.tensor([st], dtype=torch.int32, device=dev)
    v, hs = torch.zeros((1, 6), dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    H, hi = torch.zeros((1, 9), dtype=torch.float64, device=dev), torch.full((1, 8), -1, dtype=torch.int32, device=dev)
    w, sg = torch.zeros((1, eng.max_rows), dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    rc = eng.lib.vitvs_homography_consensus_velocity_dev(eng.handle, 1, p(kd), p(sd), ZHAT, n_iter, n_hyp, seed, p(v), p(hs), p(H), p(hi),
                                                         p(w), p(sg), None)
    torch.cuda.synchronize()
    return rc, dict(v=v.cpu().numpy(), status=hs.cpu().numpy(), H=H.cpu().numpy(), info=hi.cpu().numpy(), weights=w.cpu().numpy(),
                    sigma=sg.cpu().numpy())


@pytest.mark.parametrize("num_pairs", [24, 130])
def test_device_equals_the_reference_with_and_without_a_depth_image(num_pairs):
    """Random intrinsics, 12 % wrong matches, N = 0 and 4 behind 256 hypotheses; the call changes nothing the velocity call left; the
    host-pointer form is the same launch; no hypotheses through the new entry point is homography_velocity bit for bit; and a
    velocity call without a depth image (NO_DEPTH) is followed by the same twist bit for bit."""
    eng, params, sc = _scenario(81000 + num_pairs, num_pairs)
    pitches = ls.pitches(params, 16, IMG)
    v_c, st = ls.servo_law(eng, sc)
    assert st == _lib.STATUS_OK
    before = _snapshot(eng, v_c)
    with_depth = {}
    for n_iter in (0, 4):
        v, info = eng.homography_velocity(sc["K"], [st], ZHAT, n_iter, M, SEED)
        ref = _reference(before, st, sc["K"], params.lambda_, n_iter, pitches)
        assert ref["status"] == hr.OK and ref["info"][6] >= 1 and 4 <= ref["info"][7] < ref["info"][0]
        _compare(v, info, ref, f"{num_pairs} pairs, N = {n_iter}", n_iter)
        v_h, info_h = eng.homography_velocity_host(sc["K"], [st], ZHAT, n_iter, M, SEED)
        assert np.array_equal(v_h, v.cpu().numpy()) and ls.same_values(ls.host(info), info_h)
        with_depth[n_iter] = (v.cpu().numpy(), ls.host(info))
        # no hypotheses: the law as it was, through the old and the new entry point
        v0, info0 = eng.homography_velocity(sc["K"], [st], ZHAT, n_iter)
        rc, got = _c_entry(eng, sc["K"], st, n_iter, 0, SEED)
        info0 = ls.host(info0)
        assert rc == 0 and np.array_equal(got["v"], v0.cpu().numpy()) and np.array_equal(got["H"], info0["H"].reshape(1, 9))
        assert np.array_equal(got["weights"], info0["weights"]) and np.array_equal(got["sigma"], info0["sigma"])
        assert list(got["info"][0]) == [int(info0[name][0]) for name in Engine.HOMOGRAPHY_INFO_FIELDS] + [0, 0]
        assert not info0["winner"].any() and not info0["start_weights"].any()
    assert ls.same_values(_snapshot(eng, v_c), before)                   # v_c and every vitvs_last_* output as the velocity call left them
    v_c, st = ls.servo_law(eng, sc, depth=False)
    assert st == _lib.STATUS_NO_DEPTH and not v_c.any()
    for n_iter in (0, 4):
        v, info = eng.homography_velocity(sc["K"], [st], ZHAT, n_iter, M, SEED)
        assert np.array_equal(v.cpu().numpy(), with_depth[n_iter][0]) and ls.same_values(ls.host(info), with_depth[n_iter][1])


@pytest.mark.parametrize("option", ["subpatch", "robust_law"])
def test_with_the_other_law_options(option):
    """subpatch: the hypotheses are drawn from the moved matches (feat's x, y); robust_law: the camera's own weights do not reach the
    homography law."""
    eng, params, sc = _scenario(82000 + len(option), 24)
    offsets = None
    if option == "subpatch":
        offsets = np.random.default_rng(7).uniform(-0.5, 0.5, size=(G * G, 2)).astype(np.float32)
    else:
        eng.set_option("robust_law", 4)
    v_c, st = ls.servo_law(eng, sc, offsets=offsets)
    assert st == _lib.STATUS_OK
    before = _snapshot(eng, v_c)
    if option == "subpatch":
        assert before["offsets"][0, :24].any()
    pitches = ls.pitches(params, 16, IMG)
    for n_iter in (0, 4):
        v, info = eng.homography_velocity(sc["K"], [st], ZHAT, n_iter, M, SEED)
        _compare(v, info, _reference(before, st, sc["K"], params.lambda_, n_iter, pitches), f"{option}, N = {n_iter}", n_iter)
    assert ls.same_values(_snapshot(eng, v_c), before)
    eng.set_option("robust_law", 0)


@pytest.mark.parametrize("num_pairs", [24, 130])
def test_a_third_of_the_matches_permuted_to_wrong_tokens(num_pairs):
    """No planted outlier but the first third of the selected goal tokens matched to each other's current tokens: the start weights
    drop exactly the rows the reference drops."""
    eng, params, sc = _scenario(83000 + num_pairs, num_pairs, share=0.0)
    third = num_pairs // 3
    ids = np.asarray(sc["ids"], np.int64)
    nn1 = sc["nn_1"].copy()
    nn1[ids[:third]] = np.roll(sc["nn_1"][ids[:third]], third // 2)
    nn2 = np.zeros_like(sc["nn_2"])
    nn2[nn1] = np.arange(len(nn1))
    sc = dict(sc, nn_1=nn1, nn_2=nn2)
    v_c, st = ls.servo_law(eng, sc)
    assert st == _lib.STATUS_OK
    before = _snapshot(eng, v_c)
    pitches = ls.pitches(params, 16, IMG)
    for n_iter in (0, 4):
        v, info = eng.homography_velocity(sc["K"], [st], ZHAT, n_iter, M, SEED)
        ref = _reference(before, st, sc["K"], params.lambda_, n_iter, pitches)
        _compare(v, info, ref, f"{num_pairs} pairs, a third permuted, N = {n_iter}", n_iter)
        if n_iter == 0:
            got = ls.host(info)["weights"][0]
            usable = np.asarray(before["selected"][0]) >= 0
            assert np.array_equal(got == 0.0, ref["start"] == 0.0)
            dropped = usable & (ref["start"] == 0.0)
            assert dropped[:third].any() and dropped.sum() == ref["info"][0] - ref["info"][7]    # (a condition on the inputs)
            print(f"{num_pairs} pairs: {dropped[:third].sum()} of the {usable[:third].sum()} permuted rows dropped (a permuted match "
                  f"within the cut-off of the right one stays), {dropped[third:].sum()} of the others")


def test_error_returns():
    eng, params, sc = _scenario(84000, 24)
    v_c, st = ls.servo_law(eng, sc)
    for bad in (-1, 4097):
        assert _c_entry(eng, sc["K"], st, 4, bad, 0)[0] == -2
    assert _c_entry(eng, sc["K"], st, 17, 256, 0)[0] == -2
    assert _c_entry(eng, sc["K"], st, 4, 4096, 0xFFFFFFFF)[0] == 0
    with pytest.raises(ValueError, match="0 .. 4096"):
        eng.homography_velocity(sc["K"], [st], ZHAT, 4, 5000)
