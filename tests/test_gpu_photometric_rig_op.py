"""The photometric rig law on the device (vitvs_photometric_rig_velocity[_dev], photometric.hip) against
tests/photometric_rig_ref.py, the law in fp64 numpy (GPU).  The cases, their crops and the rule by which a run would be left out of
the exact comparisons are tests/photometric_rig_cases.py's; no run is left out (asserted here and, on the CPU, in
tests/test_photometric_rig_host.py).  Each case runs with N = 0, 1, 4 re-weightings, the lighting model on and off.

Asserted:
  * exactly: the status and every count of rig_info (live cameras, n_total, rows of final weight 0, re-weightings run, holes, a
    pivot failed, the pooled size), and the median bin of the last re-weighting (read off sigma: sigma_min is below a bin's scale);
  * N = 0, where every term is formed by the reference's own operations: each camera's 45 sums within (n + 16) 2^-53 sum |term| of the
    reference's.  (With N > 0 the weights come from the solve before, whose last digits differ: the bound's premise is gone; the
    largest ratio is printed.)  v_rig, gamma_i and beta_i within 1e-9 of the reference's solve of the DEVICE's own sums;
  * over all runs: v_rig (relative L2), gamma_i, beta_i (absolute) and sum w_i (relative) within ten times the reference's distance
    to itself with every camera's rows summed in reversed order and the cameras added in descending order (both printed);
  * bit for bit: one camera with cVr = I against vitvs_photometric_robust_velocity_dev; two calls; the host form against the _dev
    form; a captured graph replayed against the eager call; a dead camera against the call without it; at N = 0, each camera's own
    45 sums with the cameras, cVr and K permuted alike (with N > 0 a camera's weights follow x, and x the order of the sum over
    the cameras: there the counts and the status are compared);
  * every refusal; the velocity path's state and the other photometric laws' outputs untouched by a rig call, and the reverse.

Measured (MI355X, profiles/photometric_rig.txt), the largest over the 42 runs: the device against the reference 7.2e-11 (v_rig),
9.9e-12 (gamma), 1.7e-9 (beta), 1.8e-12 (sum w); the reference against itself in reversed order 6.6e-11, 1.7e-11, 2.9e-9, 1.6e-12.  The
crops hold two or three texels of the scene, a third of one camera's under a block: (gamma, beta) and the twist are badly
conditioned, for both sides alike.  With N = 4 a camera's sums are up to 21 times the N = 0 bound away from the reference's."""
import ctypes as C

import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib, config, synth, weights
from vitvs_amd.engine import Engine
import law_support as ls
import photometric_ref as pr
import photometric_robust_ref as rr
import photometric_rig_ref as rg
import photometric_rig_cases as pc

pytestmark = pytest.mark.gpu

MU, LAM, SMIN = pc.MU, pc.LAM, pc.SMIN
U = 2.0 ** -53


@pytest.fixture(scope="module")
def eng():
    cfg = ls.tiny_cfg(64)
    params = config.ServoParams(dino_input_size=64, use_feature_binning=False)
    e = Engine(cfg, params, precision="fp32", max_pairs=5, max_rows=48).load_state_dict(weights.synthetic_state_dict(cfg, 0))
    yield e
    e.close()


_DEVICE = {}


def _call(eng, name, illum, N, host=False, order=None, smin=SMIN):
    cams, H, W, level, _, _, _, inter, _ = pc.CASES[name]
    cur, des, Z, scalar, K, W6, live = pc.fixture(name)
    if order is not None:
        cur, des, K, W6 = cur[order], des[order], K[order], W6[order]
        Z = None if Z is None else Z[order]
        live = None if live is None else [live[i] for i in order]
    form = eng.photometric_rig_velocity_host if host else eng.photometric_rig_velocity
    v, info = form(cur, des, Z, K, W6, live, level, inter, MU, LAM, scalar, bool(illum), N, smin)
    return (v if host else v.cpu().numpy()), info


def _device(eng, name, illum, N):
    key = (name, illum, N)
    if key not in _DEVICE:
        _DEVICE[key] = _call(eng, name, illum, N)
    return _DEVICE[key]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _rinfo(info):
    return [info["live"], info["n"], info["zero_weight"], info["reweightings"], info["holes"], int(info["pivot_failed"]), *info["pooled"]]


FLOATS = ("normal", "rig_normal", "gamma", "bias", "sigma", "weight")


def _same(v1, i1, v2, i2):
    return (np.array_equal(_bits(v1), _bits(v2)) and all(np.array_equal(_bits(i1[k]), _bits(i2[k])) for k in FLOATS)
            and i1["status"] == i2["status"] and _rinfo(i1) == _rinfo(i2))


def _bin_of(sigma):
    return int(round(sigma / rr.MAD_SCALE * rr.BIN_SCALE - 0.5))


def test_no_run_is_left_out_and_the_cases_reach_the_paths_they_name():
    plans = {name: pr.plan(c[1], c[2], c[3]) for name, c in pc.CASES.items()}
    assert plans["2cam-24x32-l0"][2:4] == (1, 24) and plans["2cam-70x24-l0"][3] == 70 > 64
    assert plans["3cam-41x54-l1"][:2] == (20, 27) and 54 % 4 == 2
    assert len(pc.CASES["5cam-24x32-l0"][0]) == 5 > 4
    out = [run for run in pc.RUNS if pc.left_out(pc.reference(*run))]
    assert not out, out
    for name, illum, N in pc.RUNS:
        assert pc.reference(name, illum, N)["status"] == pr.OK, (name, illum, N)
    assert pc.reference("3cam-dead", 1, 4)["info"][0] == 2 and pc.reference("3cam-holes", 1, 4)["info"][4] == 22 * 30
    for name in pc.CASES:                                       # the planted block is set aside
        assert pc.reference(name, 1, 4)["zeros"][0] > 20, name


@pytest.mark.parametrize("name,illum,N", pc.RUNS, ids=lambda x: str(x))
def test_a_run_against_the_reference(eng, name, illum, N):
    ref = pc.reference(name, illum, N)
    v, info = _device(eng, name, illum, N)
    assert info["status"] == ref["status"] == pr.OK
    assert _rinfo(info) == list(ref["info"]), (_rinfo(info), list(ref["info"]))
    adds = [i for i in range(len(ref["n"])) if ref["n"][i] > 0]
    for i in range(len(ref["n"])):
        if i not in adds:                                       # a dead camera, a camera without a row: zeros everywhere
            assert not info["normal"][i].any() and not info["gamma"][i] and not info["bias"][i] and not info["weight"][i]
            assert info["sigma"][i] == 0.0
    if N > 0:
        last = ref["passes"][-1]
        assert ref["robust"][adds[0], 2] > SMIN and _bin_of(ref["robust"][adds[0], 2]) == last["bin"]
        bins = {_bin_of(float(info["sigma"][i])) for i in adds}
        print(f"{name} illumination {illum} N {N}: median bin {sorted(bins)} (reference {last['bin']}; margins: {ref['margin_m']} rows, "
              f"{ref['margin_e']:.2e} bins to an edge, |t - 1| >= {ref['margin_t']:.2e}), rows of weight 0 {info['zero_weight']} of {info['n']}")
        assert bins == {last["bin"]}
        assert all(info["sigma"][i] == info["sigma"][adds[0]] for i in adds)                    # one sigma for the stack
    else:
        assert not info["sigma"].any() and info["zero_weight"] == 0
    # the 45 sums per camera
    worst = 0.0
    for i in adds:
        err = np.abs(info["normal"][i] - ref["normal"][i])
        bound = (int(ref["n"][i]) + 16) * U * ref["abs"][i]
        worst = max(worst, float(np.max(np.where(bound > 0, err / np.maximum(bound, 1e-300), 0.0))))
        if N == 0:
            assert np.all(err <= bound), (name, i, [rr.NAMES[q] for q in np.nonzero(err > bound)[0]])
    print(f"{name} illumination {illum} N {N}: largest |sum - reference| / ((n + 16) 2^-53 sum |term|) over the cameras' 45 sums: {worst:.3f}"
          + ("" if N == 0 else " (not asserted: the weights follow the solve before)"))
    if N == 0:
        # the solve of the device's own sums, by the reference's arithmetic
        cVr = pc.fixture(name)[5]
        rn, factors = np.zeros(28), {}
        for i in adds:
            T, Wg, factors[i], good = rg.camera_system(info["normal"][i], cVr[i], illum)
            assert good
            rn[:21] += T
            rn[21:27] += Wg
            rn[27] += info["normal"][i][27]
        assert np.allclose(info["rig_normal"], rn, rtol=1e-12, atol=1e-12 * np.abs(rn).max())
        own_v, solved = pr.solve(rn, MU, LAM)
        x, _ = pr.solve(rn, MU, 1.0)
        assert solved and np.linalg.norm(v - own_v) <= 1e-9 * np.linalg.norm(own_v)
        for i in adds:
            if illum:
                gamma, beta = rg._lighting(info["normal"][i], factors[i], rg.camera_step(cVr[i], x))
                assert abs(info["gamma"][i] - gamma) <= 1e-9 * max(1.0, abs(gamma)) and abs(info["bias"][i] - beta) <= 1e-9 * max(1.0, abs(beta))
            else:
                assert info["gamma"][i] == 0.0 and info["bias"][i] == 0.0
            assert info["weight"][i] == float(ref["n"][i])


def _gaps(v, gamma, beta, weight, ref):
    adds = ref["n"] > 0
    return np.array([np.linalg.norm(v - ref["v"]) / max(np.linalg.norm(ref["v"]), 1e-300),
                     np.max(np.abs(gamma[adds] - ref["robust"][adds, 0])), np.max(np.abs(beta[adds] - ref["robust"][adds, 1])),
                     np.max(np.abs(weight[adds] - ref["robust"][adds, 3]) / ref["robust"][adds, 3])])


def test_gaps_over_all_runs(eng):
    """v_rig (relative L2), gamma_i, beta_i (absolute) and sum w_i (relative), the largest over the cameras and over every run, of the
    device against the reference, and of the reference against itself summed in reversed order: at most ten times."""
    gap_dev, gap_self = np.zeros(4), np.zeros(4)
    for name, illum, N in pc.RUNS:
        ref, rev = pc.reference(name, illum, N), pc.reference(name, illum, N, True)
        v, info = _device(eng, name, illum, N)
        gap_dev = np.maximum(gap_dev, _gaps(v, info["gamma"], info["bias"], info["weight"], ref))
        gap_self = np.maximum(gap_self, _gaps(rev["v"], rev["robust"][:, 0], rev["robust"][:, 1], rev["robust"][:, 3], ref))
    print(f"photometric rig law, gaps over {len(pc.RUNS)} runs (v_rig relative L2, gamma, beta, sum w relative): the device against the "
          "reference " + " ".join(f"{g:.3e}" for g in gap_dev) + "; the reference against itself summed in reversed order "
          + " ".join(f"{g:.3e}" for g in gap_self))
    assert np.all(gap_dev <= 10.0 * gap_self), (gap_dev, gap_self)


# ---------------------------------------------------------------------------------------------- bit-identity
@pytest.mark.parametrize("name,cam", [("2cam-24x32-l0", 0), ("3cam-41x54-l1", 1), ("2cam-70x24-l0", 1), ("2cam-scalar", 0)])
def test_one_camera_with_the_identity_is_the_robust_law_bit_for_bit(eng, name, cam):
    cams, H, W, level, _, _, _, inter, _ = pc.CASES[name]
    cur, des, Z, scalar, K, _, _ = pc.fixture(name)
    z1 = None if Z is None else Z[cam:cam + 1]
    for illum, N, smin in ((1, 4, SMIN), (1, 4, 1.0), (0, 4, SMIN), (1, 1, SMIN), (1, 0, SMIN), (0, 0, SMIN)):
        rv, rinfo = eng.photometric_robust_velocity(cur[cam], des[cam], z1, K[cam], level, inter, MU, LAM, scalar, bool(illum), N, smin)
        v, info = eng.photometric_rig_velocity(cur[cam], des[cam], z1, K[cam], np.eye(6)[None], None, level, inter, MU, LAM, scalar,
                                               bool(illum), N, smin)
        assert int(rinfo["status"][0]) == info["status"] and (info["status"] == pr.OK or N > 0)
        assert np.array_equal(_bits(v.cpu().numpy()), _bits(rv.cpu().numpy()[0]))
        for key in ("normal", "gamma", "bias", "sigma", "weight"):
            assert np.array_equal(_bits(info[key]), _bits(rinfo[key])), (key, illum, N)
        assert np.array_equal(_bits(info["rig_normal"][27]), _bits(rinfo["normal"][0, 27]))
        assert _rinfo(info) == [1, int(rinfo["n"][0]), int(rinfo["zero_weight"][0]), N, int(rinfo["holes"][0]), 0, *rinfo["pooled"][0]]
    # and where the robust law fails: a flat goal, the 2 x 2 pivot
    flat = np.full_like(des[cam], 77)
    rv, rinfo = eng.photometric_robust_velocity(flat, flat, z1, K[cam], level, inter, MU, LAM, scalar, True, 4, 1.0)
    v, info = eng.photometric_rig_velocity(flat, flat, z1, K[cam], np.eye(6)[None], None, level, inter, MU, LAM, scalar, True, 4, 1.0)
    assert int(rinfo["status"][0]) == info["status"] == _lib.STATUS_TOO_FEW and info["pivot_failed"] and info["reweightings"] == 0
    assert not v.cpu().numpy().any() and not info["gamma"].any() and not info["weight"].any()
    assert np.array_equal(_bits(info["normal"]), _bits(rinfo["normal"]))


@pytest.mark.parametrize("name", list(pc.CASES))
def test_two_calls_and_both_forms_are_bit_identical(eng, name):
    v1, i1 = _call(eng, name, 1, 4)
    v2, i2 = _call(eng, name, 1, 4)
    vh, ih = _call(eng, name, 1, 4, host=True)
    assert _same(v1, i1, v2, i2), "two calls"
    assert _same(v1, i1, vh, ih), "the host form against the _dev form"


def test_a_dead_camera_leaves_no_trace(eng):
    cams, H, W, level, _, _, _, inter, live = pc.CASES["3cam-dead"]
    cur, des, Z, scalar, K, W6, _ = pc.fixture("3cam-dead")
    keep = [i for i, a in enumerate(live) if a]
    for illum, N in ((1, 4), (0, 1), (1, 0)):
        args = (level, inter, MU, LAM, scalar, bool(illum), N, SMIN)
        v2, i2 = eng.photometric_rig_velocity(cur[keep], des[keep], Z[keep], K[keep], W6[keep], None, *args)
        for junk in (cur, np.random.default_rng(3).integers(0, 256, cur.shape).astype(np.uint8)):
            frames = cur.copy()
            frames[1] = junk[1]
            v3, i3 = eng.photometric_rig_velocity(frames, des, Z, K, W6, live, *args)
            assert np.array_equal(_bits(v3.cpu().numpy()), _bits(v2.cpu().numpy())) and i3["status"] == i2["status"] == pr.OK
            assert _rinfo(i3) == _rinfo(i2) and np.array_equal(_bits(i3["rig_normal"]), _bits(i2["rig_normal"]))
            for key in ("normal", "gamma", "bias", "sigma", "weight"):
                assert np.array_equal(_bits(i3[key][keep]), _bits(i2[key])), key
                assert not np.asarray(i3[key][1]).any(), key


def test_a_camera_without_a_row_adds_nothing(eng):
    cams, H, W, level, _, _, _, inter, _ = pc.CASES["3cam-holes"]
    cur, des, Z, scalar, K, W6, _ = pc.fixture("3cam-holes")
    keep = [0, 2]
    args = (level, inter, MU, LAM, scalar, True, 4, SMIN)
    v2, i2 = eng.photometric_rig_velocity(cur[keep], des[keep], Z[keep], K[keep], W6[keep], None, *args)
    v3, i3 = eng.photometric_rig_velocity(cur, des, Z, K, W6, None, *args)
    assert np.array_equal(_bits(v3.cpu().numpy()), _bits(v2.cpu().numpy())) and i3["status"] == pr.OK
    assert (i3["live"], i3["n"], i3["holes"], i3["zero_weight"]) == (3, i2["n"], i2["holes"] + 22 * 30, i2["zero_weight"])
    none = eng.photometric_rig_velocity(cur, des, np.zeros_like(Z), K, W6, None, *args)[1]
    assert none["status"] == _lib.STATUS_TOO_FEW and _rinfo(none) == [3, 0, 0, 0, 3 * 22 * 30, 0, 24, 32]


def _yardstick(name, illum, N):
    """Ten times the reference's relative distance to itself with the rows reversed and the cameras added in descending order."""
    ref, rev = pc.reference(name, illum, N), pc.reference(name, illum, N, True)
    return max(10.0 * np.linalg.norm(rev["v"] - ref["v"]) / np.linalg.norm(ref["v"]), 1e-15)


@pytest.mark.parametrize("name", ["5cam-24x32-l0", "3cam-41x54-l1"])
def test_the_cameras_permuted(eng, name):
    """At N = 0 each camera's own 45 sums and weights are the same bits at any place, whichever wave takes it; v_rig is the same
    twist to rounding (the cameras are added in another order): within ten times the reference's distance to itself in reversed
    order.  With N = 4 the counts, the status and the twist by the same bar."""
    n = len(pc.CASES[name][0])
    order = [3, 0, 4, 2, 1][:n] if n == 5 else [2, 0, 1]
    for illum in (1, 0):
        v, info = _device(eng, name, illum, 0)
        v2, info2 = _call(eng, name, illum, 0, order=order)
        assert info2["status"] == pr.OK and _rinfo(info2) == _rinfo(info)
        for key in ("normal", "weight"):
            assert np.array_equal(_bits(info2[key]), _bits(info[key][order])), key
        assert np.linalg.norm(v2 - v) <= _yardstick(name, illum, 0) * np.linalg.norm(v)
    v, info = _device(eng, name, 1, 4)
    v2, info2 = _call(eng, name, 1, 4, order=order)
    assert info2["status"] == pr.OK and _rinfo(info2) == _rinfo(info) and np.linalg.norm(v2 - v) <= _yardstick(name, 1, 4) * np.linalg.norm(v)


class _Raw:
    """A case's device buffers and the raw _dev call on them."""

    def __init__(self, eng, name):
        dev = eng.device
        cams, H, W, level, _, _, _, inter, _ = pc.CASES[name]
        cur, des, Z, scalar, K, W6, live = pc.fixture(name)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        self.eng, self.n, self.shape, self.level, self.inter, self.scalar = eng, len(cams), (H, W), level, inter, scalar
        self.cur, self.des, self.Z, self.K, self.W = t(cur), t(des), (None if Z is None else t(Z)), t(K), t(W6)
        self.v = torch.empty(6, dtype=torch.float64, device=dev)
        self.st = torch.empty(1, dtype=torch.int32, device=dev)
        self.robust = torch.empty((self.n, 4), dtype=torch.float64, device=dev)
        self.normal = torch.empty((self.n, 45), dtype=torch.float64, device=dev)
        self.rig_normal = torch.empty(28, dtype=torch.float64, device=dev)
        self.rinfo = torch.empty(8, dtype=torch.int32, device=dev)

    def call(self, level=None, inter=None, illum=1, N=4, smin=SMIN, n=None, H=None, W=None, scale=None, mu=MU, lam=LAM, cur=True,
             robust=True, cVr=True, v=True, st=True):
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        e = self.eng
        return e.lib.vitvs_photometric_rig_velocity_dev(
            e.handle, self.n if n is None else n, p(self.cur) if cur else None, p(self.des), self.shape[0] if H is None else H,
            self.shape[1] if W is None else W, p(self.Z), self.scalar if scale is None else scale, p(self.K), p(self.W) if cVr else None,
            None, self.level if level is None else level, self.inter if inter is None else inter, mu, lam, illum, N, smin,
            p(self.v) if v else None, p(self.st) if st else None, p(self.robust) if robust else None, p(self.normal), p(self.rig_normal),
            p(self.rinfo), C.c_void_p(torch.cuda.current_stream(e.device).cuda_stream))

    def results(self):
        return [t.cpu().numpy().copy() for t in (self.v, self.st, self.robust, self.normal, self.rig_normal, self.rinfo)]


def _equal_results(a, b):
    return all(np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x, y.view(np.uint64) if y.dtype == np.float64 else y)
               for x, y in zip(a, b))


def test_a_captured_graph_replays_the_direct_call(eng):
    op = _Raw(eng, "3cam-41x54-l1")
    assert op.call() == 0, _lib.last_error(eng.handle)          # (the direct call, outside the capture: it may allocate)
    torch.cuda.synchronize()
    want = op.results()
    assert int(want[1][0]) == pr.OK and list(want[5][[0, 3]]) == [3, 4]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert op.call() == 0, _lib.last_error(eng.handle)
    for _ in range(2):
        op.v.fill_(float("nan"))
        op.robust.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert _equal_results(op.results(), want)
    op.cur.copy_(op.cur.flip(0))                                # other frames at the same addresses: the replay reads them
    graph.replay()
    torch.cuda.synchronize()
    replayed = op.results()
    assert op.call() == 0
    torch.cuda.synchronize()
    assert _equal_results(replayed, op.results()) and not _equal_results(replayed, want)


# ---------------------------------------------------------------------------------------------- refusals and neighbours
def test_refusals(eng):
    op = _Raw(eng, "2cam-24x32-l0")
    nan, inf = float("nan"), float("inf")
    assert op.call() == 0
    bad = [dict(n=0), dict(n=-1), dict(n=eng.max_pairs + 1), dict(n=17), dict(level=-1), dict(level=4), dict(inter=-1), dict(inter=2),
           dict(mu=-1e-9), dict(mu=nan), dict(mu=inf), dict(lam=nan), dict(lam=inf), dict(scale=nan), dict(scale=-inf),
           dict(H=11, level=2), dict(W=11, level=2), dict(H=2, level=0), dict(H=4097), dict(W=4097), dict(H=0), dict(W=-5),
           dict(illum=2), dict(illum=-1), dict(N=-1), dict(N=5), dict(smin=0.0), dict(smin=-1.0), dict(smin=nan), dict(smin=inf)]
    for kw in bad:
        assert op.call(**kw) == -2, kw
        assert _lib.last_error(eng.handle), kw
    for kw in (dict(cur=False), dict(robust=False), dict(cVr=False), dict(v=False), dict(st=False)):
        assert op.call(**kw) == -1, kw
    big = np.zeros((1, eng.params.v_max + 1, eng.params.u_max, 3), np.uint8)
    hp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    Kh, Wh, vh, sth, rh = np.array([pc.fixture("2cam-24x32-l0")[4][0]]), np.eye(6)[None].copy(), np.zeros(6), np.zeros(1, np.int32), np.zeros((1, 4))
    rc = eng.lib.vitvs_photometric_rig_velocity(eng.handle, 1, hp(big), hp(big), big.shape[1], big.shape[2], None, 0.6, hp(Kh), hp(Wh), None, 2,
                                                1, MU, LAM, 1, 4, 1.0, hp(vh), hp(sth), hp(rh), None, None, None)
    assert rc == -2 and "v_max" in _lib.last_error(eng.handle)
    rc = eng.lib.vitvs_photometric_rig_velocity(eng.handle, 1, hp(big), hp(big), 24, 32, None, 0.6, hp(Kh), None, None, 0, 1, MU, LAM, 1, 4,
                                                1.0, hp(vh), hp(sth), hp(rh), None, None, None)
    assert rc == -1
    assert op.call() == 0                                        # a refusal leaves the handle usable
    for form in (eng.photometric_rig_velocity, eng.photometric_rig_velocity_host):   # no depth at all
        cur, des, _, _, K, W6, _ = pc.fixture("2cam-24x32-l0")
        v, info = form(cur, des, None, K, W6, None, 0, 1, MU, LAM, -1.0, True, 4, 1.0)
        v = v.cpu().numpy() if torch.is_tensor(v) else v
        assert info["status"] == _lib.STATUS_NO_DEPTH and not v.any() and _rinfo(info) == [2, 0, 0, 0, 0, 0, 24, 32]
        assert not info["normal"].any() and not info["rig_normal"].any()


def test_the_op_and_everything_else_the_handle_holds_leave_each_other_alone(eng):
    """A velocity call, a plain and a robust photometric call, then the rig op in both forms: last_details, the next velocity call
    and the other photometric laws are what a fresh handle's are; and the rig op after all of them is what it was before.  The rig op
    runs in the robust law's blocks: each finds the histograms as it needs them behind the other."""
    cfg, params = eng.cfg, eng.params
    fresh = Engine(cfg, params, precision="fp32", max_pairs=5, max_rows=48).load_state_dict(weights.synthetic_state_dict(cfg, 0))
    try:
        des, cur = synth.frame_pair(64, 20250705)
        des2, cur2 = synth.frame_pair(64, 20250706)
        Z, K = synth.depth_pattern(), params.intrinsics()
        order = torch.randperm(eng.tokens, generator=torch.Generator().manual_seed(3)).to(torch.int32).numpy()
        curs, dess, Zs, _, Ks, _, _ = pc.fixture("3cam-41x54-l1")
        photo_args = (curs, dess, Zs, Ks, 1, 1, MU, LAM)
        rig0 = _call(fresh, "3cam-41x54-l1", 1, 4)                              # the op needs nothing before it
        first = [e.compute_velocity_host(cur, des, Z, K, _lib.SELECT_DENSE) for e in (eng, fresh)]
        assert np.array_equal(_bits(first[0][0]), _bits(first[1][0])) and np.array_equal(first[0][1], first[1][1])
        plain = [e.photometric_velocity(*photo_args) for e in (eng, fresh)]
        robust = [e.photometric_robust_velocity(*photo_args, 0.0, True, 4, SMIN) for e in (eng, fresh)]
        before = eng.last_details(1)
        rig1 = _call(eng, "3cam-41x54-l1", 1, 4)
        _call(eng, "2cam-scalar", 0, 1, host=True)
        _call(eng, "3cam-dead", 1, 4)
        assert _same(*rig0, *rig1)
        after = eng.last_details(1)
        for name in before:
            assert np.array_equal(before[name], after[name], equal_nan=True), name
        plain2 = eng.photometric_velocity(*photo_args)
        robust2 = eng.photometric_robust_velocity(*photo_args, 0.0, True, 4, SMIN)
        for got in (plain[1], plain2):
            assert np.array_equal(_bits(got[0].cpu().numpy()), _bits(plain[0][0].cpu().numpy()))
            assert np.array_equal(_bits(got[1]["normal"]), _bits(plain[0][1]["normal"]))
        for got in (robust[1], robust2):
            assert np.array_equal(_bits(got[0].cpu().numpy()), _bits(robust[0][0].cpu().numpy()))
            for key in ("normal", "gamma", "bias", "sigma", "weight"):
                assert np.array_equal(_bits(got[1][key]), _bits(robust[0][1][key])), key
            assert np.array_equal(got[1]["zero_weight"], robust[0][1]["zero_weight"])
        nxt = [e.compute_velocity_host(cur2, des2, Z, K, _lib.SELECT_ORDER, order, num_pairs=8) for e in (eng, fresh)]
        assert np.array_equal(_bits(nxt[0][0]), _bits(nxt[1][0])) and np.array_equal(nxt[0][1], nxt[1][1])
        d0, d1 = eng.last_details(1), fresh.last_details(1)
        for name in d0:
            assert np.array_equal(d0[name], d1[name], equal_nan=True), name
        assert _same(*rig0, *_call(eng, "3cam-41x54-l1", 1, 4))
    finally:
        fresh.close()
