"""The robust photometric law on the device (vitvs_photometric_robust_velocity[_dev], photometric.hip) against
tests/photometric_robust_ref.py, the law in fp64 numpy (GPU).

Inputs: ONE rendered pair of tests/planar_sim.py's scene on the CPU (640 x 480, synth.texture(128, 11), the goal pose and a start
along test_photometric_robust_host.py's direction and axis, 0.3 cm / 0.4 degrees: a crop of a few dozen pixels is linear no further),
the current frame disturbed as there ("gain+bias", "block", both), then cropped (the principal point moved with it) across a corner
of the block to the smallest shapes that reach every path:
  24 x 32, levels 0 and 1   16-pixel loads, bands of one row          23 x 29, level 0   byte loads, a ragged tail
  48 x 64, level 2          pooled 12 x 16                            70 x 32, level 0   70 bands: past the solve's 64-band chunk
  521 x 16, level 0         bands of two rows and a ragged last band (the 480 rows and the first 41 again)
and 48 x 64 with holes in the depth image, 24 x 32 RGB-only, a batch of three with max_pairs 4.  sigma_min is 0.01 in the cases, below
the smallest scale a histogram bin can give (1.4826 / 32), so that the returned sigma tells the median bin of the last re-weighting;
one test runs the default 1.0.

Asserted:
  * both options off: v, status, p_info[:6] and normal45[:28] are the plain entry point's bit for bit;
  * N = 0 with illumination: n, holes, status exactly; each of the 45 sums within (n + 16) 2^-53 sum |term| of the reference's (as
    test_gpu_photometric_op.py derives it: the terms are formed by the reference's operations, the sums differ in order); v, gamma
    and beta within 1e-9 of the reference's solve of the DEVICE's own sums;
  * N = 1 .. 4: the median bin of the last re-weighting (every pass, over the four calls) equals the reference's where the
    reference's half count lies at least 3 rows inside its bin (at least three quarters of the cases, asserted), else within one
    bin; the rows of weight 0 differ by at most the reference's rows with |t - 1| < 1e-9; and over all cases v, gamma, beta and
    sum w are within ten times the reference's distance to itself with every pass summed in reversed row order (both printed);
  * bit-identity of two calls, a pair alone and at each place of a batch, both forms, frames at odd addresses, a captured graph;
  * every refusal; the plain law's and the velocity path's state untouched by a robust call, and the reverse.

Measured (MI355X, profiles/photometric_robust.txt), the largest over the 34 runs: the device against the reference 1.5e-10 (v), 1.0e-12
(gamma), 1.6e-10 (beta), 7.2e-14 (sum w); the reference against itself in reversed row order 1.7e-10, 7.4e-13, 8.8e-11, 6.9e-14.  The
crops hold two or three texels of the scene: (gamma, beta) and the twist are badly conditioned, for both sides alike."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib, config, synth, weights
from vitvs_amd.engine import Engine
import law_support as ls
import photometric_ref as pr
import photometric_robust_ref as rr
from planar_sim import PlanarScene, rodrigues

pytestmark = pytest.mark.gpu

MU, LAM, SMIN = 0.01, 0.5, 0.01
U = 2.0 ** -53
PARAMS = config.ServoParams(dino_input_size=224, use_feature_binning=False)


def gain_bias(rgb, gain=1.15, bias=8.0):
    return np.clip(np.round(gain * rgb.astype(np.float64) + bias), 0, 255).astype(np.uint8)


def block(rgb):
    out = rgb.copy()
    out[120:240, 160:320] = np.kron(np.random.default_rng(5).integers(0, 256, (6, 8, 3)), np.ones((20, 20, 1))).astype(np.uint8)
    return out


DISTURB = {"none": lambda rgb: rgb, "gain+bias": gain_bias, "block": block, "both": lambda rgb: block(gain_bias(rgb))}


START_CM, START_DEG = 0.3, 0.4     # the host test's start direction and axis at a fifth of its size: inside the crops' linear range


@functools.lru_cache(maxsize=None)
def _scene_pair():
    """(current frame, goal frame, goal depth) at 640 x 480, rendered on the CPU."""
    sc = PlanarScene(synth.texture(128, 11), 1.6 / 128, PARAMS, plane_z=0.61, device="cpu")
    goal_rgb, goal_depth = sc.render(np.eye(3), np.zeros(3))
    axis, direction = np.array([0.3, -0.4, 0.85]), np.array([0.6, -0.5, 0.6])
    rgb, _ = sc.render(rodrigues(axis / np.linalg.norm(axis) * np.deg2rad(START_DEG)),
                       direction / np.linalg.norm(direction) * START_CM / 100)
    return rgb, goal_rgb, goal_depth


# name: (H, W, level, disturbance, the crop's first row and column, depth: "z" / "holes" / "scalar", interaction).  The crops with
# the block lie across one of its edges (3 .. 10 % of the crop); the origins were chosen on the CPU, by a search over a grid of
# them, for a reference whose half count lies at least 3 rows inside its median bin in every re-weighting (margin_m).
CASES = {
    "24x32-l0": (24, 32, 0, "both", 236, 148, "z", 1),
    "24x32-l1": (24, 32, 1, "gain+bias", 359, 484, "z", 1),
    "23x29-l0": (23, 29, 0, "block", 99, 308, "z", 0),
    "48x64-l2": (48, 64, 2, "both", 218, 104, "z", 1),
    "70x32-l0": (70, 32, 0, "gain+bias", 322, 484, "z", 1),
    "521x16-l0": (521, 16, 0, "both", 0, 149, "z", 1),
    "48x64-l2-holes": (48, 64, 2, "block", 181, 98, "holes", 1),
    "24x32-l0-rgb": (24, 32, 0, "gain+bias", 100, 166, "scalar", 0),
}
# the runs of N = 1 .. 4: every case with illumination, and without it where no exposure change is planted
RUNS = [(name, 1) for name in CASES] + [(name, 0) for name, c in CASES.items() if c[3] == "block"]
REJECTING = ("23x29-l0", "48x64-l2", "521x16-l0", "48x64-l2-holes")      # cases whose reference gives rows the weight 0


@functools.lru_cache(maxsize=None)
def _fixture(name):
    """(cur, des, Z or None, depth_scale, K) of a case."""
    H, W, level, disturb, y0, x0, depth, inter = CASES[name]
    rgb, goal, gdepth = _scene_pair()

    def cut(img):
        img = img[y0:, x0:]
        if img.shape[0] < H:                                     # 521 rows: the image and its first rows again
            img = np.concatenate([img, img[:H - img.shape[0]]])
        return np.ascontiguousarray(img[:H, :W])
    fx, fy, cx, cy = PARAMS.intrinsics()
    K = (fx, fy, cx - x0, cy - y0)
    cur, des, Z = cut(DISTURB[disturb](rgb)), cut(goal), cut(gdepth)
    if depth == "holes":
        Z = Z.copy()
        Z[8:20, 24:36] = 0                                       # nine pooled pixels without a sample
        Z[30, ::3] = 0                                           # and blocks that miss some
    return cur, des, (None if depth == "scalar" else Z), (0.61 if depth == "scalar" else 0.0), K


@functools.lru_cache(maxsize=None)
def _reference(name, illum, N, reverse=False, smin=SMIN):
    H, W, level, _, _, _, _, inter = CASES[name]
    cur, des, Z, scalar, K = _fixture(name)
    return rr.velocity(cur, des, Z, scalar, K, level, inter, MU, LAM, illum, N, smin, reverse=reverse)


@pytest.fixture(scope="module")
def eng():
    cfg = ls.tiny_cfg(64)
    params = config.ServoParams(dino_input_size=64, use_feature_binning=False)
    e = Engine(cfg, params, precision="fp32", max_pairs=4, max_rows=48).load_state_dict(weights.synthetic_state_dict(cfg, 0))
    yield e
    e.close()


_DEVICE = {}


def _device(eng, name, illum, N, smin=SMIN):
    key = (name, illum, N, smin)
    if key not in _DEVICE:
        H, W, level, _, _, _, _, inter = CASES[name]
        cur, des, Z, scalar, K = _fixture(name)
        v, info = eng.photometric_robust_velocity(cur, des, Z, K, level, inter, MU, LAM, scalar, bool(illum), N, smin)
        _DEVICE[key] = (v.cpu().numpy()[0], info)
    return _DEVICE[key]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _pinfo(info, b=0):
    return [int(info["n"][b]), int(info["pooled"][b, 0]), int(info["pooled"][b, 1]), int(info["bands"][b]), int(info["holes"][b]),
            int(info["pivot_failed"][b]), int(info["zero_weight"][b]), int(info["reweightings"][b])]


def _robust4(info, b=0):
    return np.array([info["gamma"][b], info["bias"][b], info["sigma"][b], info["weight"][b]])


def _same(v1, i1, v2, i2, b1=slice(None), b2=slice(None)):
    keys = ("normal", "gamma", "bias", "sigma", "weight")
    return (np.array_equal(_bits(v1[b1]), _bits(v2[b2])) and all(np.array_equal(_bits(i1[k][b1]), _bits(i2[k][b2])) for k in keys)
            and all(np.array_equal(i1[k][b1], i2[k][b2]) for k in ("status", "n", "holes", "zero_weight", "reweightings")))


def test_the_cases_reach_the_paths_they_name():
    plans = {name: pr.plan(c[0], c[1], c[2]) for name, c in CASES.items()}
    assert plans["24x32-l0"][2:4] == (1, 24) and plans["70x32-l0"][3] == 70 > 64
    assert plans["521x16-l0"][2:4] == (2, 261) and 521 % 2 == 1
    assert plans["48x64-l2"][:2] == (12, 16) and plans["24x32-l1"][:2] == (12, 16)
    ref = _reference("48x64-l2-holes", 1, 0)
    assert ref["info"][4] == 9 and ref["info"][0] == 140 - 9
    margins = [_reference(name, illum, 4)["margin_m"] for name, illum in RUNS]
    print("the reference's half count lies this many rows inside its median bin (the smallest over the four re-weightings): "
          + ", ".join(f"{n}/{i} {m}" for (n, i), m in zip(RUNS, margins)))
    assert sum(m >= 3 for m in margins) * 4 >= 3 * len(margins)
    for name, illum in RUNS:
        assert _reference(name, illum, 4)["status"] == pr.OK, name
    for name in REJECTING:
        assert _reference(name, 1, 4)["info"][6] > 0, name


@pytest.mark.parametrize("name", list(CASES))
def test_both_options_off_is_the_plain_law_bit_for_bit(eng, name):
    H, W, level, _, _, _, _, inter = CASES[name]
    cur, des, Z, scalar, K = _fixture(name)
    pv, pinfo = eng.photometric_velocity(cur, des, Z, K, level, inter, MU, LAM, scalar)
    v, info = eng.photometric_robust_velocity(cur, des, Z, K, level, inter, MU, LAM, scalar, False, 0, 1.0)
    assert int(pinfo["status"][0]) == _lib.STATUS_OK
    assert np.array_equal(_bits(v.cpu().numpy()), _bits(pv.cpu().numpy()))
    assert np.array_equal(_bits(info["normal"][:, :28]), _bits(pinfo["normal"]))
    assert np.array_equal(info["status"], pinfo["status"])
    for key in ("n", "pooled", "bands", "holes", "pivot_failed"):
        assert np.array_equal(info[key], pinfo[key]), key
    assert _pinfo(info)[6:] == [0, 0] and np.array_equal(_robust4(info), [0.0, 0.0, 0.0, float(info["n"][0])])


def _check_sums(v, info, ref, what, illum, b=0):
    n = int(ref["info"][0])
    assert int(info["status"][b]) == ref["status"] == pr.OK, what
    assert _pinfo(info, b)[:6] == list(ref["info"][:6]), (what, _pinfo(info, b), list(ref["info"]))
    err = np.abs(info["normal"][b] - ref["normal"])
    bound = (n + 16) * U * ref["abs"]
    worst = float(np.max(np.where(bound > 0, err / np.maximum(bound, 1e-300), 0.0)))
    print(f"{what}: n {n}, largest |sum - reference| / ((n + 16) 2^-53 sum |term|) over the 45 sums: {worst:.3f}")
    assert np.all(err <= bound), (what, [rr.NAMES[i] for i in np.nonzero(err > bound)[0]])
    own_v, _, own_gamma, own_beta, solved = rr.solve45(info["normal"][b], MU, LAM, illum)
    assert solved
    rel = float(np.linalg.norm(v - own_v) / max(np.linalg.norm(own_v), 1e-300))
    got = _robust4(info, b)
    print(f"{what}: v against the solve of its own sums {rel:.2e}; gamma {got[0]:.6f} (own {own_gamma:.6f}), beta {got[1]:.5f} "
          f"(own {own_beta:.5f}); against the reference's v {np.linalg.norm(v - ref['v']) / np.linalg.norm(ref['v']):.2e}")
    assert rel <= 1e-9, what
    assert abs(got[0] - own_gamma) <= 1e-9 * max(1.0, abs(own_gamma)) and abs(got[1] - own_beta) <= 1e-9 * max(1.0, abs(own_beta)), what


@pytest.mark.parametrize("name", list(CASES))
def test_one_solve_with_illumination_against_the_reference(eng, name):
    ref = _reference(name, 1, 0)
    v, info = _device(eng, name, 1, 0)
    _check_sums(v, info, ref, name, 1)
    assert _pinfo(info)[6:] == [0, 0] and info["sigma"][0] == 0.0
    assert info["weight"][0] == float(ref["info"][0])


def _bin_of(sigma):
    return int(round(sigma / rr.MAD_SCALE * rr.BIN_SCALE - 0.5))


def _gaps(v, info, ref):
    got = _robust4(info)
    return np.array([np.linalg.norm(v - ref["v"]) / max(np.linalg.norm(ref["v"]), 1e-300), abs(got[0] - ref["robust"][0]),
                     abs(got[1] - ref["robust"][1]), abs(got[3] - ref["robust"][3]) / ref["robust"][3]])


@pytest.mark.parametrize("name,illum", RUNS, ids=lambda x: str(x))
def test_reweighted_passes_against_the_reference(eng, name, illum):
    for N in (1, 2, 3, 4):
        ref = _reference(name, illum, N)
        v, info = _device(eng, name, illum, N)
        assert ref["status"] == pr.OK and int(info["status"][0]) == pr.OK, (name, N)
        assert _pinfo(info)[:6] == list(ref["info"][:6]) and _pinfo(info)[7] == N
        last = ref["passes"][-1]
        assert last["sigma"] > SMIN and _bin_of(last["sigma"]) == last["bin"]
        m, slack = _bin_of(float(info["sigma"][0])), (0 if ref["margin_m"] >= 3 else 1)
        zeros = _pinfo(info)[6]
        print(f"{name} illumination {illum} N {N}: median bin {m} (reference {last['bin']}, margin {ref['margin_m']} rows), rows of weight 0 "
              f"{zeros} (reference {ref['info'][6]}, {ref['near_t']} within 1e-9 of t = 1), gamma {info['gain'][0] - 1:.5f} beta "
              f"{info['bias'][0]:.4f}")
        assert abs(m - last["bin"]) <= slack, (name, N)
        assert abs(zeros - int(ref["info"][6])) <= ref["near_t"], (name, N)
        if not illum:
            assert info["gain"][0] == 1.0 and info["bias"][0] == 0.0


def test_gaps_over_all_cases(eng):
    """v (relative L2), gamma, beta (absolute) and sum w (relative) of the device against the reference, the largest over every case
    and N = 1 .. 4, against the reference's distance to itself with every pass summed in reversed row order: at most ten times."""
    gap_dev, gap_self = np.zeros(4), np.zeros(4)
    runs = [(name, N, SMIN) for name in CASES for N in (1, 2, 3, 4)] + [(name, 4, 1.0) for name in FLOORED]
    for name, N, smin in runs:
        ref, rev = _reference(name, 1, N, smin=smin), _reference(name, 1, N, True, smin)
        v, info = _device(eng, name, 1, N, smin)
        gap_dev = np.maximum(gap_dev, _gaps(v, info, ref))
        rev_info = dict(gamma=[rev["robust"][0]], bias=[rev["robust"][1]], sigma=[rev["robust"][2]], weight=[rev["robust"][3]])
        gap_self = np.maximum(gap_self, _gaps(rev["v"], rev_info, ref))
    print(f"robust photometric law, gaps over {len(runs)} runs ({len(CASES)} cases x N = 1 .. 4, {len(FLOORED)} at sigma_min 1) (v relative "
          f"L2, gamma, beta, sum w relative): the device against the reference " + " ".join(f"{g:.3e}" for g in gap_dev) + "; the reference against itself summed in reversed row "
          "order " + " ".join(f"{g:.3e}" for g in gap_self))
    assert np.all(gap_dev <= 10.0 * gap_self), (gap_dev, gap_self)


FLOORED = ("24x32-l1", "48x64-l2")


def test_the_default_sigma_min_floors_the_scale(eng):
    for name in FLOORED:
        ref = _reference(name, 1, 4, smin=1.0)
        v, info = _device(eng, name, 1, 4, smin=1.0)
        assert ref["status"] == pr.OK and int(info["status"][0]) == pr.OK
        assert info["sigma"][0] == ref["robust"][2]
        assert abs(_pinfo(info)[6] - int(ref["info"][6])) <= ref["near_t"]


# ---------------------------------------------------------------------------------------------- bit-identity
def _pairs_of_three():
    names = ("48x64-l2", "48x64-l2-holes", "48x64-l2")
    fx = [_fixture(n) for n in names]
    curs, dess, Zs = (np.stack([f[i] for f in fx]) for i in range(3))
    curs[2], dess[2] = dess[2][::-1, ::-1].copy(), curs[2][::-1, ::-1].copy()
    Ks = np.array([fx[0][4], fx[1][4], (55.0, 65.0, 30.0, 25.0)])
    return curs, dess, Zs, Ks


@pytest.mark.parametrize("illum,N", [(1, 4), (0, 2), (1, 0)])
def test_a_batch_of_three_pairs(eng, illum, N):
    curs, dess, Zs, Ks = _pairs_of_three()
    args = (2, 1, MU, LAM, 0.0, bool(illum), N, SMIN)
    v, info = eng.photometric_robust_velocity(curs, dess, Zs, Ks, *args)
    v = v.cpu().numpy()
    for b in range(3):
        ref = rr.velocity(curs[b], dess[b], Zs[b], 0.0, Ks[b], 2, 1, MU, LAM, illum, N, SMIN)
        assert int(info["status"][b]) == ref["status"] == pr.OK and _pinfo(info, b)[:6] == list(ref["info"][:6])
        assert abs(_pinfo(info, b)[6] - int(ref["info"][6])) <= ref["near_t"] and _pinfo(info, b)[7] == N
        alone_v, alone = eng.photometric_robust_velocity(curs[b], dess[b], Zs[b:b + 1], Ks[b], *args)
        assert _same(v, info, alone_v.cpu().numpy(), alone, slice(b, b + 1)), f"pair {b} alone is not pair {b} of the batch"
    back = [2, 0, 1]
    v2, info2 = eng.photometric_robust_velocity(curs[back], dess[back], Zs[back], Ks[back], *args)
    v2 = v2.cpu().numpy()
    for place, b in enumerate(back):
        assert _same(v, info, v2, info2, slice(b, b + 1), slice(place, place + 1)), f"pair {b} at place {place}"


@pytest.mark.parametrize("name", ["24x32-l0", "23x29-l0", "48x64-l2-holes", "521x16-l0", "24x32-l0-rgb"])
def test_two_calls_and_both_forms_are_bit_identical(eng, name):
    H, W, level, _, _, _, _, inter = CASES[name]
    cur, des, Z, scalar, K = _fixture(name)
    args = (cur, des, Z, K, level, inter, MU, LAM, scalar, True, 4, SMIN)
    v1, i1 = eng.photometric_robust_velocity(*args)
    v2, i2 = eng.photometric_robust_velocity(*args)
    vh, ih = eng.photometric_robust_velocity_host(*args)
    assert _same(v1.cpu().numpy(), i1, v2.cpu().numpy(), i2), "two calls"
    assert _same(v1.cpu().numpy(), i1, vh, ih), "the host form against the _dev form"
    assert np.array_equal(i1["pooled"], ih["pooled"]) and np.array_equal(i1["bands"], ih["bands"])


class _Raw:
    """One pair's device buffers and the raw _dev call on them."""

    def __init__(self, eng, cur, des, Z, K, pad=0, zpad=0):
        dev = eng.device

        def padded(a, k):
            host = np.zeros(a.size + 16, a.dtype)
            host[k:k + a.size] = a.reshape(-1)
            return torch.from_numpy(host).to(dev)
        self.eng, self.pad, self.zpad, self.shape = eng, pad, zpad, cur.shape[:2]
        self.cur, self.des, self.Z = padded(cur, pad), padded(des, pad), padded(Z, zpad)
        self.K = torch.tensor([K], dtype=torch.float64, device=dev)
        self.v = torch.empty((1, 6), dtype=torch.float64, device=dev)
        self.st = torch.empty(1, dtype=torch.int32, device=dev)
        self.robust = torch.empty((1, 4), dtype=torch.float64, device=dev)
        self.normal = torch.empty((1, 45), dtype=torch.float64, device=dev)
        self.pinfo = torch.empty((1, 8), dtype=torch.int32, device=dev)

    def call(self, level=2, inter=1, illum=1, N=4, smin=SMIN, n=1, H=None, W=None, scale=0.0, mu=MU, lam=LAM, cur=True, robust=True):
        p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
        e = self.eng
        return e.lib.vitvs_photometric_robust_velocity_dev(
            e.handle, n, p(self.cur, self.pad) if cur else None, p(self.des, self.pad), self.shape[0] if H is None else H,
            self.shape[1] if W is None else W, p(self.Z, 2 * self.zpad), scale, p(self.K), level, inter, mu, lam, illum, N, smin, p(self.v),
            p(self.st), p(self.robust) if robust else None, p(self.normal), p(self.pinfo),
            C.c_void_p(torch.cuda.current_stream(e.device).cuda_stream))

    def results(self):
        return [t.cpu().numpy().copy() for t in (self.v, self.st, self.robust, self.normal, self.pinfo)]


def _equal_results(a, b):
    return all(np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x, y.view(np.uint64) if y.dtype == np.float64 else y)
               for x, y in zip(a, b))


def test_frames_at_odd_addresses_take_the_narrow_loads_to_the_same_bits(eng):
    cur, des, Z, _, K = _fixture("48x64-l2")
    base = _Raw(eng, cur, des, Z, K)
    assert base.call() == 0, _lib.last_error(eng.handle)
    want = base.results()
    assert int(want[1][0]) == pr.OK and want[4][0, 7] == 4
    for pad, zpad in ((1, 1), (4, 2), (5, 0)):
        other = _Raw(eng, cur, des, Z, K, pad, zpad)
        assert other.call() == 0, _lib.last_error(eng.handle)
        assert _equal_results(other.results(), want), pad


def test_a_captured_graph_replays_the_direct_call(eng):
    cur, des, Z, _, K = _fixture("48x64-l2")
    op = _Raw(eng, cur, des, Z, K)
    assert op.call() == 0, _lib.last_error(eng.handle)          # (the direct call, outside the capture: it may allocate)
    torch.cuda.synchronize()
    want = op.results()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert op.call() == 0, _lib.last_error(eng.handle)
    for _ in range(2):
        op.v.fill_(float("nan"))
        op.robust.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert _equal_results(op.results(), want)
    cur2, des2, Z2, _, _ = _fixture("48x64-l2-holes")               # other frames at the same addresses: the replay reads them
    op.cur[:cur2.size].copy_(torch.from_numpy(cur2.reshape(-1)))
    op.des[:des2.size].copy_(torch.from_numpy(des2.reshape(-1)))
    op.Z[:Z2.size].copy_(torch.from_numpy(Z2.reshape(-1)))
    graph.replay()
    torch.cuda.synchronize()
    replayed = op.results()
    assert op.call() == 0
    torch.cuda.synchronize()
    assert _equal_results(replayed, op.results()) and not _equal_results(replayed, want)


# ---------------------------------------------------------------------------------------------- statuses and refusals
def test_statuses(eng):
    cur, des, Z, _, K = _fixture("48x64-l2")
    flat = np.full_like(des, 77)
    v, info = eng.photometric_robust_velocity(flat, flat, Z, K, 2, 1, MU, LAM, 0.0, True, 4, 1.0)      # D constant: the 2 x 2 pivot
    assert int(info["status"][0]) == _lib.STATUS_TOO_FEW and np.array_equal(v.cpu().numpy(), np.zeros((1, 6)))
    assert _pinfo(info) == [140, 12, 16, 12, 0, 1, 0, 0] and np.array_equal(_robust4(info), np.zeros(4))
    ref = rr.velocity(flat, flat, Z, 0.0, K, 2, 1, MU, LAM, 1, 4, 1.0)
    assert ref["status"] == pr.TOO_FEW and list(ref["info"]) == [140, 12, 16, 12, 0, 1, 0, 0]
    # a textured goal, no motion: v = 0 exactly, gamma = beta = 0, every weight 1
    v, info = eng.photometric_robust_velocity(des, des, Z, K, 2, 1, MU, LAM, 0.0, True, 4, 1.0)
    assert int(info["status"][0]) == _lib.STATUS_OK and np.array_equal(v.cpu().numpy(), np.zeros((1, 6)))
    assert info["gain"][0] == 1.0 and info["bias"][0] == 0.0 and info["sigma"][0] == 1.0 and info["weight"][0] == 140.0
    assert _pinfo(info) == [140, 12, 16, 12, 0, 0, 0, 4]
    # every depth a hole: no row; no depth at all
    v, info = eng.photometric_robust_velocity(cur, des, np.zeros_like(Z), K, 2, 1, MU, LAM, 0.0, True, 4, 1.0)
    assert int(info["status"][0]) == _lib.STATUS_TOO_FEW and _pinfo(info) == [0, 12, 16, 12, 140, 0, 0, 0]
    for form in (eng.photometric_robust_velocity, eng.photometric_robust_velocity_host):
        v, info = form(cur, des, None, K, 2, 1, MU, LAM, -1.0, True, 4, 1.0)
        v = v.cpu().numpy() if torch.is_tensor(v) else v
        assert int(info["status"][0]) == _lib.STATUS_NO_DEPTH and np.array_equal(v, np.zeros((1, 6)))
        assert _pinfo(info) == [0, 12, 16, 12, 0, 0, 0, 0] and np.array_equal(info["normal"], np.zeros((1, 45)))
    # fewer than six rows keep a weight (photometric_robust_ref.few_weights_pair): the first re-weighting ends the call
    fc, fd, fK = rr.few_weights_pair()
    ref = rr.velocity(fc, fd, None, 0.6, fK, 0, 1, MU, LAM, 0, 4, 1e-3)
    v, info = eng.photometric_robust_velocity(fc, fd, None, fK, 0, 1, MU, LAM, 0.6, False, 4, 1e-3)
    assert ref["status"] == pr.TOO_FEW and int(info["status"][0]) == _lib.STATUS_TOO_FEW
    assert _pinfo(info) == list(ref["info"]) == [10, 4, 7, 4, 0, 0, 5, 1]
    assert np.array_equal(v.cpu().numpy(), np.zeros((1, 6))) and np.array_equal(_robust4(info), np.zeros(4))
    # and the next call on the handle finds its histogram empty
    again = eng.photometric_robust_velocity(des, des, Z, K, 2, 1, MU, LAM, 0.0, True, 4, 1.0)[1]
    assert int(again["status"][0]) == _lib.STATUS_OK and again["sigma"][0] == 1.0 and _pinfo(again)[6:] == [0, 4]


def test_refusals(eng):
    cur, des, Z, _, K = _fixture("48x64-l2")
    op = _Raw(eng, cur, des, Z, K)
    nan, inf = float("nan"), float("inf")
    assert op.call() == 0
    bad = [dict(n=0), dict(n=-1), dict(n=eng.max_pairs + 1), dict(level=-1), dict(level=4), dict(inter=-1), dict(inter=2),
           dict(mu=-1e-9), dict(mu=nan), dict(mu=inf), dict(lam=nan), dict(lam=inf), dict(scale=nan), dict(scale=-inf),
           dict(H=11, level=2), dict(W=11, level=2), dict(H=2, level=0), dict(H=4097), dict(W=4097), dict(H=0), dict(W=-5),
           dict(illum=2), dict(illum=-1), dict(N=-1), dict(N=5), dict(smin=0.0), dict(smin=-1.0), dict(smin=nan), dict(smin=inf)]
    for kw in bad:
        assert op.call(**kw) == -2, kw
        assert _lib.last_error(eng.handle), kw
    assert op.call(cur=False) == -1 and op.call(robust=False) == -1
    big = np.zeros((1, eng.params.v_max + 1, eng.params.u_max, 3), np.uint8)
    hp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    Kh, vh, sth, rh = np.array([K]), np.zeros((1, 6)), np.zeros(1, np.int32), np.zeros((1, 4))
    rc = eng.lib.vitvs_photometric_robust_velocity(eng.handle, 1, hp(big), hp(big), big.shape[1], big.shape[2], None, 0.6, hp(Kh), 2, 1, MU,
                                                   LAM, 1, 4, 1.0, hp(vh), hp(sth), hp(rh), None, None)
    assert rc == -2 and "v_max" in _lib.last_error(eng.handle)
    assert op.call() == 0                                        # a refusal leaves the handle usable


def test_the_op_and_everything_else_the_handle_holds_leave_each_other_alone(eng):
    """A velocity call and a plain photometric call, then the robust op in both forms: last_details, vitvs_reselect, the next
    velocity call and the plain law are what a fresh handle's are; and the robust op after all of them is what it was before."""
    cfg, params = eng.cfg, eng.params
    fresh = Engine(cfg, params, precision="fp32", max_pairs=4, max_rows=48).load_state_dict(weights.synthetic_state_dict(cfg, 0))
    try:
        des, cur = synth.frame_pair(64, 20250705)
        des2, cur2 = synth.frame_pair(64, 20250706)
        Z, K = synth.depth_pattern(), params.intrinsics()
        order = torch.randperm(eng.tokens, generator=torch.Generator().manual_seed(3)).to(torch.int32).numpy()
        curs, dess, Zs, Ks = _pairs_of_three()
        robust_args = (curs, dess, Zs, Ks, 2, 1, MU, LAM, 0.0, True, 4, SMIN)
        rv0, rinfo0 = fresh.photometric_robust_velocity(*robust_args)          # the op needs nothing before it
        first = [e.compute_velocity_host(cur, des, Z, K, _lib.SELECT_DENSE) for e in (eng, fresh)]
        assert np.array_equal(_bits(first[0][0]), _bits(first[1][0])) and np.array_equal(first[0][1], first[1][1])
        plain = [e.photometric_velocity(curs, dess, Zs, Ks, 2, 1, MU, LAM) for e in (eng, fresh)]
        before = eng.last_details(1)
        rv1, rinfo1 = eng.photometric_robust_velocity(*robust_args)
        eng.photometric_robust_velocity_host(curs[:2], dess[:2], Zs[:2], Ks[:2], 1, 0, MU, LAM, 0.0, False, 3, 1.0)
        assert _same(rv0.cpu().numpy(), rinfo0, rv1.cpu().numpy(), rinfo1)
        after = eng.last_details(1)
        for name in before:
            assert np.array_equal(before[name], after[name], equal_nan=True), name
        again = [e.reselect_host(_lib.SELECT_ORDER, order[None], num_pairs=8) for e in (eng, fresh)]
        assert np.array_equal(_bits(again[0][0]), _bits(again[1][0])) and np.array_equal(again[0][1], again[1][1])
        plain2 = eng.photometric_velocity(curs, dess, Zs, Ks, 2, 1, MU, LAM)
        for pv, pi in (plain[1], plain2):
            assert np.array_equal(_bits(pv.cpu().numpy()), _bits(plain[0][0].cpu().numpy()))
            assert np.array_equal(_bits(pi["normal"]), _bits(plain[0][1]["normal"]))
        nxt = [e.compute_velocity_host(cur2, des2, Z, K, _lib.SELECT_ORDER, order, num_pairs=8) for e in (eng, fresh)]
        assert np.array_equal(_bits(nxt[0][0]), _bits(nxt[1][0])) and np.array_equal(nxt[0][1], nxt[1][1])
        d0, d1 = eng.last_details(1), fresh.last_details(1)
        for name in d0:
            assert np.array_equal(d0[name], d1[name], equal_nan=True), name
        rv2, rinfo2 = eng.photometric_robust_velocity(*robust_args)
        assert _same(rv0.cpu().numpy(), rinfo0, rv2.cpu().numpy(), rinfo2)
    finally:
        fresh.close()
