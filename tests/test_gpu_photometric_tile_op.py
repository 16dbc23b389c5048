"""The tile photometric law on the device (vitvs_photometric_tile_velocity[_dev], photometric.hip) against
tests/photometric_tile_ref.py, the law in fp64 numpy (GPU).

Inputs: tests/photometric_tile_cases.py: small crops of the robust op test's scene pair, half of each shaded by 0.6 across a slanted
edge through the crop.  The cases are the smallest at which the new code can go wrong:
  24 x 32, level 0, 2 x 2 and 3 x 5   tile edges that do not divide the sides       23 x 29, level 0, 4 x 4   odd sides, byte loads
  48 x 64, level 2, 4 x 4 with holes, and 8 x 8 (the most tiles)                     70 x 32, level 0, 8 x 2   9 bands per tile row: the
  1042 x 16, level 1, 3 x 1   pooled 521 rows in two-row bands, the tile rows beginning where bands begin     solve's second group of 8
  1042 x 16, level 1, 4 x 1   the same with the tile rows beginning at 131, 261, 391: three bands lie across a tile-row edge, their
                              rows go to the band's two slots and the solve reads the second slot
  24 x 32 RGB-only with a scalar depth, 48 x 64 with a flat patch (a dead tile), 24 x 8 with gx = pooled w (border-only dead tiles)
sigma_min is 0.01 in the cases, below the smallest scale a histogram bin can give, so that the returned sigma tells the median bin.

Asserted per case, against the reference:
  * N = 0: n, p_info, status, live and dead tiles exactly; every per-tile sum within (n_k + 16) 2^-53 sum |term| (the terms are
    formed by the reference's operations, the sums differ in order); v, gamma_k, beta_k within 1e-9 of the reference's solve of the
    DEVICE's own sums;
  * N = 1 .. 4: the median bin equals the reference's where its half count lies at least 3 rows inside its bin, else within one
    bin; the rows of weight 0 differ by at most the reference's rows with |t - 1| < 1e-9; live and dead tiles exactly; and over all
    N of a case v, gamma_k, beta_k and sum w are within ten times the reference's distance to itself with every tile's rows reversed
    and the tiles taken in descending order, case by case (both printed);
  * 1 x 1 tiles against the robust call on the device within that same yardstick;
  * bit-identity of two calls, a pair alone and at each place of a batch, both forms, frames at odd addresses, a captured graph;
  * every refusal; the other laws' outputs and the handle's state untouched by a tile call, and the reverse.
(test_photometric_tile_host.py asserts, without a device, that every reference status is OK and where the margins lie.)"""
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
import photometric_tile_ref as tr
import photometric_tile_cases as tc

pytestmark = pytest.mark.gpu

MU, LAM, SMIN = tc.MU, tc.LAM, tc.SMIN
U = 2.0 ** -53
CASES = tc.CASES


@pytest.fixture(scope="module")
def eng():
    cfg = ls.tiny_cfg(64)
    params = config.ServoParams(dino_input_size=64, use_feature_binning=False)
    e = Engine(cfg, params, precision="fp32", max_pairs=4, max_rows=48).load_state_dict(weights.synthetic_state_dict(cfg, 0))
    yield e
    e.close()


_DEVICE = {}


def _device(eng, name, N, smin=SMIN):
    key = (name, N, smin)
    if key not in _DEVICE:
        _, _, level, grid, _, _, _, inter, _ = CASES[name]
        cur, des, Z, scalar, K = tc.fixture(name)
        v, info = eng.photometric_tile_velocity(cur, des, Z, K, level, inter, MU, LAM, scalar, grid, N, smin)
        _DEVICE[key] = (v.cpu().numpy()[0], info)
    return _DEVICE[key]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _pinfo(info, b=0):
    return [int(info["n"][b]), int(info["pooled"][b, 0]), int(info["pooled"][b, 1]), int(info["bands"][b]), int(info["holes"][b]),
            int(info["pivot_failed"][b]), int(info["zero_weight"][b]), int(info["reweightings"][b])]


def _tiles4(info, b=0):
    """[T, 4] gamma_k, beta_k, sum w_k, live of pair b."""
    return np.stack([info["tile_gain"][b] - 1.0, info["tile_bias"][b], info["tile_weight"][b], info["tile_live"][b].astype(np.float64)],
                    axis=-1).reshape(-1, 4)


KEYS = ("normal", "tile_gain", "tile_bias", "tile_weight", "sigma", "weight")
INTS = ("status", "n", "holes", "zero_weight", "reweightings", "tile_live", "live_tiles", "dead_tiles")


def _same(v1, i1, v2, i2, b1=slice(None), b2=slice(None)):
    return (np.array_equal(_bits(v1[b1]), _bits(v2[b2])) and all(np.array_equal(_bits(i1[k][b1]), _bits(i2[k][b2])) for k in KEYS)
            and all(np.array_equal(i1[k][b1], i2[k][b2]) for k in INTS))


def _check_tiles(info, ref, what, b=0):
    assert int(info["status"][b]) == ref["status"] == pr.OK, what
    assert (int(info["live_tiles"][b]), int(info["dead_tiles"][b])) == (int(ref["robust"][0]), int(ref["robust"][1])), what
    assert np.array_equal(_tiles4(info, b)[:, 3], ref["tiles"][:, 3]), what


@pytest.mark.parametrize("name", list(CASES))
def test_one_solve_against_the_reference(eng, name):
    ref = tc.reference(name, 0)
    v, info = _device(eng, name, 0)
    _check_tiles(info, ref, name)
    assert _pinfo(info) == list(ref["info"]), (name, _pinfo(info), list(ref["info"]))
    err = np.abs(info["normal"][0] - ref["normal"])
    bound = (ref["tile_n"][:, None] + 16) * U * ref["abs"]
    worst = float(np.max(np.where(bound > 0, err / np.maximum(bound, 1e-300), 0.0)))
    print(f"{name}: n {ref['info'][0]} in tiles of {ref['tile_n'].min()} .. {ref['tile_n'].max()} rows, largest |sum - reference| / "
          f"((n_k + 16) 2^-53 sum |term|) over the tiles' 45 sums: {worst:.3f}")
    assert np.all(err <= bound), (name, np.argwhere(err > bound))
    own_v, _, own_gb, own_live, solved = tr.solve_tiles(info["normal"][0], MU, LAM)
    assert solved and np.array_equal(own_live, ref["tiles"][:, 3] != 0)
    rel = float(np.linalg.norm(v - own_v) / max(np.linalg.norm(own_v), 1e-300))
    got = _tiles4(info)
    gap = np.abs(got[:, :2] - own_gb) / np.maximum(1.0, np.abs(own_gb))
    print(f"{name}: v against the solve of its own sums {rel:.2e}, (gamma_k, beta_k) {gap.max():.2e}; against the reference's v "
          f"{np.linalg.norm(v - ref['v']) / np.linalg.norm(ref['v']):.2e}; live {int(ref['robust'][0])}, dead {int(ref['robust'][1])}")
    assert rel <= 1e-9 and np.all(gap <= 1e-9), name
    assert info["sigma"][0] == 0.0 and np.array_equal(got[:, 2], info["normal"][0][:, 42])
    assert info["weight"][0] == sum(info["normal"][0][k, 42] for k in range(got.shape[0]) if got[k, 3])


def _bin_of(sigma):
    return int(round(sigma / rr.MAD_SCALE * rr.BIN_SCALE - 0.5))


@pytest.mark.parametrize("name", list(CASES))
def test_reweighted_passes_against_the_reference(eng, name):
    for N in (1, 2, 3, 4):
        ref = tc.reference(name, N)
        v, info = _device(eng, name, N)
        _check_tiles(info, ref, (name, N))
        assert _pinfo(info)[:6] == list(ref["info"][:6]) and _pinfo(info)[7] == N
        last = ref["passes"][-1]
        assert last["sigma"] > SMIN and _bin_of(last["sigma"]) == last["bin"]
        m, slack = _bin_of(float(info["sigma"][0])), (0 if ref["margin_m"] >= 3 else 1)
        zeros = _pinfo(info)[6]
        print(f"{name} N {N}: median bin {m} (reference {last['bin']}, margin {ref['margin_m']} rows), rows of weight 0 {zeros} (reference "
              f"{ref['info'][6]}, {ref['near_t']} within 1e-9 of t = 1), live {int(info['live_tiles'][0])} dead {int(info['dead_tiles'][0])}")
        assert abs(m - last["bin"]) <= slack, (name, N)
        assert abs(zeros - int(ref["info"][6])) <= ref["near_t"], (name, N)


def _gaps(v, tiles, weight, ref):
    return np.array([np.linalg.norm(v - ref["v"]) / max(np.linalg.norm(ref["v"]), 1e-300), np.max(np.abs(tiles[:, 0] - ref["tiles"][:, 0])),
                     np.max(np.abs(tiles[:, 1] - ref["tiles"][:, 1])), abs(weight - ref["robust"][3]) / ref["robust"][3]])


@pytest.mark.parametrize("name", list(CASES))
def test_gaps_per_case(eng, name):
    """v (relative L2), gamma_k, beta_k (absolute, the largest over the tiles) and sum w (relative) of the device against the
    reference, the largest over N = 1 .. 4 of the case, against the reference's distance to itself in reversed order over the same
    runs: at most ten times, case by case."""
    gap_dev, gap_self = np.zeros(4), np.zeros(4)
    for N in (1, 2, 3, 4):
        ref, rev = tc.reference(name, N), tc.reference(name, N, True)
        v, info = _device(eng, name, N)
        gap_dev = np.maximum(gap_dev, _gaps(v, _tiles4(info), float(info["weight"][0]), ref))
        gap_self = np.maximum(gap_self, _gaps(rev["v"], rev["tiles"], rev["robust"][3], ref))
    print(f"{name}, gaps over N = 1 .. 4 (v relative L2, gamma_k, beta_k, sum w relative): the device against the reference "
          + " ".join(f"{g:.3e}" for g in gap_dev) + "; the reference against itself in reversed order " + " ".join(f"{g:.3e}" for g in gap_self))
    assert np.all(gap_dev <= 10.0 * gap_self), (gap_dev, gap_self)


ONE_TILE = ("24x32-l0-2x2", "23x29-l0-4x4", "48x64-l2-4x4-holes", "70x32-l0-8x2", "1042x16-l1-3x1", "24x32-l0-rgb-2x2")


def test_one_tile_against_the_robust_call(eng):
    """1 x 1 tiles on the device against vitvs_photometric_robust_velocity_dev with illumination on the same inputs: v (relative
    L2), gamma, beta (absolute) and sum w (relative) within ten times the robust reference's distance to itself in reversed row
    order (the largest over the cases and N = 1 .. 4).  The two kernels sum in different orders: no bit-identity."""
    gap_dev, gap_self = np.zeros(4), np.zeros(4)
    for name in ONE_TILE:
        _, _, level, _, _, _, _, inter, _ = CASES[name]
        cur, des, Z, scalar, K = tc.fixture(name)
        for N in (0, 1, 2, 3, 4):
            rv, rinfo = eng.photometric_robust_velocity(cur, des, Z, K, level, inter, MU, LAM, scalar, True, N, SMIN)
            tv, tinfo = eng.photometric_tile_velocity(cur, des, Z, K, level, inter, MU, LAM, scalar, (1, 1), N, SMIN)
            assert int(rinfo["status"][0]) == int(tinfo["status"][0]) == pr.OK and list(tinfo["live_tiles"]) == [1]
            assert _pinfo(tinfo)[:6] == _pinfo(rinfo)[:6] and _pinfo(tinfo)[7] == N
            rv, tv = rv.cpu().numpy()[0], tv.cpu().numpy()[0]
            gap_dev = np.maximum(gap_dev, [np.linalg.norm(tv - rv) / np.linalg.norm(rv), abs(tinfo["tile_gain"][0, 0, 0] - rinfo["gain"][0]),
                                           abs(tinfo["tile_bias"][0, 0, 0] - rinfo["bias"][0]),
                                           abs(tinfo["weight"][0] - rinfo["weight"][0]) / rinfo["weight"][0]])
            ref = rr.velocity(cur, des, Z, scalar, K, level, inter, MU, LAM, 1, N, SMIN)
            rev = rr.velocity(cur, des, Z, scalar, K, level, inter, MU, LAM, 1, N, SMIN, reverse=True)
            gap_self = np.maximum(gap_self, [np.linalg.norm(rev["v"] - ref["v"]) / np.linalg.norm(ref["v"]),
                                             abs(rev["robust"][0] - ref["robust"][0]), abs(rev["robust"][1] - ref["robust"][1]),
                                             abs(rev["robust"][3] - ref["robust"][3]) / ref["robust"][3]])
    print("1 x 1 tiles against the robust call (v relative L2, gamma, beta, sum w relative): " + " ".join(f"{g:.3e}" for g in gap_dev)
          + "; the robust reference against itself in reversed row order " + " ".join(f"{g:.3e}" for g in gap_self))
    assert np.all(gap_dev <= 10.0 * gap_self), (gap_dev, gap_self)


# ---------------------------------------------------------------------------------------------- bit-identity
def _pairs_of_three():
    names = ("48x64-l2-8x8", "48x64-l2-4x4-holes", "48x64-l2-4x4-flat")
    fx = [tc.fixture(n) for n in names]
    curs, dess, Zs = (np.stack([f[i] for f in fx]) for i in range(3))
    Ks = np.array([fx[0][4], fx[1][4], (55.0, 65.0, 30.0, 25.0)])
    return curs, dess, Zs, Ks


@pytest.mark.parametrize("grid,N", [((4, 4), 4), ((8, 8), 2), ((3, 5), 0)])
def test_a_batch_of_three_pairs(eng, grid, N):
    curs, dess, Zs, Ks = _pairs_of_three()
    args = (2, 1, MU, LAM, 0.0, grid, N, SMIN)
    v, info = eng.photometric_tile_velocity(curs, dess, Zs, Ks, *args)
    v = v.cpu().numpy()
    for b in range(3):
        ref = tr.velocity(curs[b], dess[b], Zs[b], 0.0, Ks[b], 2, 1, MU, LAM, grid[0], grid[1], N, SMIN)
        assert int(info["status"][b]) == ref["status"] and _pinfo(info, b)[:6] == list(ref["info"][:6])
        alone_v, alone = eng.photometric_tile_velocity(curs[b], dess[b], Zs[b:b + 1], Ks[b], *args)
        assert _same(v, info, alone_v.cpu().numpy(), alone, slice(b, b + 1)), f"pair {b} alone is not pair {b} of the batch"
    back = [2, 0, 1]
    v2, info2 = eng.photometric_tile_velocity(curs[back], dess[back], Zs[back], Ks[back], *args)
    v2 = v2.cpu().numpy()
    for place, b in enumerate(back):
        assert _same(v, info, v2, info2, slice(b, b + 1), slice(place, place + 1)), f"pair {b} at place {place}"


@pytest.mark.parametrize("name", ["24x32-l0-3x5", "23x29-l0-4x4", "48x64-l2-4x4-holes", "1042x16-l1-3x1", "1042x16-l1-4x1", "24x32-l0-rgb-2x2",
                                  "24x8-l0-2x8"])
def test_two_calls_and_both_forms_are_bit_identical(eng, name):
    _, _, level, grid, _, _, _, inter, _ = CASES[name]
    cur, des, Z, scalar, K = tc.fixture(name)
    args = (cur, des, Z, K, level, inter, MU, LAM, scalar, grid, 4, SMIN)
    v1, i1 = eng.photometric_tile_velocity(*args)
    v2, i2 = eng.photometric_tile_velocity(*args)
    vh, ih = eng.photometric_tile_velocity_host(*args)
    assert _same(v1.cpu().numpy(), i1, v2.cpu().numpy(), i2), "two calls"
    assert _same(v1.cpu().numpy(), i1, vh, ih), "the host form against the _dev form"
    assert np.array_equal(i1["pooled"], ih["pooled"]) and np.array_equal(i1["bands"], ih["bands"])


class _Raw:
    """One pair's device buffers and the raw _dev call on them."""

    def __init__(self, eng, cur, des, Z, K, pad=0, zpad=0, T=16):
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
        self.tiles = torch.zeros((1, 64, 4), dtype=torch.float64, device=dev)
        self.normal = torch.zeros((1, 64, 45), dtype=torch.float64, device=dev)
        self.pinfo = torch.empty((1, 8), dtype=torch.int32, device=dev)

    def call(self, level=2, inter=1, gy=4, gx=4, N=4, smin=SMIN, n=1, H=None, W=None, scale=0.0, mu=MU, lam=LAM, cur=True, robust=True,
             tiles=True):
        p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
        e = self.eng
        return e.lib.vitvs_photometric_tile_velocity_dev(
            e.handle, n, p(self.cur, self.pad) if cur else None, p(self.des, self.pad), self.shape[0] if H is None else H,
            self.shape[1] if W is None else W, p(self.Z, 2 * self.zpad), scale, p(self.K), level, inter, mu, lam, gy, gx, N, smin, p(self.v),
            p(self.st), p(self.robust) if robust else None, p(self.tiles) if tiles else None, p(self.normal), p(self.pinfo),
            C.c_void_p(torch.cuda.current_stream(e.device).cuda_stream))

    def results(self):
        return [t.cpu().numpy().copy() for t in (self.v, self.st, self.robust, self.tiles, self.normal, self.pinfo)]


def _equal_results(a, b):
    return all(np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x, y.view(np.uint64) if y.dtype == np.float64 else y)
               for x, y in zip(a, b))


def test_frames_at_odd_addresses_take_the_narrow_loads_to_the_same_bits(eng):
    cur, des, Z, _, K = tc.fixture("48x64-l2-4x4-holes")
    base = _Raw(eng, cur, des, Z, K)
    assert base.call() == 0, _lib.last_error(eng.handle)
    want = base.results()
    assert int(want[1][0]) == pr.OK and want[5][0, 7] == 4
    for pad, zpad in ((1, 1), (4, 2), (5, 0)):
        other = _Raw(eng, cur, des, Z, K, pad, zpad)
        assert other.call() == 0, _lib.last_error(eng.handle)
        assert _equal_results(other.results(), want), pad


def test_a_captured_graph_replays_the_direct_call(eng):
    cur, des, Z, _, K = tc.fixture("48x64-l2-8x8")
    op = _Raw(eng, cur, des, Z, K)
    assert op.call() == 0, _lib.last_error(eng.handle)          # (the direct call, outside the capture: it may allocate)
    torch.cuda.synchronize()
    want = op.results()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert op.call() == 0, _lib.last_error(eng.handle)
    for _ in range(2):
        op.v.fill_(float("nan"))
        op.tiles.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        got = op.results()
        got[3][0, 16:] = want[3][0, 16:]                        # (past T = 16 nothing is written)
        assert _equal_results(got, want)
    cur2, des2, Z2, _, _ = tc.fixture("48x64-l2-4x4-holes")     # other frames at the same addresses: the replay reads them
    op.cur[:cur2.size].copy_(torch.from_numpy(cur2.reshape(-1)))
    op.des[:des2.size].copy_(torch.from_numpy(des2.reshape(-1)))
    op.Z[:Z2.size].copy_(torch.from_numpy(Z2.reshape(-1)))
    op.tiles.zero_()
    graph.replay()
    torch.cuda.synchronize()
    replayed = op.results()
    assert op.call() == 0
    torch.cuda.synchronize()
    assert _equal_results(replayed, op.results()) and not _equal_results(replayed, want)


# ---------------------------------------------------------------------------------------------- statuses and refusals
def test_statuses(eng):
    cur, des, Z, _, K = tc.fixture("48x64-l2-8x8")
    flat = np.full_like(des, 77)
    v, info = eng.photometric_tile_velocity(flat, flat, Z, K, 2, 1, MU, LAM, 0.0, (4, 4), 4, 1.0)      # every tile flat: none live
    assert int(info["status"][0]) == _lib.STATUS_TOO_FEW and np.array_equal(v.cpu().numpy(), np.zeros((1, 6)))
    assert _pinfo(info) == [140, 12, 16, 12, 0, 1, 0, 0] and np.array_equal(_tiles4(info), np.zeros((16, 4)))
    assert (int(info["live_tiles"][0]), int(info["dead_tiles"][0]), info["sigma"][0], info["weight"][0]) == (0, 0, 0.0, 0.0)
    # a textured goal, no motion: v = 0 exactly, every weight 1, the dead tiles are the flat ones of the reference
    ref = tr.velocity(des, des, Z, 0.0, K, 2, 1, MU, LAM, 2, 2, 4, 1.0)
    v, info = eng.photometric_tile_velocity(des, des, Z, K, 2, 1, MU, LAM, 0.0, (2, 2), 4, 1.0)
    assert ref["status"] == pr.OK and int(info["status"][0]) == _lib.STATUS_OK and np.array_equal(v.cpu().numpy(), np.zeros((1, 6)))
    assert _pinfo(info) == [140, 12, 16, 12, 0, 0, 0, 4] and info["sigma"][0] == 1.0
    assert np.array_equal(_tiles4(info)[:, 3], ref["tiles"][:, 3]) and np.array_equal(_tiles4(info)[:, :2], np.zeros((4, 2)))
    # every depth a hole: no row; no depth at all
    v, info = eng.photometric_tile_velocity(cur, des, np.zeros_like(Z), K, 2, 1, MU, LAM, 0.0, (4, 4), 4, 1.0)
    assert int(info["status"][0]) == _lib.STATUS_TOO_FEW and _pinfo(info) == [0, 12, 16, 12, 140, 0, 0, 0]
    for form in (eng.photometric_tile_velocity, eng.photometric_tile_velocity_host):
        v, info = form(cur, des, None, K, 2, 1, MU, LAM, -1.0, (4, 4), 4, 1.0)
        v = v.cpu().numpy() if torch.is_tensor(v) else v
        assert int(info["status"][0]) == _lib.STATUS_NO_DEPTH and np.array_equal(v, np.zeros((1, 6)))
        assert _pinfo(info) == [0, 12, 16, 12, 0, 0, 0, 0] and np.array_equal(info["normal"], np.zeros((1, 16, 45)))
    # and the next call on the handle finds its histogram empty
    again = eng.photometric_tile_velocity(des, des, Z, K, 2, 1, MU, LAM, 0.0, (2, 2), 4, 1.0)[1]
    assert int(again["status"][0]) == _lib.STATUS_OK and again["sigma"][0] == 1.0 and _pinfo(again)[6:] == [0, 4]


def test_refusals(eng):
    cur, des, Z, _, K = tc.fixture("48x64-l2-8x8")
    op = _Raw(eng, cur, des, Z, K)
    nan, inf = float("nan"), float("inf")
    assert op.call() == 0
    bad = [dict(n=0), dict(n=-1), dict(n=eng.max_pairs + 1), dict(level=-1), dict(level=4), dict(inter=-1), dict(inter=2),
           dict(mu=-1e-9), dict(mu=nan), dict(mu=inf), dict(lam=nan), dict(lam=inf), dict(scale=nan), dict(scale=-inf),
           dict(H=11, level=2), dict(W=11, level=2), dict(H=2, level=0), dict(H=4097), dict(W=4097), dict(H=0), dict(W=-5),
           dict(N=-1), dict(N=5), dict(smin=0.0), dict(smin=-1.0), dict(smin=nan), dict(smin=inf),
           dict(gy=0), dict(gx=0), dict(gy=9), dict(gx=9), dict(gy=-1), dict(gy=8, level=3), dict(gx=8, W=28, level=2), dict(gy=7, H=24, level=2)]
    for kw in bad:
        assert op.call(**kw) == -2, kw
        assert _lib.last_error(eng.handle), kw
    assert op.call(cur=False) == -1 and op.call(robust=False) == -1 and op.call(tiles=False) == -1
    big = np.zeros((1, eng.params.v_max + 1, eng.params.u_max, 3), np.uint8)
    hp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    Kh, vh, sth, rh, th = np.array([K]), np.zeros((1, 6)), np.zeros(1, np.int32), np.zeros((1, 4)), np.zeros((1, 16, 4))
    rc = eng.lib.vitvs_photometric_tile_velocity(eng.handle, 1, hp(big), hp(big), big.shape[1], big.shape[2], None, 0.6, hp(Kh), 2, 1, MU,
                                                 LAM, 4, 4, 4, 1.0, hp(vh), hp(sth), hp(rh), hp(th), None, None)
    assert rc == -2 and "v_max" in _lib.last_error(eng.handle)
    assert op.call() == 0                                        # a refusal leaves the handle usable


def test_the_op_and_everything_else_the_handle_holds_leave_each_other_alone(eng):
    """A velocity call, a plain and a robust photometric call, then the tile op in both forms: last_details, vitvs_reselect, the
    next velocity call and the other photometric laws are what a fresh handle's are; and the tile op after all of them is what it
    was before."""
    cfg, params = eng.cfg, eng.params
    fresh = Engine(cfg, params, precision="fp32", max_pairs=4, max_rows=48).load_state_dict(weights.synthetic_state_dict(cfg, 0))
    try:
        des, cur = synth.frame_pair(64, 20250705)
        des2, cur2 = synth.frame_pair(64, 20250706)
        Z, K = synth.depth_pattern(), params.intrinsics()
        order = torch.randperm(eng.tokens, generator=torch.Generator().manual_seed(3)).to(torch.int32).numpy()
        curs, dess, Zs, Ks = _pairs_of_three()
        tile_args = (curs, dess, Zs, Ks, 2, 1, MU, LAM, 0.0, (4, 4), 4, SMIN)
        tv0, tinfo0 = fresh.photometric_tile_velocity(*tile_args)              # the op needs nothing before it
        first = [e.compute_velocity_host(cur, des, Z, K, _lib.SELECT_DENSE) for e in (eng, fresh)]
        assert np.array_equal(_bits(first[0][0]), _bits(first[1][0])) and np.array_equal(first[0][1], first[1][1])
        plain = [e.photometric_velocity(curs, dess, Zs, Ks, 2, 1, MU, LAM) for e in (eng, fresh)]
        robust = [e.photometric_robust_velocity(curs, dess, Zs, Ks, 2, 1, MU, LAM, 0.0, True, 4, SMIN) for e in (eng, fresh)]
        before = eng.last_details(1)
        tv1, tinfo1 = eng.photometric_tile_velocity(*tile_args)
        eng.photometric_tile_velocity_host(curs[:2], dess[:2], Zs[:2], Ks[:2], 1, 0, MU, LAM, 0.0, (2, 3), 3, 1.0)
        assert _same(tv0.cpu().numpy(), tinfo0, tv1.cpu().numpy(), tinfo1)
        after = eng.last_details(1)
        for name in before:
            assert np.array_equal(before[name], after[name], equal_nan=True), name
        again = [e.reselect_host(_lib.SELECT_ORDER, order[None], num_pairs=8) for e in (eng, fresh)]
        assert np.array_equal(_bits(again[0][0]), _bits(again[1][0])) and np.array_equal(again[0][1], again[1][1])
        plain2 = eng.photometric_velocity(curs, dess, Zs, Ks, 2, 1, MU, LAM)
        for pv, pi in (plain[1], plain2):
            assert np.array_equal(_bits(pv.cpu().numpy()), _bits(plain[0][0].cpu().numpy()))
            assert np.array_equal(_bits(pi["normal"]), _bits(plain[0][1]["normal"]))
        robust2 = eng.photometric_robust_velocity(curs, dess, Zs, Ks, 2, 1, MU, LAM, 0.0, True, 4, SMIN)
        for rv, ri in (robust[1], robust2):
            assert np.array_equal(_bits(rv.cpu().numpy()), _bits(robust[0][0].cpu().numpy()))
            for key in ("normal", "gamma", "bias", "sigma", "weight"):
                assert np.array_equal(_bits(ri[key]), _bits(robust[0][1][key])), key
        nxt = [e.compute_velocity_host(cur2, des2, Z, K, _lib.SELECT_ORDER, order, num_pairs=8) for e in (eng, fresh)]
        assert np.array_equal(_bits(nxt[0][0]), _bits(nxt[1][0])) and np.array_equal(nxt[0][1], nxt[1][1])
        d0, d1 = eng.last_details(1), fresh.last_details(1)
        for name in d0:
            assert np.array_equal(d0[name], d1[name], equal_nan=True), name
        tv2, tinfo2 = eng.photometric_tile_velocity(*tile_args)
        assert _same(tv0.cpu().numpy(), tinfo0, tv2.cpu().numpy(), tinfo2)
    finally:
        fresh.close()
