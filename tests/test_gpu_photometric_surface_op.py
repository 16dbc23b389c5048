"""The surface photometric law on the device (vitvs_photometric_surface_velocity[_dev], photometric.hip) against
tests/photometric_surface_ref.py, the law in fp64 numpy (GPU).

Inputs: tests/photometric_surface_cases.py: the tile op test's crops with cells in the place of tiles, every crop under a gain ramp
(0.9 .. 1.1 across its width) plus a bias of 8.  The cases are the smallest at which the new code can go wrong:
  24 x 32, level 0, 2 x 2 and 3 x 5   cell edges that do not divide the sides       23 x 29, level 0, 4 x 4   odd sides, byte loads
  48 x 64, level 2, 4 x 4 with holes, and 8 x 8 (162 unknowns, half-bandwidth 21)    70 x 32, level 0, 8 x 2   9 bands per cell row: the
  1042 x 16, level 1, 3 x 1   pooled 521 rows in two-row bands, the cell rows beginning where bands begin     solve's second group of 8
  1042 x 16, level 1, 4 x 1   the same with three bands across a cell-row edge: both slots written, the second read
  24 x 32 RGB-only with a scalar depth, 48 x 64 with a flat patch (a dead bias), 24 x 8 with gx = pooled w (dead border nodes)
sigma_min is 0.01 in the cases, below the smallest scale a histogram bin can give, so that the returned sigma tells the median bin.
The origins were searched so that NO case has to be left out of an exact comparison (test_photometric_surface_host.py asserts that
on the reference alone): for every case and every N of 0, 1 and 4
  * status, n, holes, the pivot flag, the re-weightings, the median bin, the rows at weight 0 and the set of dead unknowns are exact;
  * N = 0: each of the 120 sums per cell within (n_cell + 16) 2^-53 sum |term| (the terms are the reference's own);
  * N >= 1: v (relative L2), gamma_a, beta_a (absolute, the largest over the nodes) and sum w (relative) within ten times the
    reference's distance to itself with every cell's rows reversed and the cells taken in descending order, case by case (printed);
  * the same bits: two calls and both forms, a pair alone against the same pair at places 0 and 2 of a batch of 3, a captured graph's
    replay against the plain call;
  * every refusal; the plain, robust, tile and rig calls of the same handle give the same bits before and after a surface call."""
import ctypes as C

import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib, config, weights
from vitvs_amd.engine import Engine
import law_support as ls
import photometric_ref as pr
import photometric_robust_ref as rr
import photometric_surface_ref as sr
import photometric_surface_cases as sc
import photometric_rig_cases as pc

pytestmark = pytest.mark.gpu

MU, LAM, SMIN = sc.MU, sc.LAM, sc.SMIN
U = 2.0 ** -53
CASES = sc.CASES


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
        cur, des, Z, scalar, K = sc.fixture(name)
        v, info = eng.photometric_surface_velocity(cur, des, Z, K, level, inter, MU, LAM, scalar, grid, N, smin)
        _DEVICE[key] = (v.cpu().numpy()[0], info)
    return _DEVICE[key]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _pinfo(info, b=0):
    return [int(info["n"][b]), int(info["pooled"][b, 0]), int(info["pooled"][b, 1]), int(info["bands"][b]), int(info["holes"][b]),
            int(info["pivot_failed"][b]), int(info["zero_weight"][b]), int(info["reweightings"][b])]


def _nodes4(info, b=0):
    """[nodes, 4] gamma_a, beta_a, gamma_a live, beta_a live of pair b."""
    return np.stack([info["node_gain"][b] - 1.0, info["node_bias"][b], info["node_live"][b].astype(np.float64),
                     info["node_bias_live"][b].astype(np.float64)], axis=-1).reshape(-1, 4)


KEYS = ("normal", "node_gain", "node_bias", "sigma", "weight")
INTS = ("status", "n", "holes", "zero_weight", "reweightings", "node_live", "node_bias_live", "live", "dead")


def _same(v1, i1, v2, i2, b1=slice(None), b2=slice(None)):
    return (np.array_equal(_bits(v1[b1]), _bits(v2[b2])) and all(np.array_equal(_bits(i1[k][b1]), _bits(i2[k][b2])) for k in KEYS)
            and all(np.array_equal(i1[k][b1], i2[k][b2]) for k in INTS))


def _bin_of(sigma):
    return int(round(sigma / rr.MAD_SCALE * rr.BIN_SCALE - 0.5))


def _check_exact(info, ref, N, what, b=0):
    """Status, every count, the median bin, the rows at weight 0 and the set of dead unknowns."""
    assert int(info["status"][b]) == ref["status"] == pr.OK, what
    assert _pinfo(info, b) == list(ref["info"]), (what, _pinfo(info, b), list(ref["info"]))
    assert (int(info["live"][b]), int(info["dead"][b])) == (int(ref["robust"][0]), int(ref["robust"][1])), what
    assert np.array_equal(_nodes4(info, b)[:, 2:], ref["nodes"][:, 2:]), what
    assert np.array_equal(_nodes4(info, b)[:, :2][ref["nodes"][:, 2:] == 0], np.zeros(int(ref["robust"][1]))), what
    if N == 0:
        assert info["sigma"][b] == 0.0
    else:
        last = ref["passes"][-1]
        assert last["sigma"] > SMIN and _bin_of(last["sigma"]) == last["bin"]
        assert _bin_of(float(info["sigma"][b])) == last["bin"], what


@pytest.mark.parametrize("name", list(CASES))
def test_one_solve_against_the_reference(eng, name):
    ref = sc.reference(name, 0)
    v, info = _device(eng, name, 0)
    _check_exact(info, ref, 0, name)
    err = np.abs(info["normal"][0] - ref["normal"])
    bound = (ref["cell_n"][:, None] + 16) * U * ref["abs"]
    worst = float(np.max(np.where(bound > 0, err / np.maximum(bound, 1e-300), 0.0)))
    print(f"{name}: n {ref['info'][0]} in cells of {ref['cell_n'].min()} .. {ref['cell_n'].max()} rows, largest |sum - reference| / "
          f"((n_cell + 16) 2^-53 sum |term|) over the cells' 120 sums: {worst:.3f}")
    assert np.all(err <= bound), (name, np.argwhere(err > bound))
    gy, gx = CASES[name][3]
    own_v, _, own_q, own_live, _, solved = sr.solve_cells(info["normal"][0], gy, gx, MU, LAM)
    assert solved and np.array_equal(own_live.reshape(-1, 2), ref["nodes"][:, 2:] != 0)
    got = _nodes4(info)
    print(f"{name}: v against the reference's solve of the device's sums {np.linalg.norm(v - own_v) / np.linalg.norm(own_v):.2e}, "
          f"(gamma_a, beta_a) {np.max(np.abs(got[:, :2] - own_q.reshape(-1, 2))):.2e}; against the reference's v "
          f"{np.linalg.norm(v - ref['v']) / np.linalg.norm(ref['v']):.2e}; live {int(ref['robust'][0])}, dead {int(ref['robust'][1])}")
    assert info["weight"][0] == float(ref["info"][0])            # every weight 1: the sum is exact


def _gaps(v, nodes, weight, ref):
    return np.array([np.linalg.norm(v - ref["v"]) / max(np.linalg.norm(ref["v"]), 1e-300), np.max(np.abs(nodes[:, 0] - ref["nodes"][:, 0])),
                     np.max(np.abs(nodes[:, 1] - ref["nodes"][:, 1])), abs(weight - ref["robust"][3]) / ref["robust"][3]])


def case_gaps(eng, name):
    """(device against the reference, the reference against its reversed self): v, gamma_a, beta_a, sum w, the largest over N >= 1."""
    gap_dev, gap_self = np.zeros(4), np.zeros(4)
    for N in sc.NS[1:]:
        ref, rev = sc.reference(name, N), sc.reference(name, N, True)
        v, info = _device(eng, name, N)
        gap_dev = np.maximum(gap_dev, _gaps(v, _nodes4(info), float(info["weight"][0]), ref))
        gap_self = np.maximum(gap_self, _gaps(rev["v"], rev["nodes"], rev["robust"][3], ref))
    return gap_dev, gap_self


@pytest.mark.parametrize("name", list(CASES))
def test_reweighted_passes_against_the_reference(eng, name):
    for N in sc.NS[1:]:
        ref = sc.reference(name, N)
        v, info = _device(eng, name, N)
        print(f"{name} N {N}: median bin {_bin_of(float(info['sigma'][0]))} (reference {ref['passes'][-1]['bin']}, margin {ref['margin_m']} "
              f"rows), rows of weight 0 {_pinfo(info)[6]} (reference {ref['info'][6]}), live {int(info['live'][0])} dead {int(info['dead'][0])}")
        _check_exact(info, ref, N, (name, N))
    gap_dev, gap_self = case_gaps(eng, name)
    print(f"{name}, gaps over N = 1, 4 (v relative L2, gamma_a, beta_a, sum w relative): the device against the reference "
          + " ".join(f"{g:.3e}" for g in gap_dev) + "; the reference against itself in reversed order " + " ".join(f"{g:.3e}" for g in gap_self))
    assert np.all(gap_dev <= 10.0 * gap_self), (gap_dev, gap_self)


# ---------------------------------------------------------------------------------------------- bit-identity
def _pairs_of_three():
    names = ("48x64-l2-8x8", "48x64-l2-4x4-holes", "48x64-l2-4x4-flat")
    fx = [sc.fixture(n) for n in names]
    curs, dess, Zs = (np.stack([f[i] for f in fx]) for i in range(3))
    Ks = np.array([fx[0][4], fx[1][4], (55.0, 65.0, 30.0, 25.0)])
    return curs, dess, Zs, Ks


@pytest.mark.parametrize("grid,N", [((4, 4), 4), ((8, 8), 1), ((3, 5), 0)])
def test_a_pair_alone_and_in_a_batch_of_three(eng, grid, N):
    curs, dess, Zs, Ks = _pairs_of_three()
    args = (2, 1, MU, LAM, 0.0, grid, N, SMIN)
    alone_v, alone = eng.photometric_surface_velocity(curs[0], dess[0], Zs[:1], Ks[0], *args)
    alone_v = alone_v.cpu().numpy()
    assert int(alone["status"][0]) == pr.OK
    pick = [0, 1, 0]                                             # the pair at places 0 and 2
    v, info = eng.photometric_surface_velocity(curs[pick], dess[pick], Zs[pick], Ks[pick], *args)
    v = v.cpu().numpy()
    for place in (0, 2):
        assert _same(alone_v, alone, v, info, slice(0, 1), slice(place, place + 1)), f"the pair alone against place {place}"
    other_v, other = eng.photometric_surface_velocity(curs[1], dess[1], Zs[1:2], Ks[1], *args)
    assert _same(other_v.cpu().numpy(), other, v, info, slice(0, 1), slice(1, 2)) and not _same(alone_v, alone, v, info, slice(0, 1), slice(1, 2))


@pytest.mark.parametrize("name", ["24x32-l0-3x5", "23x29-l0-4x4", "48x64-l2-8x8", "1042x16-l1-4x1", "24x32-l0-rgb-2x2", "24x8-l0-2x8"])
def test_two_calls_and_both_forms_are_bit_identical(eng, name):
    _, _, level, grid, _, _, _, inter, _ = CASES[name]
    cur, des, Z, scalar, K = sc.fixture(name)
    args = (cur, des, Z, K, level, inter, MU, LAM, scalar, grid, 4, SMIN)
    v1, i1 = eng.photometric_surface_velocity(*args)
    v2, i2 = eng.photometric_surface_velocity(*args)
    vh, ih = eng.photometric_surface_velocity_host(*args)
    assert _same(v1.cpu().numpy(), i1, v2.cpu().numpy(), i2), "two calls"
    assert _same(v1.cpu().numpy(), i1, vh, ih), "the host form against the _dev form"
    d0 = _device(eng, name, 4)
    assert _same(v1.cpu().numpy(), i1, d0[0][None], d0[1]), "a call made earlier on this handle"


class _Raw:
    """One pair's device buffers and the raw _dev call on them."""

    def __init__(self, eng, cur, des, Z, K):
        dev = eng.device
        self.eng, self.shape = eng, cur.shape[:2]
        self.cur, self.des, self.Z = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (cur, des, Z))
        self.K = torch.tensor([K], dtype=torch.float64, device=dev)
        self.v = torch.empty((1, 6), dtype=torch.float64, device=dev)
        self.st = torch.empty(1, dtype=torch.int32, device=dev)
        self.robust = torch.empty((1, 4), dtype=torch.float64, device=dev)
        self.nodes = torch.zeros((1, 81, 4), dtype=torch.float64, device=dev)
        self.sums = torch.zeros((1, 64, 120), dtype=torch.float64, device=dev)
        self.pinfo = torch.empty((1, 8), dtype=torch.int32, device=dev)

    def call(self, level=2, inter=1, gy=4, gx=4, N=4, smin=SMIN, n=1, H=None, W=None, scale=0.0, mu=MU, lam=LAM, cur=True, robust=True,
             nodes=True):
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        e = self.eng
        return e.lib.vitvs_photometric_surface_velocity_dev(
            e.handle, n, p(self.cur) if cur else None, p(self.des), self.shape[0] if H is None else H,
            self.shape[1] if W is None else W, p(self.Z), scale, p(self.K), level, inter, mu, lam, gy, gx, N, smin, p(self.v),
            p(self.st), p(self.robust) if robust else None, p(self.nodes) if nodes else None, p(self.sums), p(self.pinfo),
            C.c_void_p(torch.cuda.current_stream(e.device).cuda_stream))

    def results(self):
        return [t.cpu().numpy().copy() for t in (self.v, self.st, self.robust, self.nodes, self.sums, self.pinfo)]


def _equal_results(a, b):
    return all(np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x, y.view(np.uint64) if y.dtype == np.float64 else y)
               for x, y in zip(a, b))


def test_a_captured_graph_replays_the_direct_call(eng):
    cur, des, Z, _, K = sc.fixture("48x64-l2-8x8")
    op = _Raw(eng, cur, des, Z, K)
    assert op.call(gy=8, gx=8) == 0, _lib.last_error(eng.handle)          # (the direct call, outside the capture: it may allocate)
    torch.cuda.synchronize()
    want = op.results()
    assert int(want[1][0]) == pr.OK and want[5][0, 7] == 4
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert op.call(gy=8, gx=8) == 0, _lib.last_error(eng.handle)
    for _ in range(2):
        op.v.fill_(float("nan"))
        op.nodes.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert _equal_results(op.results(), want)
    cur2, des2, Z2, _, _ = sc.fixture("48x64-l2-4x4-holes")     # other frames at the same addresses: the replay reads them
    op.cur.copy_(torch.from_numpy(cur2))
    op.des.copy_(torch.from_numpy(des2))
    op.Z.copy_(torch.from_numpy(Z2))
    graph.replay()
    torch.cuda.synchronize()
    replayed = op.results()
    assert op.call(gy=8, gx=8) == 0
    torch.cuda.synchronize()
    assert _equal_results(replayed, op.results()) and not _equal_results(replayed, want)


# ---------------------------------------------------------------------------------------------- statuses and refusals
def test_statuses(eng):
    cur, des, Z, _, K = sc.fixture("48x64-l2-8x8")
    black = np.zeros_like(des)                                   # D = 0 and e = 0: every unknown dead
    v, info = eng.photometric_surface_velocity(black, black, Z, K, 2, 1, MU, LAM, 0.0, (4, 4), 4, 1.0)
    assert int(info["status"][0]) == _lib.STATUS_TOO_FEW and np.array_equal(v.cpu().numpy(), np.zeros((1, 6)))
    assert _pinfo(info) == [140, 12, 16, 12, 0, 1, 0, 0] and np.array_equal(_nodes4(info), np.zeros((25, 4)))
    assert (int(info["live"][0]), int(info["dead"][0]), info["sigma"][0], info["weight"][0]) == (0, 0, 0.0, 0.0)
    # a textured goal, no motion: every weight 1, the dead unknowns are the reference's
    ref = sr.velocity(des, des, Z, 0.0, K, 2, 1, MU, LAM, 2, 2, 4, 1.0)
    v, info = eng.photometric_surface_velocity(des, des, Z, K, 2, 1, MU, LAM, 0.0, (2, 2), 4, 1.0)
    assert ref["status"] == pr.OK and int(info["status"][0]) == _lib.STATUS_OK and np.max(np.abs(v.cpu().numpy())) < 1e-12
    assert _pinfo(info) == [140, 12, 16, 12, 0, 0, 0, 4] and info["sigma"][0] == 1.0 and info["weight"][0] == 140.0
    assert np.array_equal(_nodes4(info)[:, 2:], ref["nodes"][:, 2:])
    # every depth a hole: no row; no depth at all
    v, info = eng.photometric_surface_velocity(cur, des, np.zeros_like(Z), K, 2, 1, MU, LAM, 0.0, (4, 4), 4, 1.0)
    assert int(info["status"][0]) == _lib.STATUS_TOO_FEW and _pinfo(info) == [0, 12, 16, 12, 140, 0, 0, 0]
    for form in (eng.photometric_surface_velocity, eng.photometric_surface_velocity_host):
        v, info = form(cur, des, None, K, 2, 1, MU, LAM, -1.0, (4, 4), 4, 1.0)
        v = v.cpu().numpy() if torch.is_tensor(v) else v
        assert int(info["status"][0]) == _lib.STATUS_NO_DEPTH and np.array_equal(v, np.zeros((1, 6)))
        assert _pinfo(info) == [0, 12, 16, 12, 0, 0, 0, 0] and np.array_equal(info["normal"], np.zeros((1, 16, 120)))
    # and the next call on the handle finds its histogram empty
    again = eng.photometric_surface_velocity(des, des, Z, K, 2, 1, MU, LAM, 0.0, (2, 2), 4, 1.0)[1]
    assert int(again["status"][0]) == _lib.STATUS_OK and again["sigma"][0] == 1.0 and _pinfo(again)[6:] == [0, 4]


def test_refusals(eng):
    cur, des, Z, _, K = sc.fixture("48x64-l2-8x8")
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
    assert "1 .. 8" in (op.call(gy=9), _lib.last_error(eng.handle))[1] and "pooled" in (op.call(gy=8, level=3), _lib.last_error(eng.handle))[1]
    assert op.call(cur=False) == -1 and op.call(robust=False) == -1 and op.call(nodes=False) == -1
    big = np.zeros((1, eng.params.v_max + 1, eng.params.u_max, 3), np.uint8)
    hp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    Kh, vh, sth, rh, nh = np.array([K]), np.zeros((1, 6)), np.zeros(1, np.int32), np.zeros((1, 4)), np.zeros((1, 25, 4))
    rc = eng.lib.vitvs_photometric_surface_velocity(eng.handle, 1, hp(big), hp(big), big.shape[1], big.shape[2], None, 0.6, hp(Kh), 2, 1,
                                                    MU, LAM, 4, 4, 4, 1.0, hp(vh), hp(sth), hp(rh), hp(nh), None, None)
    assert rc == -2 and "v_max" in _lib.last_error(eng.handle)
    assert op.call() == 0                                        # a refusal leaves the handle usable


def test_the_other_photometric_laws_give_the_same_bits_before_and_after_a_surface_call(eng):
    """The plain, robust, tile and rig calls of one handle, a surface call in both forms, and the four again; and the surface call
    after them is what it was before."""
    curs, dess, Zs, Ks = _pairs_of_three()
    _, _, _, rig_level, _, _, _, rig_inter, _ = pc.CASES["3cam-holes"]
    rig_cur, rig_des, rig_Z, rig_scalar, rig_K, rig_W6, _ = pc.fixture("3cam-holes")
    surf_args = (curs, dess, Zs, Ks, 2, 1, MU, LAM, 0.0, (4, 4), 4, SMIN)

    def others():
        pv, pi = eng.photometric_velocity(curs, dess, Zs, Ks, 2, 1, MU, LAM)
        rv, ri = eng.photometric_robust_velocity(curs, dess, Zs, Ks, 2, 1, MU, LAM, 0.0, True, 4, SMIN)
        tv, ti = eng.photometric_tile_velocity(curs, dess, Zs, Ks, 2, 1, MU, LAM, 0.0, (4, 4), 4, SMIN)
        gv, gi = eng.photometric_rig_velocity(rig_cur, rig_des, rig_Z, rig_K, rig_W6, None, rig_level, rig_inter, MU, LAM, rig_scalar, True, 4, SMIN)
        out = [pv.cpu().numpy(), pi["normal"], rv.cpu().numpy(), ri["normal"], ri["gamma"], ri["bias"], ri["sigma"], ri["weight"],
               tv.cpu().numpy(), ti["normal"], ti["tile_gain"], ti["tile_bias"], ti["tile_weight"], ti["sigma"],
               gv.cpu().numpy(), gi["normal"], gi["gain"], gi["bias"], gi["sigma"]]
        assert int(gi["status"]) == pr.OK and int(pi["status"][0]) == int(ri["status"][0]) == int(ti["status"][0]) == pr.OK
        return [np.asarray(o, np.float64) for o in out]
    s0 = eng.photometric_surface_velocity(*surf_args)
    before = others()
    s1 = eng.photometric_surface_velocity(*surf_args)
    eng.photometric_surface_velocity_host(curs[:2], dess[:2], Zs[:2], Ks[:2], 1, 0, MU, LAM, 0.0, (2, 3), 3, 1.0)
    after = others()
    for k, (x, y) in enumerate(zip(before, after)):
        assert np.array_equal(_bits(x), _bits(y)), k
    s2 = eng.photometric_surface_velocity(*surf_args)
    assert _same(s0[0].cpu().numpy(), s0[1], s1[0].cpu().numpy(), s1[1]) and _same(s0[0].cpu().numpy(), s0[1], s2[0].cpu().numpy(), s2[1])
    assert not s0[1]["status"].any()
