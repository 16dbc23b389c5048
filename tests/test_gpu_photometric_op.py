"""The photometric law on the device (vitvs_photometric_velocity[_dev], photometric.hip) against
tests/photometric_ref.py, the law in fp64 numpy (GPU).

Fixtures: des = synth.texture(96, 5)[:H, :W], cur = the same texture after synth.warp_similarity(shift (1.0, -0.7), 0.8 degrees,
scale 1.01, N(0, 1) noise, seed 5), Z = synth.depth_pattern(H, W), f = 30 px (60 from 48 x 64 up), the principal point at the
centre.  Shapes: 24 x 32 / level 0 (642 of 660 rows: 18 holes), 29 x 37 / level 1 (its ignored tail makes it the pooled image of
28 x 36: 192 rows), 48 x 64 / level 2 (140) and 88 x 96 / level 3 (90), each with both interaction matrices and with the depth image
or a scalar depth; 513 x 32 / level 0, whose 513 pooled rows are 256 bands of 2 and one row; 480 x 640 at levels 0 and 3; 5 x 4096
/ level 0 (the 640-px textures side by side, f = 2048), whose rows of 4096 pooled pixels need the LDS opt-in past 64 KiB; a batch of
three different pairs.

What is asserted per case:
  * the rows n, p_info and the status equal the reference's exactly;
  * each of the 28 sums is within (n + 16) 2^-53 sum |term| of the reference's: every term is formed by the reference's own
    operations in its own order (fp contraction off), so the two differ by the order of n - 1 additions, each of which rounds by at
    most 2^-53 of a partial sum that sum |term| bounds; the 16 leaves room for the roundings of a term itself;
  * v is within 1e-9 relative L2 (the project's bar for a twist) of photometric_ref.solve applied to the DEVICE's own sums.
Over all cases together: the gap between the device's twist and the reference's is at most ten times the gap between the reference
and itself summed in reversed row order (test_twist_gap_over_all_cases prints both).
Bit-identity: two calls, a pair alone against the same pair at any place of a batch, the host form against the _dev form.
Statuses, every -2 refusal, and independence of everything else a handle holds."""
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

pytestmark = pytest.mark.gpu

MU, LAM = 0.01, 0.5
U = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def _textures(size, seed=5):
    tex = synth.texture(size, seed)
    return tex, synth.warp_similarity(tex, shift=(1.0, -0.7), rot_deg=0.8, scale=1.01, noise_sigma=1.0, seed=seed)


@functools.lru_cache(maxsize=None)
def _fixture(H, W):
    """(cur, des, Z, K) at H x W."""
    size = 96 if max(H, W) <= 96 else 640
    tex, warped = _textures(size)
    if W > size:                                                 # a wide frame: the 640-px textures side by side
        tex, warped = (np.tile(a[:H], (1, -(-W // size), 1)) for a in (tex, warped))
    f = 30.0 if H < 48 else 60.0
    if W > size:
        f = W / 2.0                                              # a field of view of 90 degrees, as narrow frames have at f = 30
    return (np.ascontiguousarray(warped[:H, :W]), np.ascontiguousarray(tex[:H, :W]), synth.depth_pattern(H, W), (f, f, W / 2.0, H / 2.0))


# (H, W, level, interaction, with the depth image)
SMALL = [(H, W, level, inter, depth) for H, W, level in ((24, 32, 0), (29, 37, 1), (48, 64, 2), (88, 96, 3))
         for inter in (0, 1) for depth in (True, False)]
TAIL = [(513, 32, 0, 1, True), (513, 32, 0, 0, False)]
FULL = [(480, 640, 0, 1, True), (480, 640, 3, 0, True)]
WIDE = [(5, 4096, 0, 1, True)]     # 4096 pooled pixels per row: 113 KiB of LDS, the launch that opts in past 64 KiB
ROWS = {(24, 32, 0): 642, (29, 37, 1): 192, (48, 64, 2): 140, (88, 96, 3): 90}


@pytest.fixture(scope="module")
def eng():
    cfg = ls.tiny_cfg(64)
    params = config.ServoParams(dino_input_size=64, use_feature_binning=False)
    e = Engine(cfg, params, precision="fp32", max_pairs=4, max_rows=48).load_state_dict(weights.synthetic_state_dict(cfg, 0))
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def _reference(case, reverse=False):
    H, W, level, inter, depth = case
    cur, des, Z, K = _fixture(H, W)
    return pr.velocity(cur, des, Z if depth else None, 0.0 if depth else 0.6, K, level, inter, MU, LAM, reverse=reverse)


_DEVICE = {}


def _device(eng, case):
    """The case on the device, once per module: (v [6], info of pair 0)."""
    if case not in _DEVICE:
        H, W, level, inter, depth = case
        cur, des, Z, K = _fixture(H, W)
        v, info = eng.photometric_velocity(cur, des, Z if depth else None, K, level, inter, MU, LAM, 0.0 if depth else 0.6)
        _DEVICE[case] = (v.cpu().numpy()[0], info)
    return _DEVICE[case]


def _pinfo(info, b=0):
    return [int(info["n"][b]), int(info["pooled"][b, 0]), int(info["pooled"][b, 1]), int(info["bands"][b]), int(info["holes"][b]),
            int(info["pivot_failed"][b]), 0, 0]


def _check_against_reference(v, info, ref, what, b=0):
    n = int(ref["info"][0])
    print(f"{what}: n {int(info['n'][b])} (reference {n}), holes {int(info['holes'][b])}, bands {int(info['bands'][b])}, status "
          f"{int(info['status'][b])}")
    assert int(info["status"][b]) == ref["status"], what
    assert _pinfo(info, b) == list(ref["info"]), (what, _pinfo(info, b), list(ref["info"]))
    err = np.abs(info["normal"][b] - ref["normal"])
    bound = (n + 16) * U * ref["abs"]
    worst = float(np.max(np.where(bound > 0, err / np.maximum(bound, 1e-300), 0.0)))
    print(f"{what}: largest |sum - reference| / ((n + 16) 2^-53 sum |term|) over the 28 sums: {worst:.3f}")
    assert np.all(err <= bound), (what, err, bound)
    own, solved = pr.solve(info["normal"][b], MU, LAM)
    assert solved == (ref["status"] == pr.OK), what
    rel = float(np.linalg.norm(v - own) / max(np.linalg.norm(own), 1e-300))
    gap = float(np.linalg.norm(v - ref["v"]) / max(np.linalg.norm(ref["v"]), 1e-300))
    print(f"{what}: v against the solve of its own sums {rel:.2e}, against the reference's v {gap:.2e}; cond(H) "
          f"{np.linalg.cond(pr.unpack(ref['normal'])[0]):.1e}")
    assert rel <= 1e-9, (what, v, own)
    return gap


@pytest.mark.parametrize("case", SMALL + TAIL + FULL + WIDE, ids=lambda c: f"{c[0]}x{c[1]}-l{c[2]}-i{c[3]}-{'z' if c[4] else 'scalar'}")
def test_sums_and_twist_against_the_reference(eng, case):
    ref = _reference(case)
    assert ref["status"] == pr.OK
    if case[4] and case[:3] in ROWS:
        assert int(ref["info"][0]) == ROWS[case[:3]]
    v, info = _device(eng, case)
    _check_against_reference(v, info, ref, str(case))


def test_the_band_tail_is_a_band_of_one_row(eng):
    _, info = _device(eng, TAIL[0])
    assert _pinfo(info)[1:4] == [513, 32, 257]                  # 513 pooled rows = 256 bands of 2 and one row
    _, info = _device(eng, FULL[0])
    assert _pinfo(info)[1:4] == [480, 640, 480]
    _, info = _device(eng, WIDE[0])
    assert _pinfo(info)[1:4] == [5, 4096, 5]
    out = (C.c_int32 * 8)()
    assert eng.lib.vitvs_op_photometric_plan(5, 4096, 0, out) == 0 and out[4] > 64 * 1024 and out[6] == 1


def _pairs_of_three():
    """Three different pairs at 48 x 64: the fixture, the fixture's frames swapped, and another texture."""
    cur, des, Z, K = _fixture(48, 64)
    tex2, warped2 = _textures(96, 6)
    curs = np.stack([cur, des, np.ascontiguousarray(warped2[:48, :64])])
    dess = np.stack([des, cur, np.ascontiguousarray(tex2[:48, :64])])
    Zs = np.stack([Z, np.ascontiguousarray(Z[::-1]), np.ascontiguousarray(Z[:, ::-1])])
    Ks = np.array([K, (55.0, 65.0, 30.0, 25.0), (70.0, 60.0, 33.5, 22.5)])
    return curs, dess, Zs, Ks


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(v1, i1, v2, i2, b1=slice(None), b2=slice(None)):
    return (np.array_equal(_bits(v1[b1]), _bits(v2[b2])) and np.array_equal(_bits(i1["normal"][b1]), _bits(i2["normal"][b2]))
            and np.array_equal(i1["status"][b1], i2["status"][b2]) and np.array_equal(i1["n"][b1], i2["n"][b2])
            and np.array_equal(i1["holes"][b1], i2["holes"][b2]))


@pytest.mark.parametrize("level,inter", [(2, 1), (0, 0), (1, 1)])
def test_a_batch_of_three_pairs(eng, level, inter):
    curs, dess, Zs, Ks = _pairs_of_three()
    v, info = eng.photometric_velocity(curs, dess, Zs, Ks, level, inter, MU, LAM)
    v = v.cpu().numpy()
    for b in range(3):
        ref = pr.velocity(curs[b], dess[b], Zs[b], 0.0, Ks[b], level, inter, MU, LAM)
        _check_against_reference(v[b], info, ref, f"batch pair {b}, level {level}, interaction {inter}", b)
        alone_v, alone = eng.photometric_velocity(curs[b], dess[b], Zs[b:b + 1], Ks[b], level, inter, MU, LAM)
        assert _same(v, info, alone_v.cpu().numpy(), alone, slice(b, b + 1)), f"pair {b} alone is not pair {b} of the batch"
    back = [2, 0, 1]                                            # the same pairs at other places of a batch
    v2, info2 = eng.photometric_velocity(curs[back], dess[back], Zs[back], Ks[back], level, inter, MU, LAM)
    v2 = v2.cpu().numpy()
    for place, b in enumerate(back):
        assert _same(v, info, v2, info2, slice(b, b + 1), slice(place, place + 1)), f"pair {b} at place {place}"


@pytest.mark.parametrize("case", [SMALL[0], SMALL[5], SMALL[10], TAIL[0], FULL[1]], ids=str)
def test_two_calls_and_both_forms_are_bit_identical(eng, case):
    H, W, level, inter, depth = case
    cur, des, Z, K = _fixture(H, W)
    args = (cur, des, Z if depth else None, K, level, inter, MU, LAM, 0.0 if depth else 0.6)
    v1, i1 = eng.photometric_velocity(*args)
    v2, i2 = eng.photometric_velocity(*args)
    vh, ih = eng.photometric_velocity_host(*args)
    assert _same(v1.cpu().numpy(), i1, v2.cpu().numpy(), i2), "two calls"
    assert _same(v1.cpu().numpy(), i1, vh, ih), "the host form against the _dev form"
    assert np.array_equal(i1["pooled"], ih["pooled"]) and np.array_equal(i1["bands"], ih["bands"])


def test_frames_at_odd_addresses_take_the_narrow_loads_to_the_same_bits(eng):
    """The same pair behind 0, 1, 4 and 5 bytes of padding: 16-byte, byte, dword and byte loads of the frame rows (and the depth
    image behind 0, 1 and 2 samples) give the same integers, so the same bits."""
    cur, des, Z, K = _fixture(48, 64)
    want_v, want = eng.photometric_velocity(cur, des, Z[None], K, 2, 1, MU, LAM)
    dev = eng.device
    Kd = torch.tensor([K], dtype=torch.float64, device=dev)
    for pad, zpad in ((1, 1), (4, 2), (5, 0)):
        def padded(a, k):
            host = np.zeros(a.size + 16, a.dtype)
            host[k:k + a.size] = a.reshape(-1)
            return torch.from_numpy(host).to(dev)
        bc, bd, bz = padded(cur, pad), padded(des, pad), padded(Z, zpad)
        v = torch.empty((1, 6), dtype=torch.float64, device=dev)
        st = torch.empty(1, dtype=torch.int32, device=dev)
        normal = torch.empty((1, 28), dtype=torch.float64, device=dev)
        pinfo = torch.empty((1, 8), dtype=torch.int32, device=dev)
        p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
        rc = eng.lib.vitvs_photometric_velocity_dev(eng.handle, 1, p(bc, pad), p(bd, pad), 48, 64, p(bz, 2 * zpad), 0.0, p(Kd), 2, 1, MU, LAM,
                                                    p(v), p(st), p(normal), p(pinfo),
                                                    C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        assert rc == 0, _lib.last_error(eng.handle)
        assert np.array_equal(_bits(v.cpu().numpy()), _bits(want_v.cpu().numpy())), pad
        assert np.array_equal(_bits(normal.cpu().numpy()), _bits(want["normal"])), pad
        assert int(pinfo[0, 0]) == int(want["n"][0]) and int(pinfo[0, 4]) == int(want["holes"][0])


def test_identical_frames_give_an_exact_zero(eng):
    for H, W, level in ((24, 32, 0), (48, 64, 2)):
        _, des, Z, K = _fixture(H, W)
        for inter in (0, 1):
            v, info = eng.photometric_velocity(des, des, Z[None], K, level, inter, MU, LAM)
            assert int(info["status"][0]) == _lib.STATUS_OK and np.array_equal(v.cpu().numpy(), np.zeros((1, 6)))
            assert np.array_equal(info["normal"][0, 21:], np.zeros(7)) and info["normal"][0, 0] > 0


def test_too_few_and_no_depth(eng):
    cur, des, Z, K = _fixture(48, 64)
    flat = np.full_like(des, 77)
    for a, b, z, scalar, want in ((flat, flat, Z, 0.0, [140, 12, 16, 12, 0, 1, 0, 0]),              # a constant frame: H = 0, no pivot
                                  (cur, des, np.zeros_like(Z), 0.0, [0, 12, 16, 12, 140, 0, 0, 0])):  # every depth a hole: no row
        v, info = eng.photometric_velocity(a, b, z[None], K, 2, 1, MU, LAM, scalar)
        assert int(info["status"][0]) == _lib.STATUS_TOO_FEW and np.array_equal(v.cpu().numpy(), np.zeros((1, 6)))
        assert _pinfo(info) == want
        ref = pr.velocity(a, b, z, scalar, K, 2, 1, MU, LAM)
        assert ref["status"] == pr.TOO_FEW and list(ref["info"]) == want
    for scalar in (0.0, -1.0):
        for form in (eng.photometric_velocity, eng.photometric_velocity_host):
            v, info = form(cur, des, None, K, 2, 1, MU, LAM, scalar)
            v = v.cpu().numpy() if torch.is_tensor(v) else v
            assert int(info["status"][0]) == _lib.STATUS_NO_DEPTH and np.array_equal(v, np.zeros((1, 6)))
            assert _pinfo(info) == [0, 12, 16, 12, 0, 0, 0, 0] and np.array_equal(info["normal"], np.zeros((1, 28)))
    assert list(pr.velocity(cur, des, None, 0.0, K, 2, 1, MU, LAM)["info"]) == [0, 12, 16, 12, 0, 0, 0, 0]
    # five rows: a 3 x 7 pooled image has one interior row of five pixels
    v, info = eng.photometric_velocity(cur[:3, :7], des[:3, :7], None, K, 0, 1, MU, LAM, 0.6)
    assert int(info["status"][0]) == _lib.STATUS_TOO_FEW and _pinfo(info) == [5, 3, 7, 3, 0, 0, 0, 0]


def test_refusals(eng):
    cur, des, Z, K = _fixture(48, 64)
    dev = eng.device
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    c, d, z = t(cur[None]), t(des[None]), t(Z[None])
    Kd = torch.tensor([K], dtype=torch.float64, device=dev)
    v = torch.empty((4, 6), dtype=torch.float64, device=dev)
    st = torch.empty(4, dtype=torch.int32, device=dev)
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    nan, inf = float("nan"), float("inf")

    def call(n=1, H=48, W=64, scale=0.0, level=2, inter=1, mu=MU, lam=LAM):
        return eng.lib.vitvs_photometric_velocity_dev(eng.handle, n, p(c), p(d), H, W, p(z), scale, p(Kd), level, inter, mu, lam, p(v),
                                                      p(st), None, None, stream)
    assert call() == 0
    bad = [dict(n=0), dict(n=-1), dict(n=eng.max_pairs + 1), dict(level=-1), dict(level=4), dict(inter=-1), dict(inter=2),
           dict(mu=-1e-9), dict(mu=nan), dict(mu=inf), dict(lam=nan), dict(lam=inf), dict(scale=nan), dict(scale=-inf),
           dict(H=11, level=2), dict(W=11, level=2), dict(H=2, level=0), dict(H=4097), dict(W=4097), dict(H=0), dict(W=-5)]
    for kw in bad:
        assert call(**kw) == -2, kw
        assert _lib.last_error(eng.handle), kw
    assert eng.lib.vitvs_photometric_velocity_dev(eng.handle, 1, None, p(d), 48, 64, p(z), 0.0, p(Kd), 2, 1, MU, LAM, p(v), p(st), None, None,
                                                  stream) == -1
    # the host form stages frames of at most v_max x u_max pixels
    big = np.zeros((1, eng.params.v_max + 1, eng.params.u_max, 3), np.uint8)
    hp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    Kh, vh, sth = np.array([K]), np.zeros((1, 6)), np.zeros(1, np.int32)
    rc = eng.lib.vitvs_photometric_velocity(eng.handle, 1, hp(big), hp(big), big.shape[1], big.shape[2], None, 0.6, hp(Kh), 2, 1, MU, LAM,
                                            hp(vh), hp(sth), None, None)
    assert rc == -2 and "v_max" in _lib.last_error(eng.handle)
    assert call() == 0                                           # a refusal leaves the handle usable


def test_the_op_is_independent_of_everything_else_the_handle_holds(eng):
    """A velocity call, then the op in both forms, then last_details and vitvs_reselect are what they were; the next velocity
    call equals a fresh handle's bit for bit."""
    cfg, params = eng.cfg, eng.params
    fresh = Engine(cfg, params, precision="fp32", max_pairs=4, max_rows=48).load_state_dict(weights.synthetic_state_dict(cfg, 0))
    try:
        des, cur = synth.frame_pair(64, 20250705)
        des2, cur2 = synth.frame_pair(64, 20250706)
        Z, K = synth.depth_pattern(), params.intrinsics()
        order = torch.randperm(eng.tokens, generator=torch.Generator().manual_seed(3)).to(torch.int32).numpy()
        first = [e.compute_velocity_host(cur, des, Z, K, _lib.SELECT_DENSE) for e in (eng, fresh)]
        assert np.array_equal(_bits(first[0][0]), _bits(first[1][0])) and np.array_equal(first[0][1], first[1][1])
        before = eng.last_details(1)
        curs, dess, Zs, Ks = _pairs_of_three()
        eng.photometric_velocity(curs, dess, Zs, Ks, 2, 1, MU, LAM)
        eng.photometric_velocity_host(curs, dess, Zs, Ks, 1, 0, MU, LAM)
        fc, fd, fz, fk = _fixture(480, 640)
        eng.photometric_velocity_host(fc, fd, fz, fk, 0, 1, MU, LAM)
        after = eng.last_details(1)
        for name in before:
            assert np.array_equal(before[name], after[name], equal_nan=True), name
        again = [e.reselect_host(_lib.SELECT_ORDER, order[None], num_pairs=8) for e in (eng, fresh)]
        assert np.array_equal(_bits(again[0][0]), _bits(again[1][0])) and np.array_equal(again[0][1], again[1][1])
        nxt = [e.compute_velocity_host(cur2, des2, Z, K, _lib.SELECT_ORDER, order, num_pairs=8) for e in (eng, fresh)]
        assert np.array_equal(_bits(nxt[0][0]), _bits(nxt[1][0])) and np.array_equal(nxt[0][1], nxt[1][1])
        d0, d1 = eng.last_details(1), fresh.last_details(1)
        for name in d0:
            assert np.array_equal(d0[name], d1[name], equal_nan=True), name
        # and the op needs no velocity call before it: a handle that never made one
        v, info = fresh.photometric_velocity(curs, dess, Zs, Ks, 2, 1, MU, LAM)
        v0, info0 = eng.photometric_velocity(curs, dess, Zs, Ks, 2, 1, MU, LAM)
        assert _same(v.cpu().numpy(), info, v0.cpu().numpy(), info0)
    finally:
        fresh.close()


def test_twist_gap_over_all_cases(eng):
    """The device's twist against the reference's own, over every case above: at most ten times the gap the reference shows
    against itself summed in reversed row order."""
    gap_dev, gap_self = 0.0, 0.0
    for case in SMALL + TAIL + FULL + WIDE:
        ref, rev = _reference(case), _reference(case, True)
        v, _ = _device(eng, case)
        norm = max(np.linalg.norm(ref["v"]), 1e-300)
        gap_dev = max(gap_dev, float(np.linalg.norm(v - ref["v"]) / norm))
        gap_self = max(gap_self, float(np.linalg.norm(rev["v"] - ref["v"]) / norm))
    print(f"twist gap over {len(SMALL + TAIL + FULL + WIDE)} cases: device against the reference {gap_dev:.3e}; the reference against itself "
          f"summed in reversed row order {gap_self:.3e}")
    assert gap_dev <= 10.0 * gap_self
