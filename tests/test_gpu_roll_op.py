"""The two kernels of the roll search alone (csrc/roll.hip through vitvs_op_quarter_turns and vitvs_op_roll_pick) against numpy
(GPU): ``numpy.rot90`` bit for bit, and tests/roll_ref.py's pick and carry-back, tables and integers exactly, scores to 1e-12.

The quarter-turn kernel moves 32 x 32 pixel tiles through LDS: S = 8 is one partial tile, 56 and 70 have a narrower last tile in
both directions (70 = 2 x 32 + 6), 224 is 7 x 7 whole tiles; n = 3 exercises the frame index of the grid.  The pick is one
workgroup of 256 threads: T = 16 leaves most threads without a token, 196 has a tail, 3136 gives every thread 12 or 13."""
import ctypes as C

import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib
import law_support as ls
import roll_ref as rf

pytestmark = pytest.mark.gpu


def _p(t):
    return C.c_void_p(t.data_ptr())


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("S", [8, 56, 70, 224])
def test_quarter_turns_are_rot90(S, n):
    lib = _lib.load()
    rng = np.random.default_rng(100 * S + n)
    frames = rng.integers(0, 256, size=(n, S, S, 3), dtype=np.uint8)
    dev = torch.device("cuda", torch.cuda.current_device())
    f = torch.from_numpy(frames).to(dev)
    out = torch.full((n, 4, S, S, 3), 0x5A, dtype=torch.uint8, device=dev)
    guard = torch.full((4096,), 0x5A, dtype=torch.uint8, device=dev)       # (allocated next: a stray byte would likely land here)
    torch.cuda.synchronize()
    assert lib.vitvs_op_quarter_turns(_p(f), n, S, _p(out), None) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for i in range(n):
        for k in range(4):
            assert np.array_equal(got[i, k], np.rot90(frames[i], k)), (S, n, i, k)
    assert bool((guard == 0x5A).all())
    assert np.array_equal(f.cpu().numpy(), frames)                          # the input is untouched


def test_quarter_turns_refuses_bad_arguments():
    lib = _lib.load()
    buf = torch.zeros(64, dtype=torch.uint8, device="cuda")
    assert lib.vitvs_op_quarter_turns(None, 1, 4, _p(buf), None) == -2
    assert lib.vitvs_op_quarter_turns(_p(buf), 0, 4, _p(buf), None) == -2
    assert lib.vitvs_op_quarter_turns(_p(buf), 1, 0, _p(buf), None) == -2


# ----------------------------------------------------------------------------- the pick
def _device_pick(nn1, nn2, sim1):
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    T = nn1.shape[1]
    a = torch.from_numpy(np.ascontiguousarray(nn1, dtype=np.int32)).to(dev)
    b = torch.from_numpy(np.ascontiguousarray(nn2, dtype=np.int32)).to(dev)
    s = torch.from_numpy(np.ascontiguousarray(sim1, dtype=np.float32)).to(dev)
    o1 = torch.full((T,), -7, dtype=torch.int32, device=dev)
    o2 = torch.full((T,), -7, dtype=torch.int32, device=dev)
    os_ = torch.full((T,), -7.0, dtype=torch.float32, device=dev)
    info = torch.full((8,), -7, dtype=torch.int32, device=dev)
    scores = torch.full((4,), -7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    rc = lib.vitvs_op_roll_pick(T, _p(a), _p(b), _p(s), _p(o1), _p(o2), _p(os_), _p(info), _p(scores), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return dict(nn_1=o1.cpu().numpy(), nn_2=o2.cpu().numpy(), sim_1=os_.cpu().numpy(), roll_info=info.cpu().numpy(),
                scores=scores.cpu().numpy())


def _check(nn1, nn2, sim1, what, want_roll=None):
    T = nn1.shape[1]
    g = int(round(np.sqrt(T)))
    want = rf.pick(nn1, nn2, sim1, g)
    got = _device_pick(nn1, nn2, sim1)
    assert np.array_equal(got["roll_info"], want["roll_info"]), (what, got["roll_info"], want["roll_info"])
    assert np.array_equal(np.isnan(got["scores"]), np.isnan(want["scores"])), (what, got["scores"], want["scores"])
    ok = ~np.isnan(want["scores"])
    assert np.all(np.abs(got["scores"][ok] - want["scores"][ok]) <= 1e-12 * np.abs(want["scores"][ok])), (what, got["scores"], want["scores"])
    assert np.array_equal(got["nn_1"], want["nn_1"]), (what, int(np.argmax(got["nn_1"] != want["nn_1"])))
    assert np.array_equal(got["nn_2"], want["nn_2"]), (what, int(np.argmax(got["nn_2"] != want["nn_2"])))
    assert np.array_equal(got["sim_1"].view(np.uint32), want["sim_1"].astype(np.float32).view(np.uint32)), what
    if want_roll is not None:
        assert int(got["roll_info"][0]) == want_roll, (what, got["roll_info"])
    return got


def _random_four(rng, T, boosts):
    tabs = [ls.tables(rng, T, b)[:3] for b in boosts]
    return (np.stack([t[0] for t in tabs]), np.stack([t[1] for t in tabs]), np.stack([t[2] for t in tabs]).astype(np.float32))


@pytest.mark.parametrize("T", [16, 196, 3136])
def test_pick_and_carry_back(T):
    rng = np.random.default_rng(T)
    ident = np.arange(T)
    lo, hi = max(2, T // 8), max(3, T // 3)
    nn1, nn2, sim1 = _random_four(rng, T, [lo, lo, lo, lo])
    # a clear winner at each k: its mutual matches are the most similar ones
    for k in range(4):
        s = sim1.copy()
        s[k, rf.mutual(nn1[k], nn2[k])] = np.float32(0.97)
        _check(nn1, nn2, s, ("winner", T, k), want_roll=k)
    # an exact two-way tie, identical tables in two candidates: the smaller k wins
    for a, b in ((1, 3), (0, 2), (2, 3)):
        n1, n2, s = nn1.copy(), nn2.copy(), sim1.copy()
        s[a, rf.mutual(n1[a], n2[a])] = np.float32(0.96)
        n1[b], n2[b], s[b] = n1[a], n2[a], s[a]
        got = _check(n1, n2, s, ("tie", T, a, b), want_roll=a)
        assert got["scores"][a] == got["scores"][b]
    # n_mutual of 0 and of T are not valid; a same-image candidate with n_mutual = T is
    none1, none2 = (ident + 1) % T, (ident + 2) % T
    n1, n2, s = nn1.copy(), nn2.copy(), sim1.copy()
    n1[0], n2[0] = none1, none2                                 # candidate 0: nothing mutual
    n1[2], n2[2], s[2] = ident, ident, np.full(T, 0.95, np.float32)   # candidate 2: everything mutual, not the same image
    got = _check(n1, n2, s, ("0 and T", T))
    assert got["roll_info"][1] == 0 and got["roll_info"][3] == T and np.isnan(got["scores"][[0, 2]]).all()
    assert got["roll_info"][0] in (1, 3)
    s[2] = np.float32(0.995)                                    # ... now it is: valid, and it wins
    got = _check(n1, n2, s, ("same image", T), want_roll=2)
    assert got["roll_info"][5] == 1 and not np.isnan(got["scores"][2])
    # the same-image candidate's tables come back turned: nn_1' = P_2, nn_2'[P_2] = identity
    assert np.array_equal(got["nn_1"], rf.perm(int(round(np.sqrt(T))), 2))
    # nobody valid: k* = -1, pair 0 keeps candidate 0's tables
    n1 = np.stack([none1, ident, none1, ident])
    n2 = np.stack([none2, ident, none2, ident])
    s = np.full((4, T), 0.5, np.float32)
    got = _check(n1, n2, s, ("nobody", T), want_roll=-1)
    assert np.isnan(got["scores"]).all() and np.array_equal(got["nn_1"], none1) and np.array_equal(got["nn_2"], none2)
    # entries of nn_1 outside 0 .. T - 1 are never mutual and pass through the carry-back as they are
    n1, n2, s = nn1.copy(), nn2.copy(), sim1.copy()
    for k in range(4):
        where = rng.choice(T, size=max(1, T // 10), replace=False)
        n1[k, where] = rng.choice([-1, -5, T, T + 3, 2 ** 31 - 1, -2 ** 31], size=where.size)
    s[3, rf.mutual(n1[3], n2[3])] = np.float32(0.97)
    got = _check(n1, n2, s, ("out of range", T), want_roll=3)
    wild = (n1[3] < 0) | (n1[3] >= T)
    assert wild.any() and np.array_equal(got["nn_1"][wild], n1[3][wild])


def test_pick_refuses_bad_arguments():
    lib = _lib.load()
    buf = torch.zeros(4 * 200, dtype=torch.int32, device="cuda")
    d = torch.zeros(4, dtype=torch.float64, device="cuda")
    args = (_p(buf), _p(buf), _p(buf), _p(buf), _p(buf), _p(buf), _p(buf), _p(d), None)
    assert lib.vitvs_op_roll_pick(200, *args) == -2             # not a square grid
    assert lib.vitvs_op_roll_pick(0, *args) == -2
    assert lib.vitvs_op_roll_pick(196, None, *args[1:]) == -1
