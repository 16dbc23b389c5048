"""Selection mode BEST's kernel alone (csrc/select.hip through vitvs_op_best_order_dev: tables in, visiting order out) against
its numpy statement, tests/select_ref.py, element for element (GPU).

The kernel sorts 64-bit keys in LDS, one workgroup per pair: by rank counting with one token per thread up to T = 256 (T = 16:
one wave, cells > g; 196: tail threads without a token; 256: none), by a bitonic network on the next power of two of T beyond
(289 and 484: one pair of keys per thread, g not a multiple of the cells; 1024; 3136, the largest grid of the configs: 1024 threads
over two pairs of keys each, most of the last quarter padding)."""
import ctypes as C

import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib
import select_ref as sref
import law_support as ls

pytestmark = pytest.mark.gpu


def _device_order(tables, cells):
    """vitvs_op_best_order_dev on a list of (nn_1, nn_2, sim_1), one launch: int32 [pairs, T]."""
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    n, t = len(tables), len(tables[0][0])
    nn1 = torch.from_numpy(np.stack([np.asarray(x[0]) for x in tables]).astype(np.int32)).to(dev)
    nn2 = torch.from_numpy(np.stack([np.asarray(x[1]) for x in tables]).astype(np.int32)).to(dev)
    sim = torch.from_numpy(np.stack([np.asarray(x[2], np.float32) for x in tables])).to(dev)
    out = torch.full((n, t), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    p = lambda a: C.c_void_p(a.data_ptr())  # noqa: E731
    rc = lib.vitvs_op_best_order_dev(t, cells, n, p(nn1), p(nn2), p(sim), p(out), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check(tables, cells, what):
    got = _device_order(tables, cells)
    for b, (nn1, nn2, sim) in enumerate(tables):
        want = sref.best_order(nn1, nn2, sim, cells)
        assert np.array_equal(got[b], want), (what, b, int(np.argmax(got[b] != want)))


@pytest.mark.parametrize("cells", [1, 2, 4, 16])
@pytest.mark.parametrize("T", [16, 196, 256, 289, 484, 1024, 3136])
def test_order_on_random_tables(T, cells):
    rng = np.random.default_rng(10 * T + cells)
    _check([ls.tables(rng, T, int(rng.integers(T // 4, T // 2)))[:3]], cells, (T, cells))


def test_three_pairs_in_one_launch():
    rng = np.random.default_rng(77)
    tables = [ls.tables(rng, 289, n)[:3] for n in (40, 150, 250)]
    _check(tables, 4, "three pairs")
    got = _device_order(tables, 4)
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[1], got[2])


@pytest.mark.parametrize("T", [196, 484])
def test_degenerate_tables(T):
    rng = np.random.default_rng(T)
    ident = np.arange(T)
    sim = rng.uniform(0.2, 0.9, T).astype(np.float32)
    nn1, nn2, sim_r, _ = ls.tables(rng, T, T // 3)
    flat = np.full(T, 0.5, np.float32)
    ties = sim_r.copy()
    ties[rng.choice(T, size=50, replace=False)] = np.float32(0.625)      # 50 exact ties, mutual and not, across cells
    zeros = sim_r.copy()
    zeros[::3] = 0.0
    zeros[1::3] = -0.0                                                   # +0 and -0 are one value: the id decides
    wild = nn1.copy()
    wild[rng.choice(T, size=40, replace=False)] = rng.choice([-1, -5, T, T + 3, 2 ** 31 - 1, -2 ** 31], size=40)
    cases = {"every token mutual": (ident, ident, sim), "no token mutual": ((ident + 1) % T, (ident + 2) % T, sim),
             "all similarities equal": (nn1, nn2, flat), "50 exact ties": (nn1, nn2, ties), "signed zeros": (nn1, nn2, zeros),
             "nn_1 out of range": (wild, nn2, sim_r)}
    for cells in (1, 4):
        for what, tab in cases.items():
            _check([tab], cells, (what, T, cells))
    # all similarities equal and nothing mutual: pure id order within the cells
    got = _device_order([((ident + 1) % T, (ident + 2) % T, flat)], 1)[0]
    assert np.array_equal(got, ident)
    # the out-of-range entries are class 1
    m = sref.mutual_mask(wild, nn2)
    got = _device_order([(wild, nn2, sim_r)], 4)[0]
    assert not m[got[int(m.sum()):]].any() and m[got[:int(m.sum())]].all()


def test_refusals_without_a_launch():
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    t = 129 * 129                                                        # 2^15 keys of 8 bytes: 256 KiB of LDS
    buf = torch.zeros(t, dtype=torch.int32, device=dev)
    out = torch.full((t,), -7, dtype=torch.int32, device=dev)
    p = lambda a: C.c_void_p(a.data_ptr())  # noqa: E731
    assert lib.vitvs_op_best_order_dev(t, 4, 1, p(buf), p(buf), p(buf), p(out), None) == -3
    assert lib.vitvs_op_best_order_dev(200, 4, 1, p(buf), p(buf), p(buf), p(out), None) == -2      # not a square grid
    for cells in (0, 17):
        assert lib.vitvs_op_best_order_dev(196, cells, 1, p(buf), p(buf), p(buf), p(out), None) == -2
    assert lib.vitvs_op_best_order_dev(196, 4, 1, None, p(buf), p(buf), p(out), None) == -1
    torch.cuda.synchronize()
    assert bool((out == -7).all())                                       # nothing ran
    # the largest grid that fits: 128 x 128 tokens, 2^14 keys, 132 KiB (the opt-in beyond 64 KiB)
    t = 128 * 128
    rng = np.random.default_rng(3)
    nn1 = rng.integers(0, t, t)
    nn2 = rng.integers(0, t, t)
    nn2[nn1[: t // 2]] = np.arange(t // 2)
    _check([(nn1, nn2, rng.uniform(0.1, 0.9, t).astype(np.float32))], 16, "128 x 128")
