"""The robust rig law's host side: its symbols, its launch plan (vitvs_op_rig_robust_plan: host arithmetic,
checked against a restatement of the formula) and the Python arguments that are refused before any device call.  No GPU call."""
import ctypes as C

import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib, config, dist
from vitvs_amd.engine import Engine

TILE = 384                  # stacked rows the last arriver keeps in LDS: 8 cameras x 48 rows
LDS_CAP = 160 * 1024


def _plan(n_cams, ld):
    """dynamic LDS in doubles: Gs 256 + 4 (ticket word, counts) | the stack's copy [7][TILE] when resident | rho, w [pairs]"""
    resident = n_cams * ld <= TILE
    pairs = n_cams * (ld // 2)
    lds = 8 * (260 + (7 * TILE if resident else 0) + 2 * pairs)
    return lds, int(resident), pairs, int(lds > 64 * 1024)


def _call(n_cams, ld):
    out = (C.c_int32 * 4)(-1, -1, -1, -1)
    return _lib.load().vitvs_op_rig_robust_plan(n_cams, ld, out), tuple(out)


def test_the_new_symbols_load():
    lib = _lib.load()
    for name in ("vitvs_rig_robust_velocity_dev", "vitvs_rig_robust_velocity", "vitvs_op_rig_robust_law",
                 "vitvs_op_rig_robust_scratch_bytes", "vitvs_op_rig_robust_plan"):
        assert name in _lib.PROTOTYPES and getattr(lib, name) is not None, name


@pytest.mark.parametrize("shape", [(1, 2), (3, 32), (8, 48), (8, 96), (9, 260), (2, 2048), (2, 8192)])
def test_plan_equals_its_formula(shape):
    rc, out = _call(*shape)
    assert rc == 0 and out == _plan(*shape), (shape, rc, out, _plan(*shape))


def test_the_stack_is_lds_resident_up_to_the_tile():
    for shape, resident in (((8, 48), 1), ((1, 384), 1), ((1, 385), 0), ((8, 49), 0), ((8, 50), 0), ((4, 96), 1), ((5, 77), 0)):
        rc, out = _call(*shape)
        assert rc == 0 and out[1] == resident and out == _plan(*shape), (shape, out)


def test_plan_takes_4096_pairs_and_refuses_past_160_kib():
    rc, out = _call(2, 4096)                                   # 4096 pairs
    assert rc == 0 and out[2] == 4096 and out[0] <= LDS_CAP
    # the largest pair count that fits: 8 (260 + 2 pairs) <= 160 KiB
    most = (LDS_CAP // 8 - 260) // 2
    assert _call(1, 2 * most) == (0, _plan(1, 2 * most)) and _plan(1, 2 * most)[0] <= LDS_CAP
    rc, out = _call(1, 2 * (most + 1))
    assert rc == -3 and out == _plan(1, 2 * (most + 1)) and out[0] > LDS_CAP
    assert _call(4, 8192)[0] == -3 and _call(256, 96)[0] == -3


def test_plan_refuses_bad_shapes():
    lib = _lib.load()
    for n_cams, ld in ((0, 48), (-1, 48), (257, 48), (3, 0), (3, -4)):
        assert _call(n_cams, ld)[0] == -2, (n_cams, ld)
        assert lib.vitvs_op_rig_robust_scratch_bytes(n_cams, ld) == -2
    assert lib.vitvs_op_rig_robust_plan(3, 48, None) == -1
    # the scratch block: the plain law's and a third [7][n ld] block of doubles
    for n_cams, ld in ((1, 2), (3, 32), (9, 260)):
        assert lib.vitvs_op_rig_robust_scratch_bytes(n_cams, ld) == lib.vitvs_op_rig_scratch_bytes(n_cams, ld) + 8 * 7 * n_cams * ld


def test_servo_params_range_check():
    assert config.ServoParams().rig_robust_iterations == 0
    assert config.ServoParams(rig_robust_iterations=16).rig_robust_iterations == 16
    for bad in (-1, 17):
        with pytest.raises(ValueError):
            config.ServoParams(rig_robust_iterations=bad)


def test_the_distributed_rig_law_refuses_the_robust_form():
    with pytest.raises(ValueError, match="robust"):
        dist.rig_velocity(torch.zeros(28, dtype=torch.float64), 0.35, robust_iterations=4)


def test_engine_rig_velocity_checks_its_robust_arguments_before_the_device():
    eng = Engine.__new__(Engine)                               # no handle, no device: the checks come first
    W, st = np.tile(np.eye(6), (3, 1, 1)), np.zeros(3, np.int32)
    for call in (eng.rig_velocity, eng.rig_velocity_host):
        with pytest.raises(ValueError, match="needs K"):
            call(W, st, robust_iterations=4)
        with pytest.raises(ValueError, match="0 .. 16"):
            call(W, st, robust_iterations=17, K=(600.0, 600.0, 320.0, 240.0))
        with pytest.raises(ValueError, match="per camera"):
            call(W, st, robust_iterations=4, K=np.ones((2, 4)))
    assert Engine._rig_robust_arguments(3, 0, None) is None
    assert Engine._rig_robust_arguments(3, 2, (1.0, 2.0, 3.0, 4.0)).shape == (3, 4)
