"""What the pointer-level operator tests share (tests/test_gpu_ops*.py, the *_cover.py and *_exact.py GPU tests, and the host
tests of the same plans): the two ``lib`` fixtures, raw pointers and the current stream for the C ABI, random operands, the
hi / lo layout of the f16x2 precision and the fp64 attention every attention test compares with.

A test module imports the fixture it needs under the name ``lib`` (``from op_support import gpu_lib as lib``): a module-scoped
fixture is set up once per module that asks for it, wherever it is defined."""
import ctypes as C
import importlib.util
import math
import os

import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = {_lib.F32: torch.float32, _lib.BF16: torch.bfloat16, _lib.F16: torch.float16, _lib.F16X2: torch.float16}


@pytest.fixture(scope="module")
def gpu_lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return _lib.load()


@pytest.fixture(scope="module")
def host_lib():
    if not os.path.isfile(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


@pytest.fixture(scope="module")
def plan_cover():
    """tools/plan_cover.py as a module (the host tests import it under the name ``cover``)."""
    spec = importlib.util.spec_from_file_location("plan_cover", os.path.join(ROOT, "tools", "plan_cover.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def ptr(t, offset=0):
    return None if t is None else C.c_void_p(t.data_ptr() + offset)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def mk(shape, gen, scale=1.0):
    return (torch.randn(shape, generator=gen) * scale).float()


def nan_like(prec, rows, cols):
    """NaN rows of `cols` logical columns in the precision's output layout"""
    return torch.full((rows, 2 * cols if prec == _lib.F16X2 else cols), float("nan"), dtype=DTYPES[prec], device="cuda")


def rel_max(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def to_x2(t, exp=0):
    """fp32 [R, C] -> fp16 [R, 2C]: per 32 columns [hi | lo] of t * 2^exp."""
    r, c = t.shape
    ts = t.float() * (2.0 ** exp)
    hi = ts.clamp(-65504, 65504).half()
    lo = (ts - hi.float()).half()
    return torch.stack([hi.view(r, c // 32, 32), lo.view(r, c // 32, 32)], dim=2).reshape(r, 2 * c).contiguous()


def from_x2(t):
    """fp16 [R, 2C] -> the fp64 values hi + lo [R, C]."""
    r, c2 = t.shape
    v = t.reshape(r, c2 // 64, 2, 32).double()
    return (v[:, :, 0] + v[:, :, 1]).reshape(r, c2 // 2)


def values(prec, out):
    return from_x2(out) if prec == _lib.F16X2 else out.double()


def weight_exp(w):
    m = float(w.abs().max())
    return max(0, min(31, 13 - math.frexp(m)[1])) if m > 0 else 0


def attention_ref(qkv, n_img, N, H):
    D = H * 64
    q, k, v = qkv.double().reshape(n_img, N, 3, H, 64).unbind(2)
    q, k, v = (t.transpose(1, 2) for t in (q, k, v))
    att = ((q @ k.transpose(-2, -1)) * 0.125).softmax(-1)
    return (att @ v).transpose(1, 2).reshape(n_img * N, D)
