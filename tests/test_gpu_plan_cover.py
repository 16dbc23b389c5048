"""Every launch plan the forward can make, against fp64 (GPU).

tests/golden/plan_cover.json (tools/plan_cover.py) holds one representative product shape per reachable plan key: for a
linear layer (precision, epilogue, tile family, tile, k-groups, ring stages, one or several K slices, XCD map), for attention
(precision, kernel, divided, key ranges, last range short).  Each row becomes one case here, run under the row's in-flight
hint after the plan hook has confirmed that the hook launches the row's key.  Operands are rounded once to the precision (the
f16x2 hi / lo layout with the weight exponent a handle would give the weights), and the reference is an fp64 statement of the
operator on those rounded values.  Outputs start as NaN with guard rows behind them.

Bars are the op tests' (tests/test_gpu_ops.py, tests/test_gpu_ops_x2.py) for the same precision and operator; each case
records its worst relative error (max |got - ref| / max |ref|) as a junit property
(`--junitxml=FILE -o junit_family=legacy`)."""
import ctypes as C
import json
import os

import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib
from op_support import gpu_lib as lib  # noqa: F401
from op_support import DTYPES, attention_ref, from_x2, nan_like, ptr, rel_max, stream, to_x2, values, weight_exp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "plan_cover.json")) as _fh:
    ROWS = json.load(_fh)["rows"]

STORE, PARTIAL = 0, 1
GUARD = 3                 # rows behind every output that no launch may write
LOG2E = 1.4426950408889634
# (the op tests' bars)  store: test_linear; slice / x / LayerNorm: test_split_k_pair; attention: test_attention (forward form)
BAR_STORE = {_lib.F32: 2e-5, _lib.BF16: 1.5e-2, _lib.F16: 2e-3, _lib.F16X2: 2e-5}
BAR_SLICE = {_lib.F32: 2e-5, _lib.BF16: 1e-3, _lib.F16: 1e-3, _lib.F16X2: 2e-5}
BAR_X = {_lib.F32: 2e-5, _lib.BF16: 2e-6 + 1e-3, _lib.F16: 2e-6 + 1e-3, _lib.F16X2: 2e-5}
BAR_LN = {_lib.F32: 2e-5, _lib.BF16: 1e-2, _lib.F16: 2e-3, _lib.F16X2: 2e-5}
BAR_ATTN = {_lib.F32: 1e-5, _lib.BF16: 2e-2, _lib.F16: 3e-3, _lib.F16X2: 1e-5}


def _mk(shape, gen, scale=1.0):
    return (torch.randn(shape, generator=gen) * scale).float().cuda()


# the f16x2 layout (csrc/common.h; the same helpers as tests/test_gpu_ops_x2.py)


def _operand(prec, t, exp=0):
    """(what the kernel is given, the fp64 values it represents)"""
    if prec == _lib.F16X2:
        x = to_x2(t, exp)
        return x, from_x2(x) / (2.0 ** exp)
    x = t.to(DTYPES[prec]).contiguous()
    return x, x.double()


@pytest.fixture
def hint(lib):
    """Runs a case under its row's in-flight hint; the hint and the weight exponent are restored whatever happens."""
    prev = lib.vitvs_op_plan_in_flight(1)
    yield lambda n: lib.vitvs_op_plan_in_flight(n)
    lib.vitvs_op_plan_in_flight(prev)
    lib.vitvs_op_weight_exponent(0)


def _check(record, what, err, bar, row):
    record(what, f"{err:.3e}")
    assert err <= bar, f"{row['id']} ({row['model']} {row['size']}/{row['stride']} x{row['frames']} {row['layer']}): " \
                       f"{what} worst relative error {err:.3e} > {bar:g}"


def _linear_plan(lib, row):
    out = (C.c_int32 * 7)()
    prec, epi = row["key"][0], row["key"][1]
    rc = lib.vitvs_op_linear_plan(prec, epi, row["M"], row["N"], row["K"], row["slices"] if epi == PARTIAL else 0, out)
    big, rows, cols, kg, stages, slices, xcd = list(out)
    return rc, [prec, epi, big, rows, cols, kg, stages, int(slices > 1), xcd], slices


def _attention_plan(lib, row):
    out = (C.c_int32 * 6)()
    prec = row["key"][0]
    rc = lib.vitvs_op_attention_plan(prec, row["n_img"], row["N"], row["H"], out)
    nt = (row["N"] + 63) // 64
    per = out[4]
    ranges = -(-nt // per) if per else 1
    return rc, [prec, out[0], out[5], ranges, int(ranges > 1 and nt % per != 0)]


def _run_store(lib, row, record):
    prec, M, N, K = row["key"][0], row["M"], row["N"], row["K"]
    g = torch.Generator().manual_seed(M * 7 + N + K)
    A32, W32, bias = _mk((M, K), g), _mk((N, K), g, K ** -0.5), _mk((N,), g, 0.1)
    e = weight_exp(W32) if prec == _lib.F16X2 else 0
    A, Ar = _operand(prec, A32)
    W, Wr = _operand(prec, W32, e)
    lin = Ar @ Wr.t() + bias.double()
    for gelu in row["gelu"]:
        ref = torch.nn.functional.gelu(lin) if gelu else lin
        out = nan_like(prec, M + GUARD, N)
        lib.vitvs_op_weight_exponent(e)
        rc = lib.vitvs_op_linear(prec, ptr(A), ptr(W), ptr(bias), ptr(out), M, N, K, gelu, stream())
        lib.vitvs_op_weight_exponent(0)
        assert rc == 0
        torch.cuda.synchronize()
        assert torch.isnan(out[M:].float()).all(), f"{row['id']}: rows beyond M were written"
        got = values(prec, out[:M])
        assert torch.isfinite(got).all(), f"{row['id']}: non-finite outputs"
        _check(record, f"store_gelu{gelu}", rel_max(got, ref), BAR_STORE[prec], row)


def _run_partial(lib, row, record):
    prec, M, D, K, slices = row["key"][0], row["M"], row["N"], row["K"], row["slices"]
    g = torch.Generator().manual_seed(M + D * 3 + K)
    A32, W32 = _mk((M, K), g), _mk((D, K), g, K ** -0.5)
    bias, ls = _mk((D,), g, 0.1), 1.0 + 0.3 * _mk((D,), g)
    gamma, beta = 1.0 + 0.1 * _mk((D,), g), 0.1 * _mk((D,), g)
    x0 = _mk((M, D), g)
    e = weight_exp(W32) if prec == _lib.F16X2 else 0
    A, Ar = _operand(prec, A32)
    W, Wr = _operand(prec, W32, e)
    # one slice more than the launch owns: it must stay NaN, as must every row past M of the last one
    part = torch.full((slices + 1, M, D), float("nan"), dtype=torch.float32, device="cuda")
    lib.vitvs_op_weight_exponent(e)
    rc = lib.vitvs_op_linear_partial(prec, ptr(A), ptr(W), ptr(part), M, D, K, slices, stream())
    lib.vitvs_op_weight_exponent(0)
    assert rc == 0
    x = torch.cat([x0, torch.full((GUARD, D), float("nan"), device="cuda")]).contiguous()
    out = nan_like(prec, M + GUARD, D)
    assert lib.vitvs_op_residual_ln(prec, ptr(x), ptr(part), slices, ptr(bias), ptr(ls), ptr(gamma), ptr(beta), ptr(out), M, D, 1e-6,
                                    stream()) == 0
    torch.cuda.synchronize()
    assert torch.isnan(part[slices]).all(), f"{row['id']}: the slice past the launch's {slices} was written"
    assert torch.isfinite(part[:slices]).all(), f"{row['id']}: non-finite partial sums"
    ks = K // slices
    for z in range(slices):            # each slice holds the products of ITS K range, whichever workgroup computed it
        ref_z = Ar[:, z * ks:(z + 1) * ks] @ Wr[:, z * ks:(z + 1) * ks].t()
        _check(record, f"slice{z}", rel_max(part[z], ref_z), BAR_SLICE[prec], row)
    x_ref = x0.double() + ls.double() * (Ar @ Wr.t() + bias.double())
    y_ref = torch.nn.functional.layer_norm(x_ref, (D,), gamma.double(), beta.double(), 1e-6)
    assert torch.isnan(x[M:]).all() and torch.isnan(out[M:].float()).all(), f"{row['id']}: rows beyond M were written"
    got_y = values(prec, out[:M])
    assert torch.isfinite(x[:M]).all() and torch.isfinite(got_y).all(), f"{row['id']}: non-finite outputs"
    _check(record, "x", rel_max(x[:M], x_ref), BAR_X[prec], row)
    _check(record, "layernorm", rel_max(got_y, y_ref), BAR_LN[prec], row)


def _run_attention(lib, row, record):
    prec, n_img, N, H = row["key"][0], row["n_img"], row["N"], row["H"]
    D = H * 64
    g = torch.Generator().manual_seed(N * 3 + H + n_img)
    qkv32 = _mk((n_img * N, 3 * D), g)
    out = nan_like(prec, n_img * N + GUARD, D)
    if prec in (_lib.BF16, _lib.F16):
        # the forward's form: q carries 0.125 * log2(e), applied in fp32 before the one rounding to 16 bits
        qkv32[:, :D] *= 0.125 * LOG2E
        qkv, t = _operand(prec, qkv32)
        t = t.clone()
        t[:, :D] /= 0.125 * LOG2E
        rc = lib.vitvs_op_attention_q(prec, ptr(qkv), ptr(out), n_img, N, H, 1, stream())
    else:
        qkv, t = _operand(prec, qkv32)
        rc = lib.vitvs_op_attention(prec, ptr(qkv), ptr(out), n_img, N, H, stream())
    assert rc == 0
    ref = attention_ref(t, n_img, N, H)
    torch.cuda.synchronize()
    assert torch.isnan(out[n_img * N:].float()).all(), f"{row['id']}: rows beyond the last token were written"
    got = values(prec, out[:n_img * N])
    assert torch.isfinite(got).all(), f"{row['id']}: non-finite outputs"
    _check(record, "attention", rel_max(got, ref), BAR_ATTN[prec], row)


@pytest.mark.parametrize("row", [pytest.param(r, id=r["id"]) for r in ROWS])
def test_plan_against_fp64(lib, hint, record_property, row):
    hint(row["hint"])
    if row["kind"] == "linear":
        rc, key, slices = _linear_plan(lib, row)
        assert rc == 0 and key == row["key"] and slices == row["slices"], \
            f"{row['id']}: the hook plans {key} x {slices} slices here, not the row's key (run tools/plan_cover.py)"
        (_run_store if row["key"][1] == STORE else _run_partial)(lib, row, record_property)
    else:
        rc, key = _attention_plan(lib, row)
        assert rc == 0 and key == row["key"], f"{row['id']}: the hook plans {key} here, not the row's key"
        _run_attention(lib, row, record_property)
