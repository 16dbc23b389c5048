"""The GEMMs' tile, K-slice and XCD routing, exactly (GPU).

Every linear test on randn data holds max|got - ref| / max|ref| over the whole matrix to a bar; in bf16 (1.5e-2) a term dropped
or doubled at a few elements - one k-tile of one wave's sub-tile, one row of a last tile, one tile walked twice - stays under
it.  The operands of tests/gemm_exact_ref.py are small integers, so that fp32, bf16, fp16 and f16x2 all compute the product
exactly and every element is compared with == (tests/test_gemm_exact_host.py proves on the fp64 reference alone that each such
fault changes every tile it touches).  Each case first asserts, through vitvs_op_linear_plan under its in-flight hint and through
vitvs_op_linear_big_grid, that the library launches what the case declares; then runs vitvs_op_linear, vitvs_op_linear_variant
or vitvs_op_linear_partial into the middle of a NaN buffer - guard rows in front and behind, one K slice more than the launch
owns - and, where vitvs_op_residual_ln has the width, sums the slices into x.  The guards and the extra slice stay NaN, every
output is finite, got == ref everywhere (f16x2: hi + lo == ref).  A miss reports the count and the first few elements with their
tile, wave and 16-row block.  The row sweeps run every M of a (tile, precision, epilogue) inside one test.
"""
import pytest
import torch

import vitvs_amd  # noqa: F401
from op_support import gpu_lib as lib  # noqa: F401
from op_support import ptr, stream

import gemm_exact_ref as ge

pytestmark = pytest.mark.gpu

GUARD = 3                      # rows in front of and behind every output that no launch may write
ON_DEVICE = 1 << 28            # M N K from which operands and the fp64 reference are made on the device


class Operands:
    """A case's operands on the device and its fp64 references"""

    def __init__(self, c):
        dev = "cuda" if c.M * c.N * c.K >= ON_DEVICE else "cpu"
        s = max(c.slices, 1)
        A, W = ge.make_a(c.M, c.K, c.dens, dev), ge.make_w(c.N, c.K, dev)
        bias, ls = ge.make_cols(c.N, dev)
        self.part = ge.reference(A, W, s).cuda()                  # [slices, M, N]
        self.bias, self.ls = bias.cuda(), ls.cuda()
        self.store = self.part[0] + self.bias.double()
        self.A, self.W = ge.pack(c.prec, A).cuda(), ge.pack(c.prec, W).cuda()


def _values(prec, out):
    if prec == ge.F16X2:
        hi, lo = ge.from_x2(out)
        return hi + lo
    return out.double()


def _launch(lib, c, ops, M):
    """One launch of the case on the first M rows of its A, under its hint, into a NaN buffer.  Returns (rc, buffer, view of the
    rows the launch owns: [M, N] in the output layout, or fp32 [slices, M, N])."""
    s = max(c.slices, 1)
    if c.epi == ge.STORE:
        width = 2 * c.N if c.prec == ge.F16X2 else c.N
        buf = torch.full((GUARD + M + GUARD, width), float("nan"), dtype=ge.DTYPES[c.prec], device="cuda")
        own = buf[GUARD:GUARD + M]
    else:
        buf = torch.full((GUARD + (s + 1) * M + GUARD, c.N), float("nan"), dtype=torch.float32, device="cuda")
        own = buf[GUARD:GUARD + s * M].view(s, M, c.N)
    dst = ptr(buf, GUARD * buf.shape[1] * buf.element_size())
    prev_hint, prev_exp = lib.vitvs_op_plan_in_flight(c.hint), lib.vitvs_op_weight_exponent(0)
    try:
        if c.variant:
            rc = lib.vitvs_op_linear_variant(c.prec, c.variant, ptr(ops.A), ptr(ops.W), ptr(ops.bias), dst, M, c.N, c.K, 0,
                                             c.slices if c.epi == ge.PARTIAL else 0, stream())
        elif c.epi == ge.STORE:
            rc = lib.vitvs_op_linear(c.prec, ptr(ops.A), ptr(ops.W), ptr(ops.bias), dst, M, c.N, c.K, 0, stream())
        else:
            rc = lib.vitvs_op_linear_partial(c.prec, ptr(ops.A), ptr(ops.W), dst, M, c.N, c.K, c.slices, stream())
    finally:
        lib.vitvs_op_plan_in_flight(prev_hint)
        lib.vitvs_op_weight_exponent(prev_exp)
    return rc, buf, own


def _check(c, ops, M, buf, own):
    who = f"{ge.case_id(c)} M {M}"
    rest = torch.cat([buf[:GUARD].flatten(), buf[GUARD + own.numel() // buf.shape[1]:].flatten()])
    assert bool(torch.isnan(rest.float()).all()), f"{who}: the guard rows or the slice past the launch's were written"
    if c.epi == ge.STORE:
        got = _values(c.prec, own)
        assert bool(torch.isfinite(got).all()), f"{who}: {int((~torch.isfinite(got)).sum())} outputs are not finite"
        ref = ops.store[:M]
        assert torch.equal(got, ref), ge.describe_mismatch(c, got, ref, f"M {M}")
    else:
        assert bool(torch.isfinite(own).all()), f"{who}: {int((~torch.isfinite(own)).sum())} partial sums are not finite"
        for z in range(own.shape[0]):
            ref = ops.part[z, :M]
            assert torch.equal(own[z].double(), ref), ge.describe_mismatch(c, own[z].double(), ref, f"M {M} slice {z}")


def _residual(lib, c, ops, own):
    """x += ls * (sum_z part[z] + bias) over the launch's slices: exact as well"""
    M, s = c.M, max(c.slices, 1)
    x0 = ge.make_x0(M, c.N, "cuda")
    x = torch.full((GUARD + M + GUARD, c.N), float("nan"), dtype=torch.float32, device="cuda")
    x[GUARD:GUARD + M] = x0
    rc = lib.vitvs_op_residual_ln(c.prec, ptr(x, GUARD * c.N * 4), ptr(own), s, ptr(ops.bias), ptr(ops.ls), None, None, None, M, c.N,
                                  1e-6, stream())
    assert rc == 0, f"{ge.case_id(c)}: vitvs_op_residual_ln returned {rc}"
    torch.cuda.synchronize()
    assert bool(torch.isnan(x[:GUARD]).all()) and bool(torch.isnan(x[GUARD + M:]).all()), f"{ge.case_id(c)}: x guard rows were written"
    got = x[GUARD:GUARD + M].double()
    ref = x0.double() + ops.ls.double() * (ops.part.sum(0) + ops.bias.double())
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, ref), ge.describe_mismatch(c, got, ref, "x after residual_ln")


@pytest.mark.parametrize("case", [pytest.param(c, id=ge.case_id(c)) for c in ge.CASES])
def test_case_is_exact(lib, case):
    c = case
    ge.assert_plan(lib, c)
    ops = Operands(c)
    rc, buf, own = _launch(lib, c, ops, c.M)
    assert rc == 0, f"{ge.case_id(c)}: the launch returned {rc}"
    torch.cuda.synchronize()
    _check(c, ops, c.M, buf, own)
    if c.epi == ge.PARTIAL and c.N in ge.RLN_WIDTHS and c.slices <= 8:
        _residual(lib, c, ops, own)


@pytest.mark.parametrize("sweep", [pytest.param(s, id=s.name) for s in ge.SWEEPS])
def test_row_edges_are_exact(lib, sweep):
    """every M of the sweep on the first M rows of one A per width: M - 1 is then a different row each time"""
    cases = list(ge.sweep_cases(sweep))
    ops = {}
    for c in cases:
        ge.assert_plan(lib, c)
        if c.N not in ops:
            ops[c.N] = Operands(c._replace(M=max(k.M for k in cases if k.N == c.N)))
        rc, buf, own = _launch(lib, c, ops[c.N], c.M)
        assert rc == 0, f"{ge.case_id(c)}: the launch returned {rc}"
        torch.cuda.synchronize()
        _check(c, ops[c.N], c.M, buf, own)


@pytest.mark.parametrize("case", [pytest.param(c, id=ge.case_id(c)) for c in ge.REFUSED])
def test_256_k_tiles_per_slice_are_refused_and_nothing_is_written(lib, case):
    ops = Operands(case)
    rc, buf, _ = _launch(lib, case, ops, case.M)
    torch.cuda.synchronize()
    assert rc != 0, f"{ge.case_id(case)}: 256 k-tiles per slice do not fit the launch arguments, yet the call returned 0"
    assert bool(torch.isnan(buf.float()).all()), f"{ge.case_id(case)}: a refused call wrote to its output"
