"""The linear layers' GELU epilogue and the hi / lo cross terms of f16x2, per element (GPU).

The linear tests on randn data hold max |got - ref| / max |ref| to a bar per matrix: 1.5e-2 (bf16) and 2e-3 (fp16) leave room for
a tanh-form GELU, a coefficient of the fast erf wrong in its fourth digit or an activation dropped on a few rows, and f16x2's
2e-5 is about what one hi.lo term dropped in one 32-k tile moves an output.  The exact tests of tests/test_gpu_gemm_exact.py use
integer operands: no activation, and low halves that are all zero.  tests/epilogue_exact_ref.py makes operands for which

  GELU         the pre-activation z = A W^T + bias is the same exact fp32 number in every precision and summation order, so the
               output is compared per element with 0.5 z (1 + erf(z / sqrt 2)) in fp64: one rounding to the output type plus 8 x
               the implied erf error of the type's own form restated in fp32 (measured on the CPU, er.MEASURED_E), and for bf16
               and fp16 on z in [-3, 8] the output is the reference rounded to the type or its neighbour, neighbours at most 2 %
               (below -3 the factor 1 + erf cancels in fp32 in either form: only the absolute bar applies there)
  cross terms  both halves of every operand are non-zero and hi.hi + hi.lo + lo.hi is exact in fp32 in any order: hi + lo of the
               output == the fp64 statement of the mode, store and partial sums, and x after vitvs_op_residual_ln

(tests/test_epilogue_exact_host.py proves on the references alone that the faults in question would be seen.)  Each case first
asserts the plan it declares, then launches into the middle of a NaN buffer - guard rows in front and behind, one K slice more
than the launch owns - which must stay NaN while every owned element is finite.  f16x2 runs with weight exponent 0 and with
the exponent a handle would give these weights.  The last test puts vitvs_op_residual_ln on both sides of its store-policy
switch (M <= 2048) on the stress rows of tests/test_gpu_ends_cover.py.
"""
import pytest
import torch

import vitvs_amd  # noqa: F401
from op_support import gpu_lib as lib  # noqa: F401
from op_support import nan_like, ptr, stream

import epilogue_exact_ref as er
import gemm_exact_ref as ge
import test_gpu_ends_cover as ec

pytestmark = pytest.mark.gpu

GUARD = er.GUARD


def _launch(lib, c, A, W, bias, gelu, e):
    """One launch of the case under its hint and weight exponent e into a NaN buffer.  Returns (rc, buffer, view of what the
    launch owns: [M, N] in the output layout, or fp32 [slices, M, N])."""
    s = max(c.slices, 1)
    if c.epi == ge.STORE:
        width = 2 * c.N if c.prec == ge.F16X2 else c.N
        buf = torch.full((GUARD + c.M + GUARD, width), float("nan"), dtype=ge.DTYPES[c.prec], device="cuda")
        own = buf[GUARD:GUARD + c.M]
    else:
        buf = torch.full((GUARD + (s + 1) * c.M + GUARD, c.N), float("nan"), dtype=torch.float32, device="cuda")
        own = buf[GUARD:GUARD + s * c.M].view(s, c.M, c.N)
    dst = ptr(buf, GUARD * buf.shape[1] * buf.element_size())
    prev_hint, prev_exp = lib.vitvs_op_plan_in_flight(c.hint), lib.vitvs_op_weight_exponent(e)
    try:
        if c.variant:
            rc = lib.vitvs_op_linear_variant(c.prec, c.variant, ptr(A), ptr(W), ptr(bias), dst, c.M, c.N, c.K, gelu,
                                             c.slices if c.epi == ge.PARTIAL else 0, stream())
        elif c.epi == ge.STORE:
            rc = lib.vitvs_op_linear(c.prec, ptr(A), ptr(W), ptr(bias), dst, c.M, c.N, c.K, gelu, stream())
        else:
            rc = lib.vitvs_op_linear_partial(c.prec, ptr(A), ptr(W), dst, c.M, c.N, c.K, c.slices, stream())
    finally:
        lib.vitvs_op_plan_in_flight(prev_hint)
        lib.vitvs_op_weight_exponent(prev_exp)
    torch.cuda.synchronize()
    return rc, buf, own


def _owned(who, rc, buf, own):
    """the launch's own elements on the host, after the guards and the finiteness have been checked"""
    assert rc == 0, f"{who}: the launch returned {rc}"
    rest = torch.cat([buf[:GUARD].flatten(), buf[GUARD + own.numel() // buf.shape[1]:].flatten()])
    assert bool(torch.isnan(rest.float()).all()), f"{who}: the guard rows or the slice past the launch's were written"
    assert bool(torch.isfinite(own.float()).all()), f"{who}: {int((~torch.isfinite(own.float())).sum())} outputs are not finite"
    return own.cpu()


@pytest.mark.parametrize("case", [pytest.param(c, id=er.case_id(c)) for c in er.GELU_CASES])
def test_gelu_is_the_fp64_reference_per_element(lib, record_property, case):
    c = case
    ge.assert_plan(lib, c)
    A, W, bias, z = er.gelu_operands(c)
    Ad, bd = ge.pack(c.prec, A).cuda(), bias.cuda()
    record_property("family", f"{er.family(c)} {ge.PREC_NAMES[c.prec]}")
    for e in er.exponents(c, W):
        who = f"{er.case_id(c)} weight exponent {e}"
        Wd = er.pack_w(c.prec, W, e).cuda()
        out = _owned(who, *_launch(lib, c, Ad, Wd, bd, 1, e))
        ratio, neighbours, beyond = er.gelu_verdict(c.prec, z, out)
        record_property(f"e{e}_ratio", f"{ratio:.4f}")
        record_property(f"e{e}_erf_margin_used", f"{er.erf_margin_used(c.prec, z, out):.4f}")
        record_property(f"e{e}_neighbour_share", f"{neighbours:.5f}")
        assert ratio <= 1.0, f"{who}: {er.describe_gelu_misses(c, z, out)}"
        assert beyond == 0, f"{who}: {beyond} outputs on z in {er.ULP_WINDOW} are further than one ulp from the reference rounded"
        assert neighbours <= er.NEIGHBOUR_CAP, f"{who}: {neighbours:.4f} of the outputs on z in {er.ULP_WINDOW} are a neighbour"


def _residual(lib, c, who, own, part_ref, bias, ls):
    """x += ls * (sum_z part[z] + bias) over the launch's slices: exact as well"""
    M, s = c.M, max(c.slices, 1)
    x0 = ge.make_x0(M, c.N)
    x = torch.full((GUARD + M + GUARD, c.N), float("nan"), dtype=torch.float32, device="cuda")
    x[GUARD:GUARD + M] = x0.cuda()
    bd, lsd = bias.cuda(), ls.cuda()
    rc = lib.vitvs_op_residual_ln(c.prec, ptr(x, GUARD * c.N * 4), ptr(own), s, ptr(bd), ptr(lsd), None, None, None, M, c.N, 1e-6,
                                  stream())
    assert rc == 0, f"{who}: vitvs_op_residual_ln returned {rc}"
    torch.cuda.synchronize()
    x = x.cpu()
    assert bool(torch.isnan(x[:GUARD]).all()) and bool(torch.isnan(x[GUARD + M:]).all()), f"{who}: x guard rows were written"
    got = x[GUARD:GUARD + M].double()
    ref = x0.double() + ls.double() * (part_ref.sum(0) + bias.double())
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, ref), ge.describe_mismatch(c, got, ref, f"{who} x after residual_ln")


@pytest.mark.parametrize("case", [pytest.param(c, id=er.case_id(c)) for c in er.X2_CASES])
def test_f16x2_cross_terms_are_exact(lib, case):
    c = case
    ge.assert_plan(lib, c)
    A, W, bias, ls = er.x2_operands(c)
    ref = er.x2_reference(c, A, W)
    Ad, bd = ge.pack(c.prec, A).cuda(), bias.cuda()
    for e in er.exponents(c, W):
        who = f"weight exponent {e}"
        Wd = er.pack_w(c.prec, W, e).cuda()
        rc, buf, own = _launch(lib, c, Ad, Wd, bd, 0, e)
        out = _owned(f"{er.case_id(c)} {who}", rc, buf, own)
        if c.epi == ge.STORE:
            got, want = er.output_values(c.prec, out), ref[0] + bias.double()
            assert torch.equal(got, want), ge.describe_mismatch(c, got, want, who)
        else:
            for z in range(out.shape[0]):
                assert torch.equal(out[z].double(), ref[z]), ge.describe_mismatch(c, out[z].double(), ref[z], f"{who} slice {z}")
            if c.N in ge.RLN_WIDTHS and c.slices <= 8:
                _residual(lib, c, f"{er.case_id(c)} {who}", own, ref, bias, ls)


@pytest.mark.parametrize("name,prec", ec.PRECS)
@pytest.mark.parametrize("M", [2048, 2049])
def test_residual_ln_on_both_sides_of_its_store_policy_switch(lib, record_property, name, prec, M):
    """The stress rows of test_layernorm_stress_rows, repeated over M rows: residual_ln_kernel stores write-through up to 2048 rows
    and plainly beyond.  The same checks, on the first six rows, six in the middle and the last row of each kind."""
    D, slices = 128, 4
    _, gamma, beta = ec.ln_stress_rows(D)
    x0, part, bias, x_ref = ec.ln_stress_parts(D, slices)
    idx = torch.arange(M) % ec.LN_ROWS
    nan = torch.full((GUARD, D), float("nan"))
    x = torch.cat([nan, x0[idx], nan]).cuda()
    out = nan_like(prec, GUARD + M + GUARD, D)
    pd, biasd, gd, bd = part[:, idx].contiguous().cuda(), bias.cuda(), gamma.cuda(), beta.cuda()
    rc = lib.vitvs_op_residual_ln(prec, ptr(x, GUARD * D * 4), ptr(pd), slices, ptr(biasd), None, ptr(gd), ptr(bd),
                                  ptr(out, GUARD * out.shape[1] * out.element_size()), M, D, 1e-6, stream())
    assert rc == 0
    torch.cuda.synchronize()
    x, out = x.cpu(), out.cpu()
    for t in (x, out):
        assert ec._all_nan(t[:GUARD]) and ec._all_nan(t[GUARD + M:]), "residual_ln: rows in front of or beyond its M were written"
    x, out = x[GUARD:GUARD + M], out[GUARD:GUARD + M]
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(out.float()).all())
    want = x_ref[idx]
    worst = float(((x.double() - want).abs().amax(1) / want.abs().amax(1)).max())
    ec._check(record_property, "residual_ln_x", worst, ec.BAR_X[prec])
    assert torch.equal(x[idx == ec.CONSTANT[0]], torch.full((int((idx == ec.CONSTANT[0]).sum()), D), 2.0)), \
        "residual_ln: a constant row's sum is not exact"
    groups = {"first": list(range(ec.LN_ROWS)), "middle": list(range(1020, 1020 + ec.LN_ROWS)),
              "last": [max(r for r in range(M) if r % ec.LN_ROWS == k) for k in range(ec.LN_ROWS)]}
    assert M - 1 in groups["last"] and all(r % ec.LN_ROWS == k for g in groups.values() for k, r in enumerate(g))
    for tag, g in groups.items():
        ec._check_ln_rows(record_property, prec, f"residual_ln_{tag}", out[g], x[g], gamma, beta)
