"""The cases of tests/epilogue_exact_ref.py, without a GPU: the pre-activations and the hi / lo splits are exact, the recorded
statement errors are what the CPU re-measures, every case plans the launch it declares, and every fault model would be seen -
the GELU ones break a per-element bar or the neighbour cap in every precision they apply to, the cross-term ones change at least
three quarters of every output tile they touch.  tests/test_gpu_epilogue_exact.py runs the cases."""
import collections
import functools
import json
import os

import pytest
import torch

import vitvs_amd  # noqa: F401
from op_support import host_lib as lib  # noqa: F401

import epilogue_exact_ref as er
import gemm_exact_ref as ge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECS = (ge.F32, ge.BF16, ge.F16, ge.F16X2)


def _shape(c):
    return c.M, c.N, c.K


@functools.lru_cache(maxsize=2)
def _gelu_operands(M, N, K):
    return er.gelu_operands(ge.Case("rows", "", ge.F32, 1, ge.STORE, 0, M, N, K, 0, 8, None, None))


def test_ids_are_unique_and_shapes_are_the_tables():
    for cases in (er.GELU_CASES, er.X2_CASES):
        ids = [er.case_id(c) for c in cases]
        assert len(set(ids)) == len(ids)
    table = {(c.prec, c.epi, c.variant, c.M, c.N, c.K, c.slices, c.hint) for c in ge.CASES}
    table |= {(c.prec, c.epi, c.variant, c.M, c.N, c.K, c.slices, c.hint) for s in ge.SWEEPS for c in ge.sweep_cases(s)}
    for c in er.GELU_CASES + er.X2_CASES:
        assert (c.prec, c.epi, c.variant, c.M, c.N, c.K, c.slices, c.hint) in table, er.case_id(c)
        bm = c.key[1]
        assert c.dens == 8 and c.K % (32 * max(c.slices, 1)) == 0
        if c in er.GELU_CASES:
            assert c.epi == ge.STORE and c.M > bm and c.M % bm == 7, er.case_id(c)     # full row tiles and a ragged one


def test_every_case_plans_its_declared_launch(lib):
    for c in er.GELU_CASES + er.X2_CASES:
        ge.assert_plan(lib, c)
    assert lib.vitvs_op_plan_in_flight(0) == 1                   # every hint was restored


def test_every_declared_key_is_a_plan_of_the_forward_or_a_forced_tile():
    with open(os.path.join(ROOT, "tests", "golden", "plan_cover.json")) as fh:
        keys = {tuple(r["key"]) for r in json.load(fh)["rows"] if r["kind"] == "linear"}
    assert keys == er.FORWARD_KEYS
    for c in er.GELU_CASES + er.X2_CASES:
        assert c.variant != 0 or tuple([c.prec, c.epi] + c.key) in keys, f"{er.case_id(c)}: {c.key} is no key of plan_cover.json"


def test_cases_cover_every_family():
    """GELU: every store instantiation of test_gemm_exact_host's sweep table, both hints where the table has both.  Cross terms:
    every tile, both epilogues, one and two k-groups, 2 / 3 / 8 slices, one k-tile and K = 1024."""
    have = {(c.key[1], c.key[2], c.key[3], c.key[4], c.prec, c.variant != 0) for c in er.GELU_CASES}
    want = {(64, bn, kg, 0, p, False) for bn in (64, 96, 128) for kg in (1, 2) for p in PRECS}
    # the 128 x 128 tile: the forward plans it in fp32 only; forced for the plain 16-bit types.  The 2-stage ring on 128 columns.
    want |= {(128, 128, 1, 0, ge.F32, False)} | {(128, 128, 1, 0, p, True) for p in (ge.BF16, ge.F16)}
    want |= {(64, 128, 1, 2, p, False) for p in PRECS}
    want |= {(bm, bn, 0, 0, p, True) for bm, bn in ge.BIG_VARIANT.values() for p in (ge.BF16, ge.F16, ge.F16X2)}
    assert have == want
    hints = collections.defaultdict(set)
    for c in er.GELU_CASES:
        hints[c.key[3]].add(c.hint)
    assert hints[1] >= {1, 2} and hints[2] == {1}            # (two k-groups are planned under hint 1 only)
    x2 = er.X2_CASES
    assert all(c.prec == ge.F16X2 for c in x2)
    # (the forward plans no 128 x 128 tile in f16x2, and vitvs_op_linear_variant forces it for the plain 16-bit types only)
    tiles = {(64, 64), (64, 96), (64, 128)} | set(ge.BIG_VARIANT.values())
    assert {tuple(c.key[1:3]) for c in x2 if c.epi == ge.STORE} == tiles
    assert {tuple(c.key[1:3]) for c in x2 if c.epi == ge.PARTIAL} == tiles - {(64, 96), (64, 128)}   # (no partial form of those)
    assert {(c.key[3], c.key[4]) for c in x2 if not c.key[0]} == {(1, 0), (1, 2), (1, 3), (2, 0)}         # k-groups, ring stages
    assert {c.key[3] for c in x2 if not c.key[0]} == {1, 2}
    assert {c.slices for c in x2} >= {2, 3, 4, 6, 8}
    for tile in ge.BIG_VARIANT.values():
        assert {c.slices for c in x2 if tuple(c.key[1:3]) == tile} >= {2, 3}
    assert {c.K // max(c.slices, 1) for c in x2} >= {32, 64, 96, 512} and max(c.K for c in x2) == er.X2_MAX_K
    assert any(c.K == 32 for c in x2) and any(c.key[6] for c in x2)
    assert any(c.epi == ge.PARTIAL and c.N in ge.RLN_WIDTHS and 1 < c.slices <= 8 for c in x2)


# ------------------------------------------------------------------------------------------------ GELU
@pytest.fixture(scope="module")
def gelu_walk():
    """One pass over the GELU cases: per case the exactness conditions and the coverage of z; over all of them the statements'
    implied erf errors and neighbour shares, and each fault model's verdict."""
    E = dict.fromkeys(er.MEASURED_E, 0.0)
    share = dict.fromkeys(er.MEASURED_SHARE, 0.0)
    own = {}                   # case id -> verdict of the type's own restatement
    faults = {}                # (fault, case id) -> verdict
    for c in sorted(er.GELU_CASES, key=_shape):
        who = er.case_id(c)
        A, W, bias, z = _gelu_operands(*_shape(c))
        # z is exact in fp32 whatever the order: every product and the bias are multiples of 2^-12, every partial sum < 2^12
        assert torch.equal(z.float().double(), z) and torch.equal((z * 4096).round(), z * 4096), who
        assert float(z.abs().max()) < 16 and float((A.abs().double() @ W.abs().double().t()).max()) + 4.5 < 2 ** 12, who
        assert torch.equal((bias.double() * 4096).round(), bias.double() * 4096) and float(bias.abs().max()) <= 4.5
        assert torch.equal(ge.pack(c.prec, A).double() if c.prec != ge.F16X2 else ge.from_x2(ge.pack(c.prec, A))[0], A.double()), who
        for e in er.exponents(c, W):
            given = er.pack_w(c.prec, W, e)
            if c.prec == ge.F16X2:
                hi, lo = ge.from_x2(given)
                assert torch.equal(hi, W.double() * 2.0 ** e) and not bool(lo.any()), f"{who}: weights with exponent {e}"
            else:
                assert torch.equal(given.double(), W.double()), who
        if c.prec == ge.F16X2:
            assert er.exponents(c, W) == [0, 13], who
        cover = er.z_coverage(z)
        assert min(cover) >= er.Z_PER_UNIT, f"{who}: distinct z per unit interval of {er.Z_RANGE}: {cover}"
        form = er.FORM[c.prec]
        g = er.gelu_f32(form, z)
        E[form] = max(E[form], er.implied_erf_error(g, z))
        own[who] = er.gelu_verdict(c.prec, z, er.to_output(c.prec, g))
        if c.prec in share:
            share[c.prec] = max(share[c.prec], own[who][1])
        for name, (model, forms) in er.GELU_FAULTS.items():
            if form in forms:
                faults[(name, who, c.prec)] = er.gelu_verdict(c.prec, z, er.to_output(c.prec, model(c, A, W, bias, z)))
    return E, share, own, faults


def test_gelu_inputs_are_exact_and_the_recorded_figures_hold(gelu_walk):
    E, share, own, _ = gelu_walk
    for form, got in E.items():
        assert er.MEASURED_E[form] / 2 <= got <= er.MEASURED_E[form], (form, got)
    for prec, got in share.items():
        assert er.MEASURED_SHARE[prec] / 2 <= got <= er.MEASURED_SHARE[prec], (ge.PREC_NAMES[prec], got)
        assert 8 * er.MEASURED_SHARE[prec] <= er.NEIGHBOUR_CAP                  # the cap leaves the device the same room as the bars
    # the two forms are told apart from a tanh-form GELU (3.6e-4 implied) by two orders even after the margin
    assert er.MARGIN * max(er.MEASURED_E.values()) < 3.6e-4 / 50
    # every type's own restatement passes what the device is asked to pass, with the margin unused
    for who, (ratio, neighbours, beyond) in own.items():
        assert ratio <= 1.0 and neighbours <= er.NEIGHBOUR_CAP and beyond == 0, (who, ratio, neighbours, beyond)


def _broken(verdict):
    ratio, neighbours, beyond = verdict
    return ratio > 1.0 or neighbours > er.NEIGHBOUR_CAP or beyond > 0


@pytest.mark.parametrize("fault", sorted(er.GELU_FAULTS))
def test_every_gelu_fault_breaks_a_bar_in_every_case(gelu_walk, record_property, fault):
    mine = {k: v for k, v in gelu_walk[3].items() if k[0] == fault}
    forms = er.GELU_FAULTS[fault][1]
    assert {k[2] for k in mine} == {p for p in PRECS if er.FORM[p] in forms}
    for prec in sorted({k[2] for k in mine}):
        v = [x for k, x in mine.items() if k[2] == prec]
        record_property(f"{ge.PREC_NAMES[prec]}_least_ratio", f"{min(x[0] for x in v):.3g}")
        record_property(f"{ge.PREC_NAMES[prec]}_least_neighbour_share", f"{min(x[1] for x in v):.3g}")
    missed = [(who, ge.PREC_NAMES[p], v) for (_, who, p), v in mine.items() if not _broken(v)]
    assert not missed, f"{fault} passes: {missed}"


# ------------------------------------------------------------------------------------------------ f16x2 cross terms
@pytest.mark.parametrize("case", [pytest.param(c, id=er.case_id(c)) for c in er.X2_CASES])
def test_cross_term_case_is_exact_and_every_fault_shows(case):
    c, who = case, er.case_id(case)
    A, W, bias, ls = er.x2_operands(c)
    (ah, al), (wh, wl) = er.split(A), er.split(W)
    # the splits are exact, both halves are non-zero, and the kernel is given exactly them (the weights times 2^e)
    assert torch.equal((ah + al).float(), A) and torch.equal((wh + wl).float(), W)
    assert torch.equal(ah != 0, A != 0) and torch.equal(al != 0, A != 0) and bool((wh != 0).all()) and bool((wl != 0).all())
    assert torch.equal(ah, ge.make_a(c.M, c.K, 8).double()) and torch.equal(wh, ge.make_w(c.N, c.K).double())
    hi, lo = ge.from_x2(ge.pack(c.prec, A))
    assert torch.equal(hi, ah) and torch.equal(lo, al), who
    assert er.exponents(c, W) == [0, 11]
    for e in er.exponents(c, W):
        hi, lo = ge.from_x2(er.pack_w(c.prec, W, e))
        assert torch.equal(hi, wh * 2.0 ** e) and torch.equal(lo, wl * 2.0 ** e), f"{who}: weights with exponent {e}"
    ref = er.x2_reference(c, A, W)
    # every term is a multiple of 2^-13 and every partial sum is below 2^11: fp32 accumulation is exact in any order
    assert torch.equal((ref * 8192).round(), ref * 8192)
    assert float((A.abs().double() @ W.abs().double().t()).max()) + 8 < 2 ** 11, who
    first, second = er.x2_fp32_sums(c, A, W)
    assert torch.equal(first.double(), ref) and torch.equal(second.double(), ref), f"{who}: an fp32 summation order is not exact"
    # the dropped lo.lo is visible: the comparison really is against the three-term statement
    assert float((er.x2_full_product(c, A, W) != ref).double().mean()) > 0.9, who
    if c.epi == ge.STORE:
        out = ref[0] + bias.double()
        assert torch.equal(out.float().double(), out)
        hi, lo = ge.from_x2(ge.to_x2(out.float()))
        assert torch.equal(hi + lo, out), f"{who}: hi + lo of the output does not hold the sum"
    elif c.N in ge.RLN_WIDTHS:
        x = ge.make_x0(c.M, c.N).double() + ls.double() * (ref.sum(0) + bias.double())
        assert torch.equal(x.float().double(), x) and float(x.abs().max()) < 2 ** 10
    faults = er.x2_faults(c, A, W, ref)
    z = er.x2_fault_tile(c)[0]
    for name, faulty in faults.items():
        share = er.changed_share_per_tile(c, faulty[z], ref[z])
        assert share >= 0.75, f"{who}: {name} changes only {share:.2f} of an output tile"
    assert len(faults) == (4 if c.K // max(c.slices, 1) > 32 else 3)
