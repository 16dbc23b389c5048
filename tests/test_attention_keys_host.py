"""CPU-side checks of the attention key-set cases (tests/attention_keys_ref.py; tests/test_gpu_attention_keys.py runs them on the
GPU): every case plans the kernel it names, every attention plan the forward can make is reached by a case, the fixtures are
exact in every precision, and - the condition that makes the GPU comparison meaningful - every fault model, applied to the fp64
reference alone, moves the rows it touches by at least ten times the loosest attention bar.  The plans are host arithmetic in
the library (vitvs_op_attention_plan): no device calls here.

What "the rows it touches" means per fault.  In the every_key and tail families the two partners weigh 1/2 : 1/2 and EVERY
touched row must move by >= 0.2.  In the tilted family they weigh w : 1 - w with w up to sigmoid(2) = 0.88, and a fault that
only doubles one partner (the last key counted once more: 2 w (1 - w) / (2 - w), a tile counted twice: 2 w (1 - w) / (1 + w))
moves the most tilted rows by 0.11 .. 0.19, and such a row can be alone in the ragged last group of 16 (N = 129: one row).  For
these two faults the tilted family is held to the WORST row the fault touches in an (image, head) - what the GPU test asserts
on - being moved by >= 0.2; the every_key and tail families run at the same shapes and hold every row.  Faults that remove a partner, exchange it or fail to rescale it
are held to every touched row in all three families.  K and V of a neighbouring head or image together are held to every row;
K alone or V alone (not asked for by the fault list, added here) to the worst row of every group of 16 query rows, since one row
in ten thousand lands near its reference by chance."""
import ctypes as C
import json
import os

import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib
from op_support import host_lib as lib  # noqa: F401

import attention_keys_ref as ak

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = sorted({(c.n_img, c.N, c.H) for c in ak.CASES if c.N > 1})


def _plan(lib, c):
    """the case's plan under its hint (the hint is restored)"""
    out = (C.c_int32 * 6)()
    prev = lib.vitvs_op_plan_in_flight(c.hint)
    try:
        rc = lib.vitvs_op_attention_plan(c.prec, c.n_img, c.N, c.H, out)
    finally:
        lib.vitvs_op_plan_in_flight(prev)
    return rc, list(out)


def test_constants_are_the_librarys():
    assert (ak.F32, ak.BF16, ak.F16, ak.F16X2) == (_lib.F32, _lib.BF16, _lib.F16, _lib.F16X2)
    assert ak.SENSITIVITY >= 10 * max(ak.BARS.values()) and ak.SENSITIVITY >= 10 * ak.BAR_F16_RAW_LONG
    assert len({ak.case_id(c) for c in ak.CASES}) == len(ak.CASES)


@pytest.mark.parametrize("case", [pytest.param(c, id=ak.case_id(c)) for c in ak.CASES])
def test_case_plans_the_key_it_names(lib, case):
    rc, plan = _plan(lib, case)
    assert rc == 0
    assert ak.plan_key(case.prec, case.N, plan) == ak.case_key(case), f"{ak.case_id(case)}: the hook plans {plan} here"


def test_every_reachable_attention_plan_has_a_case():
    """A plan the planner gains later fails here by name until a case reaches it."""
    with open(os.path.join(ROOT, "tests", "golden", "plan_cover.json")) as fh:
        rows = [r for r in json.load(fh)["rows"] if r["kind"] == "attention"]
    assert rows
    have = {tuple(ak.case_key(c)) for c in ak.CASES}
    missing = [r["id"] for r in rows if tuple(r["key"]) not in have]
    assert not missing, f"no case of tests/attention_keys_ref.py reaches the plans {missing}"


@pytest.mark.parametrize("shape", SHAPES + [(1, 1, 1)], ids=lambda s: "x".join(map(str, s)))
def test_fixtures_are_exact_in_every_precision(shape):
    n_img, N, H = shape
    for family, launch in ak.launches(N):
        fx = ak.fixture(n_img, N, H, family, launch)
        q = fx.qkv[:, :H * 64]
        assert bool((q == q.round()).all()) and float(q.abs().max()) <= 9
        assert family == "tilted" or bool(((q == 0) | (q.abs() == 8)).all())
        assert bool((fx.qkv[:, H * 64:].abs() == 1).all())
        assert N == 1 or not bool((fx.a == N - 1).any())
        for prec in (ak.F32, ak.BF16, ak.F16, ak.F16X2):
            x, t = ak.operand(prec, fx.qkv)
            assert torch.equal(t, fx.qkv.double()), (family, launch, ak.PREC_NAMES[prec])
            if prec == ak.F16X2:            # lo = 0
                assert not bool(x.reshape(x.shape[0], -1, 2, 32)[:, :, 1].any())


def test_one_token_attends_to_itself():
    fx = ak.fixture(1, 1, 1, "every_key", 0)
    assert torch.equal(ak.reference(fx.qkv, 1, 1, 1), fx.qkv[:, 128:].double())


def test_draws_differ_between_images_and_heads():
    for n_img, N, H in SHAPES:
        k, v = ak._kv(n_img, N, H)
        for t in (k, v):
            flat = t.reshape(n_img * H, -1)
            agree = (flat @ flat.t() / flat.shape[1] + 1) / 2             # the share of entries on which two draws agree
            agree.fill_diagonal_(0.5)
            assert float((agree - 0.5).abs().max()) < 0.15, (n_img, N, H)      # independent +-1 draws agree on half their entries


def _part_kinds(lib, shape):
    """the distinct key partitions of the cases that share a shape"""
    kinds = {}
    for c in ak.CASES:
        if (c.n_img, c.N, c.H) != shape:
            continue
        rc, plan = _plan(lib, c)
        assert rc == 0
        parts = ak.key_parts(c, plan[4])
        kinds.setdefault(("ranges", plan[4]) if c.kernel == ak.K_LONG and c.divided else
                         "groups" if c.kernel == ak.K_Q64KS2 else "tiles", parts)
    return kinds


def _floor(err, touched, every_row, what):
    """the fault moved every touched row (every_row) or its worst touched row by >= SENSITIVITY"""
    assert bool(touched.any()), f"{what}: touches no row"
    e = err[touched]
    got = float(e.min() if every_row else e.max())
    assert got >= ak.SENSITIVITY, f"{what}: moves {'a' if every_row else 'its worst'} row by only {got:.3f} < {ak.SENSITIVITY}"
    return got


def _floor_groups(err, every_row, what, rows=16):
    """the same per group of `rows` query rows of an (image, head); 16 are the fewest a workgroup of any kernel here owns"""
    n = err.shape[-1]
    rows = min(rows, n)
    fill = float("inf") if every_row else float("-inf")
    e = torch.nn.functional.pad(err, (0, -n % rows), value=fill).reshape(*err.shape[:-1], -1, rows)
    got = float((e.amin(-1) if every_row else e.amax(-1)).min())
    assert got >= ak.SENSITIVITY, f"{what}: moves {'a' if every_row else 'the worst'} row of a group of {rows} by only {got:.3f} < {ak.SENSITIVITY}"
    return got


def check_sensitivity(lib, shape, q_factor=ak.Q_FACTOR):
    """Every fault model on every launch of a shape; returns the smallest movement seen per model."""
    n_img, N, H = shape
    nt, R = (N + 63) // 64, ak.last_tile_keys(N)
    kinds = _part_kinds(lib, shape)
    worst = {}
    probed = torch.zeros(N, max(R - 1, 1), dtype=torch.bool)

    def note(model, value):
        worst[model] = min(worst.get(model, 1e30), value)

    for family, launch in ak.launches(N):
        fx = ak.fixture(n_img, N, H, family, launch, q_factor)
        sm = ak.Softmax(fx)
        half = family != "tilted"                  # the partners weigh 1/2 : 1/2
        tag = f"{shape} {family} {launch}"
        everyone = torch.ones_like(fx.a, dtype=torch.bool)
        # 1. the last key counted once more, per group of 16 query rows
        note(1, _floor_groups(sm.errors(sm.reweigh_key(sm.last, 2.0)), half, f"{tag}: last key counted twice", 16 if half else N))
        # 2. one real key of the last tile masked for one query: the last key, and the row's other partner
        note(2, _floor(sm.errors(sm.reweigh_key(sm.last, 0.0)), everyone, True, f"{tag}: last key masked"))
        note(2, _floor(sm.errors(sm.reweigh_key(fx.a, 0.0)), everyone, True, f"{tag}: partner masked"))
        if family == "tail":
            probed[torch.arange(N), N - 2 - fx.a[0, 0]] = True
        # 3. one 64-key tile dropped, or counted twice
        for t in range(nt if nt >= 2 else 0):
            own, one = sm.owners(t), sm.owners(t, exactly_one=True)      # every_key: every tile has rows that own it
            if family == "every_key" or bool(own.any()):
                note(3, _floor(sm.errors(sm.reweigh_tile(t, 0.0)), own, True, f"{tag}: tile {t} dropped"))
            if family == "every_key" or bool(one.any()):
                note(3, _floor(sm.errors(sm.reweigh_tile(t, 2.0)), one, half, f"{tag}: tile {t} counted twice"))
        # 4. one key range / key group merged without rescaling to the common maximum
        if family == "tilted" and nt >= 2:
            for kind, parts in kinds.items():
                out, apart = sm.unscaled_part(parts)
                touched = apart & (sm.gap().abs() > 0.5)
                share = float(touched.float().mean())
                assert share >= 0.1, f"{tag} {kind}: only {share:.3f} of the rows have partners in different parts > 0.5 nat apart"
                note(4, _floor(sm.errors(out), touched, True, f"{tag} {kind}: part merged unscaled"))
        # 5. K and V from the neighbouring head, and from the neighbouring image
        for dim, n in ((0, n_img), (1, H)):
            for which in (("kv", "k", "v") if n >= 2 else ()):
                note(5, _floor_groups(sm.errors(sm.other_operands(dim, which)), which == "kv",
                                      f"{tag}: {which} of the neighbouring {'image' if dim == 0 else 'head'}"))
        # 6. the V rows of two keys of one tile swapped: the partner and its neighbour, the last key and its neighbour
        other = fx.a ^ 1
        down = (other == N - 1) & (fx.a % 64 != 0)
        other = torch.where(down, fx.a - 1, other)
        ok = other != N - 1
        if bool(ok.any()):
            note(6, _floor(sm.errors(sm.swapped_values(fx.a, torch.where(ok, other, fx.a))), ok, True, f"{tag}: partner's V swapped"))
        if R >= 2 and bool((fx.a != N - 2).any()):
            note(6, _floor(sm.errors(sm.swapped_values(sm.last, sm.last - 1)), fx.a != N - 2, True, f"{tag}: last key's V swapped"))
        if half:                                   # the fixture's premise: two partners, one half each
            p_last = sm.p[..., N - 1] / sm.L
            assert 0.45 <= float(p_last.min()) and float(p_last.max()) <= 0.5 + 1e-12, f"{tag}: last key's share"
    if R >= 2:
        assert bool(probed.all()), f"{shape}: the tail sweep leaves (query, key of the last tile) pairs unprobed"
    return worst


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_fault_model_moves_the_rows_it_touches(lib, record_property, shape):
    for model, value in sorted(check_sensitivity(lib, shape).items()):
        record_property(f"fault{model}_least_movement", f"{value:.3f}")


def test_a_blunt_fixture_fails_the_sensitivity_check(lib):
    """q = 0.25 (k[a] + k[N - 1]) in place of 4 (...): the softmax is close to uniform again and the check must say so."""
    with pytest.raises(AssertionError, match="moves"):
        check_sensitivity(lib, (43, 130, 2), q_factor=0.25)
