"""Every Gram form and tile of the correspondence stage, against an fp64 Gram (GPU).

The velocity path's correspondence is decided by plan_gram (correspond.hip): the fused arg-max over fp32 descriptors (32 x 32
tiles with two k-groups up to 512 tokens, 64 x 64 beyond), the same from the fp16 hi / lo split in the 16-bit modes from 1024
tokens (64 x 64 below 256 tiles of 128 x 128 over all pairs, 128 x 128 from there), and for binned descriptors the raw token
Gram with the 3 x 3 stencil arg-max.  Each case below names the plan it expects and asserts it through vitvs_op_gram_plan, then
runs the stage through vitvs_op_gram_argmax / vitvs_op_gram_stencil, which launch the steps of that plan through launch_gram_step
(correspond.hip) as the velocity path does: the same launches by construction.  The reference is an
fp64 Gram of the same normalised descriptors (for the stencil: of the concatenated 9 D-wide descriptors).  Bars:
  * every device arg-max is a row (nn_1) or column (nn_2) maximum to within 1e-6;
  * sim_1 is within 2e-6 of the row maximum;
  * the index is exactly fp64's wherever fp64's top-1 / top-2 margin exceeds 4e-6, so a dropped tile cannot hide;
  * exact duplicates keep the first index; keys and tables of pairs beyond n_pairs stay untouched.
tests/test_gram_cover_host.py checks without a GPU that these cases reach every plan key the product can."""
import ctypes as C
import zlib
from collections import namedtuple

import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib
from op_support import gpu_lib as lib  # noqa: F401
from op_support import ptr, stream

pytestmark = pytest.mark.gpu

GRAM_F32, GRAM_SPLIT, GRAM_STENCIL, GRAM_WIDE = 1, 2, 3, 4
FORM_NAMES = {GRAM_F32: "f32", GRAM_SPLIT: "split", GRAM_STENCIL: "stencil", GRAM_WIDE: "wide"}
ARGMAX_TOL, SIM_TOL, MARGIN = 1e-6, 2e-6, 4e-6
KEY_SENTINEL = 0x5A5A5A5A5A5A5A5A
IDX_SENTINEL = -7

# op: "fused" (vitvs_op_gram_argmax; D = the descriptor width Dp) or "stencil" (vitvs_op_gram_stencil; D = the token width,
# T = grid^2, P prefix rows).  special: "dup" exact duplicate rows and columns, "neg" every similarity negative (d2 ~ -d1),
# "binned" 9 D-wide concatenated neighbourhoods.
# family: (form, tile rows, tile columns, k-groups) that vitvs_op_gram_plan must report.
Case = namedtuple("Case", "id op prec T D pairs shared P special family")


def _c(cid, op, prec, T, D, pairs, shared, family, P=1, special=""):
    return Case(cid, op, prec, T, D, pairs, shared, P, special, family)


F32_32, F32_64 = (GRAM_F32, 32, 32, 2), (GRAM_F32, 64, 64, 1)
SPLIT_64, SPLIT_128 = (GRAM_SPLIT, 64, 64, 1), (GRAM_SPLIT, 128, 128, 1)
ST_32, ST_64 = (GRAM_STENCIL, 32, 32, 2), (GRAM_STENCIL, 64, 64, 1)
B16 = _lib.BF16
CASES = [
    # fp32 fused arg-max: both sides of T = 512, the Dp parity rule, ragged T, 1 .. 8 pairs with and without a shared goal
    _c("f32-t512", "fused", _lib.F32, 512, 64, 1, False, F32_32),
    _c("f32-t513", "fused", _lib.F32, 513, 64, 1, False, F32_64),
    _c("f32-t200-d96-odd-kgroups-2p", "fused", _lib.F32, 200, 96, 2, False, F32_64),
    _c("f32-t300-3p-shared", "fused", _lib.F32, 300, 64, 3, True, F32_32),
    _c("f32-t100-8p", "fused", _lib.F32, 100, 64, 8, False, F32_32),
    _c("f32-t150-8p-shared", "fused", _lib.F32, 150, 64, 8, True, F32_32),
    _c("f32-t777-3p", "fused", _lib.F32, 777, 128, 3, False, F32_64),
    _c("f32-t700-4p-shared", "fused", _lib.F32, 700, 64, 4, True, F32_64),
    _c("f16x2-t1024-2p", "fused", _lib.F16X2, 1024, 64, 2, False, F32_64),
    _c("f32-t333-dup", "fused", _lib.F32, 333, 64, 1, False, F32_32, special="dup"),
    _c("f32-t601-dup-2p", "fused", _lib.F32, 601, 64, 2, False, F32_64, special="dup"),
    _c("f32-t257-neg", "fused", _lib.F32, 257, 64, 1, False, F32_32, special="neg"),
    _c("f32-t640-neg-2p-shared", "fused", _lib.F32, 640, 64, 2, True, F32_64, special="neg"),
    _c("f32-t529-binned-9d-2p", "fused", _lib.F32, 529, 9 * 64, 2, False, F32_64, special="binned"),   # the 9 D-wide form's rows
    # split-f16 fused arg-max: ceil(T / 128)^2 * n_pairs = 192 and 256 at T = 1024, shared goals in both families, ragged T
    _c("split-t1024-3p", "fused", B16, 1024, 64, 3, False, SPLIT_64),
    _c("split-t1024-4p", "fused", B16, 1024, 64, 4, False, SPLIT_128),
    _c("split-t1024-2p-shared", "fused", B16, 1024, 64, 2, True, SPLIT_64),
    _c("split-t1024-4p-shared", "fused", B16, 1024, 64, 4, True, SPLIT_128),
    _c("split-t1100", "fused", _lib.F16, 1100, 64, 1, False, SPLIT_64),
    _c("split-t2000", "fused", B16, 2000, 64, 1, False, SPLIT_128),
    _c("split-t1030-8p", "fused", _lib.F16, 1030, 64, 8, False, SPLIT_128),
    _c("split-t1030-8p-shared", "fused", B16, 1030, 128, 8, True, SPLIT_128),
    _c("split-t1024-dup", "fused", B16, 1024, 64, 1, False, SPLIT_64, special="dup"),
    _c("split-t2100-dup", "fused", B16, 2100, 64, 1, False, SPLIT_128, special="dup"),
    _c("split-t1500-neg", "fused", B16, 1500, 64, 1, False, SPLIT_64, special="neg"),
    _c("split-t2100-neg", "fused", _lib.F16, 2100, 64, 1, False, SPLIT_128, special="neg"),
    # raw token Gram + stencil: grids 22 and 23 (T = 484, 529), P = 1 and 5, 1 .. 8 pairs with and without a shared goal
    _c("stencil-g22-p1", "stencil", _lib.F32, 484, 64, 1, False, ST_32, P=1),
    _c("stencil-g23-p5", "stencil", _lib.F32, 529, 64, 1, False, ST_64, P=5),
    _c("stencil-g22-p5-3p", "stencil", _lib.F32, 484, 128, 3, False, ST_32, P=5),
    _c("stencil-g22-p1-2p-shared", "stencil", _lib.F32, 484, 64, 2, True, ST_32, P=1),
    _c("stencil-g23-p1-2p", "stencil", _lib.F32, 529, 64, 2, False, ST_64, P=1),
    _c("stencil-g23-p5-3p-shared", "stencil", _lib.F32, 529, 64, 3, True, ST_64, P=5),
    _c("stencil-g7-p1-8p", "stencil", _lib.F32, 49, 64, 8, False, ST_32, P=1),
    _c("stencil-g30-p5-4p-shared", "stencil", _lib.F32, 900, 64, 4, True, ST_64, P=5),
]


def plan_args(case):
    """vitvs_op_gram_plan's arguments for the case: (precision, binned, T, D, n_pairs, max_pairs)."""
    return (case.prec, 1 if case.op == "stencil" else 0, case.T, case.D, case.pairs, case.pairs)


def gram_plan(lib, prec, binned, T, D, n_pairs, max_pairs):
    out = (C.c_int32 * 7)()
    rc = lib.vitvs_op_gram_plan(prec, binned, T, D, n_pairs, max_pairs, out)
    return rc, list(out)


def goal_kind(n_pairs, shared):
    return "one" if n_pairs == 1 else ("shared" if shared else "own")


def gram_key(plan, n_pairs, shared):
    """The code path a plan runs: form, tile rows, columns, k-groups and how the pairs find their desired frame.  The 9 D-wide
    form of binned descriptors launches the fused arg-max of the fp32 or the split form on wider rows: it shares their keys."""
    form = plan[0]
    if form == GRAM_WIDE:
        form = GRAM_SPLIT if plan[6] else GRAM_F32
    return (form, plan[1], plan[2], plan[3], goal_kind(n_pairs, shared))


def key_id(key):
    form, rows, cols, kg, goal = key
    return f"{FORM_NAMES.get(form, form)}-{rows}x{cols}-kg{kg}-{goal}"


def _unit(x):
    return x / x.norm(dim=-1, keepdim=True)


def _descriptors(case, gen):
    """fp32 rows [n_des + n_pairs][T][D], L2-normalised in fp32 (what the forward hands the Gram)."""
    n_des = 1 if case.shared else case.pairs
    T, D = case.T, case.D
    if case.special == "neg":          # every row in one cone, the current frames in the opposite one: all maxima < 0
        axis = _unit(torch.randn(D, generator=gen))
        des = _unit(axis + 0.1 * torch.randn(n_des, T, D, generator=gen))
        cur = -_unit(axis + 0.1 * torch.randn(case.pairs, T, D, generator=gen))
        return torch.cat([des, cur]).float()
    if case.special == "binned":       # concatenated 3 x 3 neighbourhoods of random tokens, as the 9 D-wide form takes them
        grid = int(round(T ** 0.5))
        return _binned_fp64(torch.randn(n_des + case.pairs, 1 + T, D // 9, generator=gen), T, 1, grid).float()
    d = torch.randn(n_des + case.pairs, T, D, generator=gen)
    if case.special == "dup":
        for b in range(case.pairs):
            a, c = (0 if case.shared else b), n_des + b
            # columns 3 (first) and T - 2 (another tile) hold the same descriptor, which row 17 also holds: S[17] ties there
            d[c, T - 2] = d[c, 3]
            d[a, 17] = d[c, 3]
            d[c, 41] = d[c, 40]     # a tie inside one tile
            d[a, 60] = d[c, 40]
            # rows 5 (first) and T - 5 are equal, and column 9 holds them: S[:, 9] ties there
            d[a, T - 5] = d[a, 5]
            d[c, 9] = d[a, 5]
    return _unit(d).float()


def _check_tables(case, S, nn1, nn2, sim1, b):
    T = case.T
    n1, n2 = nn1.astype(np.int64), nn2.astype(np.int64)
    assert n1.min() >= 0 and n1.max() < T and n2.min() >= 0 and n2.max() < T, (case.id, b)
    rmax, cmax = S.max(1), S.max(0)
    assert float((rmax - S[np.arange(T), n1]).max()) <= ARGMAX_TOL, (case.id, b, "nn_1 is not a row maximum")
    assert float((cmax - S[n2, np.arange(T)]).max()) <= ARGMAX_TOL, (case.id, b, "nn_2 is not a column maximum")
    assert float(np.abs(sim1.astype(np.float64) - rmax).max()) <= SIM_TOL, (case.id, b, "sim_1")
    top_r = np.sort(S, axis=1)[:, -2:]
    top_c = np.sort(S, axis=0)[-2:, :]
    clear_r = (top_r[:, 1] - top_r[:, 0]) > MARGIN
    clear_c = (top_c[1] - top_c[0]) > MARGIN
    assert clear_r.mean() > 0.5 and clear_c.mean() > 0.5, (case.id, "too few clear maxima to pin the indices")
    assert np.array_equal(n1[clear_r], S.argmax(1)[clear_r]), (case.id, b, "nn_1 differs from fp64 at a clear maximum")
    assert np.array_equal(n2[clear_c], S.argmax(0)[clear_c]), (case.id, b, "nn_2 differs from fp64 at a clear maximum")
    if case.special == "neg":
        assert float(rmax.max()) < 0 and float(cmax.max()) < 0
        assert float(sim1.max()) < 0
    if case.special == "dup":          # exact ties: the first index, as torch.max / numpy.argmax
        assert int(n1[17]) == 3 and int(n1[60]) == 40, (case.id, b, int(n1[17]), int(n1[60]))
        assert int(n2[9]) == 5, (case.id, b, int(n2[9]))


def _binned_fp64(x, T, P, grid):
    """[frames][P + T][D] tokens -> fp64 normalised 9 D-wide binned descriptors (dy, dx row-major, replicate-clamped)."""
    t = x[:, P:, :].double()
    ys, xs = np.divmod(np.arange(T), grid)
    parts = []
    for o in range(9):
        yy = np.clip(ys + o // 3 - 1, 0, grid - 1)
        xx = np.clip(xs + o % 3 - 1, 0, grid - 1)
        parts.append(t[:, torch.from_numpy(yy * grid + xx), :])
    b = torch.cat(parts, dim=-1)
    return b / b.norm(dim=-1, keepdim=True).clamp_min(1e-8)


def test_cases_are_unique():
    assert len({c.id for c in CASES}) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_gram_form_matches_fp64(lib, case):
    rc, plan = gram_plan(lib, *plan_args(case))
    assert rc == 0 and tuple(plan[:4]) == case.family, (case.id, plan)
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(zlib.crc32(case.id.encode()))
    T, n = case.T, case.pairs
    n_des = 1 if case.shared else n
    frames = n_des + n
    # outputs and keys of one guard pair behind the call's pairs; none may be written
    keys_r = torch.full(((n + 1) * T,), KEY_SENTINEL, dtype=torch.int64, device=dev)
    keys_c = keys_r.clone()
    nn1 = torch.full(((n + 1) * T,), IDX_SENTINEL, dtype=torch.int32, device=dev)
    nn2 = nn1.clone()
    sim1 = torch.full(((n + 1) * T,), float("nan"), dtype=torch.float32, device=dev)
    if case.op == "fused":
        dn = _descriptors(case, gen)
        dh = torch.empty(3 * frames * T * case.D, dtype=torch.float16, device=dev) if plan[6] else None
        dn_dev = dn.to(dev)
        rc = lib.vitvs_op_gram_argmax(case.prec, ptr(dn_dev), T, case.D, n, int(case.shared), ptr(dh), ptr(keys_r), ptr(keys_c),
                                      ptr(nn1), ptr(nn2), ptr(sim1), stream())
        ref = dn.double()
    else:
        grid = int(round(T ** 0.5))
        x = torch.randn(frames, case.P + T, case.D, generator=gen)
        x[:, :case.P] *= 50.0          # prefix rows far larger than the tokens: one that leaks in shows
        G = torch.full(((n + 1) * T * T,), float("nan"), dtype=torch.float32, device=dev)
        sq = torch.full(((frames + 1) * T,), float("nan"), dtype=torch.float32, device=dev)
        x_dev = x.to(dev)
        rc = lib.vitvs_op_gram_stencil(ptr(x_dev), T, case.P, case.D, grid, n, int(case.shared), ptr(G), ptr(sq), ptr(keys_r),
                                       ptr(keys_c), ptr(nn1), ptr(nn2), ptr(sim1), stream())
        ref = _binned_fp64(x, T, case.P, grid)
    assert rc == 0, (case.id, rc, _lib.last_error(None))
    torch.cuda.synchronize()
    tail = slice(n * T, None)
    assert bool((keys_r[tail] == KEY_SENTINEL).all()) and bool((keys_c[tail] == KEY_SENTINEL).all()), (case.id, "guard keys")
    assert bool((nn1[tail] == IDX_SENTINEL).all()) and bool((nn2[tail] == IDX_SENTINEL).all()), (case.id, "guard tables")
    assert bool(sim1[tail].isnan().all()), (case.id, "guard sim_1")
    if case.op == "stencil":
        assert bool(G[n * T * T:].isnan().all()) and bool(sq[frames * T:].isnan().all()), (case.id, "guard Gram / norms")
    n1, n2, s1 = nn1.cpu().numpy(), nn2.cpu().numpy(), sim1.cpu().numpy()
    for b in range(n):
        a = 0 if case.shared else b
        S = (ref[a] @ ref[n_des + b].T).numpy()
        o = slice(b * T, (b + 1) * T)
        _check_tables(case, S, n1[o], n2[o], s1[o], b)
