"""The exact GEMM cases of tests/gemm_exact_ref.py, without a GPU: every case is exact in its precision, plans the launch it
declares, and every fault model changes the reference in every tile it touches.  tests/test_gpu_gemm_exact.py runs the cases."""
import collections
import ctypes
import functools
import json
import os

import pytest
import torch

import vitvs_amd  # noqa: F401
from op_support import host_lib as lib  # noqa: F401
from op_support import plan_cover as cover  # noqa: F401

import gemm_exact_ref as ge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=2)
def _shape_operands(M, N, K, dens, slices):
    A, W = ge.make_a(M, K, dens), ge.make_w(N, K)
    bias, _ = ge.make_cols(N)
    return A, W, bias, ge.reference(A, W, slices)


def _operands(c):
    """(shared among the precisions that run the same shape: the cases are visited in the order of _shape)"""
    return _shape_operands(*_shape(c))


def _shape(c):
    return c.M, c.N, c.K, c.dens, max(c.slices, 1)


def test_ids_are_unique():
    ids = [ge.case_id(c) for c in ge.CASES + ge.REFUSED] + [ge.case_id(c) for s in ge.SWEEPS for c in ge.sweep_cases(s)]
    assert len(set(ids)) == len(ids)
    assert len({s.name for s in ge.SWEEPS}) == len(ge.SWEEPS)


@pytest.mark.parametrize("case", [pytest.param(c, id=ge.case_id(c)) for c in sorted(ge.CASES, key=_shape)])
def test_case_is_exact_and_every_fault_shows(case):
    A, W, bias, ref = _operands(case)
    ge.check_conditions(case, A, W, bias, ref)
    ge.check_faults(case, A, W, bias, ref)


@pytest.mark.parametrize("sweep", [pytest.param(s, id=s.name) for s in ge.SWEEPS])
def test_sweep_is_exact_and_every_fault_shows(sweep):
    """every M of the sweep, on the rows the GPU test gives it: the first M of one A per width"""
    cases = list(ge.sweep_cases(sweep))
    for N in sorted({c.N for c in cases}):
        mine = [c for c in cases if c.N == N]
        A, W, bias, ref = _operands(mine[0]._replace(M=max(c.M for c in mine)))
        for c in mine:
            ge.check_conditions(c, A[:c.M], W, bias, ref[:, :c.M], weights_checked=c is not mine[0])
            ge.check_faults(c, A[:c.M], W, bias, ref[:, :c.M])
    assert [c.M for c in cases] == (list(sweep.rows) if sweep.rows else ge.sweep_rows(sweep.BM)) and len(cases) == (14 if sweep.rows else 28)


def test_refused_cases_keep_the_conditions():
    for c in ge.REFUSED:       # (their launches never run: the operands only have to be well-formed)
        assert c.K // max(c.slices, 1) // ge.KTILE[c.prec] == 256 and c.K % c.dens == 0


def test_every_case_plans_its_declared_launch(lib):
    for c in ge.CASES:
        ge.assert_plan(lib, c)
        assert (c.grid is not None) == bool(c.key[0]) and (c.variant == 0 or c.variant == 2 or ge.BIG_VARIANT[c.variant] == tuple(c.key[1:3]))
    n = 0
    for s in ge.SWEEPS:
        for c in ge.sweep_cases(s):
            ge.assert_plan(lib, c)
            n += 1
    assert n == 74 * 28 + 20 * 14
    assert lib.vitvs_op_plan_in_flight(0) == 1                   # every hint was restored


def test_sweeps_cover_every_tile_precision_and_epilogue():
    """(rows, columns, k-groups, ring stages, precision, epilogue, forced by vitvs_op_linear_variant)"""
    have = {(s.BM, s.BN, s.kg, s.stages, s.prec, s.epi, s.variant != 0) for s in ge.SWEEPS}
    want = {(64, bn, kg, 0, p, ge.STORE, False) for bn in (64, 96, 128) for kg in (1, 2) for p in ge.PREC_NAMES}
    want |= {(64, 64, kg, 0, p, ge.PARTIAL, False) for kg in (1, 2) for p in ge.PREC_NAMES}
    want |= {(128, 128, 1, 0, p, e, False) for p in ge.PREC_NAMES for e in (0, 1)}            # as the library plans it
    want |= {(128, 128, 1, 0, p, e, True) for p in (ge.BF16, ge.F16) for e in (0, 1)}         # and at several k-tiles
    want |= {(bm, bn, 0, 0, p, e, True) for bm, bn in ge.BIG_VARIANT.values() for p in (ge.BF16, ge.F16, ge.F16X2) for e in (0, 1)}
    # the tails of the 3- and 2-stage rings: 64 columns in both forms, 128 columns (2 stages only) in the store form
    want |= {(64, 64, 1, st, p, e, False) for st in (3, 2) for p in ge.PREC_NAMES for e in (0, 1)}
    want |= {(64, 128, 1, 2, p, ge.STORE, False) for p in ge.PREC_NAMES}
    assert have == want
    for bm in (64, 128, 192, 256):
        rows = ge.sweep_rows(bm)
        for r in (1, 7, 8, 9, 15, 16, 17, bm // 2 - 1, bm // 2, bm // 2 + 1, bm - 17, bm - 16, bm - 1, bm):
            assert r in rows and bm + r in rows
    assert [m - 4096 for m in ge.ring_rows()] == [1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 63, 64]
    for s in ge.SWEEPS:
        if s.rows:     # more than 256 workgroups, which is what picks the shallower ring
            assert list(s.rows) == ge.ring_rows() and 65 * (s.N[0] // s.BN) > 256


def test_every_linear_key_of_plan_cover_is_hit(lib):
    """... by a case the LIBRARY plans (a forced tile does not count)."""
    with open(os.path.join(ROOT, "tests", "golden", "plan_cover.json")) as fh:
        rows = [r for r in json.load(fh)["rows"] if r["kind"] == "linear"]
    hit = {tuple([c.prec, c.epi] + c.key) for c in ge.CASES if c.variant == 0}
    hit |= {tuple([c.prec, c.epi] + c.key) for s in ge.SWEEPS if s.variant == 0 for c in ge.sweep_cases(s)}
    missing = [r["id"] for r in rows if tuple(r["key"]) not in hit]
    assert not missing, f"no exact case plans {missing}"
    product = [c for c in ge.CASES if c.name.endswith("-product")]
    assert len(product) == 6 and all(c.prec == ge.F16X2 and c.epi == ge.PARTIAL for c in product)
    by_id = {r["id"]: r for r in rows}
    for c in product:
        r = by_id[c.name[:-len("-product")]]
        assert (c.hint, c.M, c.N, c.K, c.slices) == (r["hint"], r["M"], r["N"], r["K"], r["slices"])


def test_product_domain_reaches_exactly_the_declared_maps(lib, cover):
    """A fresh walk of tools/plan_cover.py's domain through vitvs_op_linear_big_grid: a planner change that reaches another
    (tile, epilogue, XCD map), or stops reaching one, fails here by name; and each has a case."""
    reached = collections.Counter()
    out = (ctypes.c_int32 * 4)()
    seen = set()
    prev = lib.vitvs_op_plan_in_flight(1)
    try:
        for hint in cover.HINTS:
            lib.vitvs_op_plan_in_flight(hint)
            for _, _, _, cfg in cover.geometries():
                for frames in cover.FRAMES:
                    shapes = cover.layer_shapes(cfg, frames)
                    for layer, epi, _ in cover.LAYERS:
                        M, N, K = shapes[layer]
                        for prec in cover.PRECISIONS:
                            if (hint, prec, epi, M, N, K) in seen:
                                continue
                            seen.add((hint, prec, epi, M, N, K))
                            rc, (big, rows, cols, _, _, slices, _) = cover.linear_plan(lib, prec, epi, M, N, K)
                            assert rc == 0
                            if big:
                                assert lib.vitvs_op_linear_big_grid(prec, rows, cols, M, N, K, slices, out) == 0
                                reached[(rows, cols, epi, out[2])] += 1
                                assert out[2] == 0 or N // cols >= 8 // out[2], (prec, rows, cols, M, N, K, slices)
    finally:
        lib.vitvs_op_plan_in_flight(prev)
    new = sorted(set(reached) - ge.PRODUCT_REACHED)
    gone = sorted(ge.PRODUCT_REACHED - set(reached))
    assert not new, f"the product now reaches (rows, columns, epilogue, XCD map) {new}: add a map case for each"
    assert not gone, f"the product no longer reaches {gone}"
    have = {(c.key[1], c.key[2], c.epi, c.grid[2]) for c in ge.CASES if c.key[0]}
    assert not sorted(ge.PRODUCT_REACHED - have), f"no case runs {sorted(ge.PRODUCT_REACHED - have)}"
    named = {(c.key[1], c.key[2], c.epi, c.grid[2]) for c in ge.CASES if c.family == "map" and c.name.startswith("product-")}
    assert named == {k for k in ge.PRODUCT_REACHED if k[3]} and len(named) == 15


def test_map_family_reaches_the_edges_of_the_tile_walk():
    maps = [c for c in ge.CASES if c.family == "map"]
    assert all(c.variant in ge.BIG_VARIANT for c in maps)
    assert sum(c.grid[2] == 1 for c in maps) >= 2
    uneven_rows, uneven_cols = set(), set()
    for c in maps:
        xr = c.grid[2]
        if xr:
            bm, bn = c.key[1], c.key[2]
            R, nx = -(-c.M // bm) * max(c.slices, 1), c.N // bn
            assert R * nx == c.grid[0] > 256
            if R % xr:
                uneven_rows.add((bm, bn))
            if nx % (8 // xr):
                uneven_cols.add((bm, bn))
    assert uneven_rows == set(ge.BIG_VARIANT.values()) and uneven_cols == set(ge.BIG_VARIANT.values())
    assert any(c.grid[2] == 8 and c.N == c.key[2] for c in maps)     # one column tile
    flat = sorted(c.grid[0] for c in maps if c.grid[2] == 0)
    assert flat[0] < 8 and 9 in flat and 255 in flat and 256 in flat and flat[-1] <= 256


def test_launch_side_picks_no_map_that_leaves_an_xcd_without_a_column(lib):
    """Why no case has fewer column tiles than 8 / XR: over 1 .. 7 column tiles, up to 600 row tiles and 1 .. 4 slices on every
    tile the rule never picks such a map (nor does the product: test_product_domain_reaches_exactly_the_declared_maps)."""
    out = (ctypes.c_int32 * 4)()
    mapped = 0
    for bm, bn in ge.BIG_VARIANT.values():
        for nz in (1, 2, 3, 4):
            for nx in range(1, 8):
                for ny in range(1, 601):
                    if lib.vitvs_op_linear_big_grid(ge.BF16, bm, bn, ny * bm - 5, nx * bn, 128 * nz, nz, out) == 0 and out[2]:
                        mapped += 1
                        assert nx >= 8 // out[2], (bm, bn, nx, ny, nz, list(out))
    assert mapped > 10000


def test_kloop_and_slice_families_cover_what_they_name():
    per_ring = collections.defaultdict(set)
    for c in ge.CASES:
        if not c.key[0] and c.key[1] == 64:
            nk = c.K // max(c.slices, 1) // ge.KTILE[c.prec]
            per_ring[(c.key[3], c.key[4])].add(nk // c.key[3])
    for ring in ((1, 0), (1, 3), (1, 2)):
        assert per_ring[ring] >= {1, 2, 3, 4, 5, 8, 9}, ring
    assert per_ring[(2, 0)] >= {2, 3, 4}
    for tile in ge.BIG_VARIANT.values():
        nks = {c.grid[3] for c in ge.CASES if c.key[0] and tuple(c.key[1:3]) == tile and c.epi == ge.PARTIAL}
        assert nks >= {2, 3, 4, 5}
        assert {c.slices for c in ge.CASES if c.key[0] and tuple(c.key[1:3]) == tile} >= {2, 3, 4}
    assert any(c.key[0] and c.grid[3] == 255 for c in ge.CASES)
    for prec in ge.PREC_NAMES:
        assert {c.slices for c in ge.CASES if c.prec == prec and not c.key[0] and c.key[1] == 64} >= {2, 3, 4, 6, 8}
    xcd = {(c.N // 64, -(-c.M // 64)) for c in ge.CASES if c.key[6]}
    assert xcd >= {(nx, ny) for nx in (4, 8, 12) for ny in (1, 2, 3)}
    for c in ge.CASES:
        if c.family == "slices" and not c.name.startswith("xcd-nx8"):
            assert c.N in ge.RLN_WIDTHS, ge.case_id(c)        # vitvs_op_residual_ln runs over their slices


def test_tile_walk_restated_covers_every_grid_once_and_notices_a_shift():
    for nx, ny, nz, xmap in ((9, 29, 1, 4), (18, 15, 1, 2), (6, 43, 1, 8), (2, 43, 3, 8), (22, 21, 1, 1), (11, 8, 3, 4), (5, 51, 1, 0)):
        tiles = nx * ny * nz
        slots = min(8 * -(-tiles // 8), 256)
        seen = collections.Counter(t for wg in ge.tile_walk(nx, ny, nz, slots, xmap) for t in wg)
        assert len(seen) == tiles and set(seen.values()) == {1}
        off = collections.Counter(t for wg in ge.tile_walk(nx, ny, nz, slots, xmap, shift=1) for t in wg)
        assert len([t for t in seen if t not in off]) >= 1


def test_grid_hook_refuses_what_the_launcher_refuses(lib):
    out = (ctypes.c_int32 * 4)()

    def grid(prec, rows, cols, M, N, K, slices):
        return lib.vitvs_op_linear_big_grid(prec, rows, cols, M, N, K, slices, out), list(out)
    # (tests/test_cabi_symbols.py pins the values the hook reports; here: where it refuses)
    refused = [(ge.F32, 256, 256, 6274, 2304, 768, 0),          # no fp32 kernel
               (ge.BF16, 256, 64, 6274, 2304, 768, 0), (ge.BF16, 128, 128, 6274, 2304, 768, 0), (ge.BF16, 192, 192, 6274, 2304, 768, 0),
               (ge.BF16, 256, 256, 6274, 2304 + 128, 768, 0),   # N is not a multiple of the tile's columns
               (ge.BF16, 256, 256, 6274, 2304, 64, 0),          # one k-tile
               (ge.BF16, 256, 256, 6274, 2304, 768, 5),         # K is not a multiple of 5 k-tiles
               (ge.BF16, 256, 256, 6274, 2304, 768, 12),        # one k-tile per slice
               (ge.BF16, 256, 256, 6274, 2304, 256 * 64, 1),    # 256 k-tiles per slice
               (ge.F16X2, 256, 256, 6274, 2304, 256 * 32, 1),
               (ge.BF16, 256, 128, 300, 256 * 128, 128, 0),     # 256 column tiles
               (ge.BF16, 256, 256, 0, 2304, 768, 0), (ge.BF16, 256, 256, 300, 0, 768, 0), (ge.BF16, 256, 256, 300, 256, 0, 0),
               (ge.BF16, 256, 256, 1 << 21, 256, 1024, 0)]      # A past 4 GiB
    for args in refused:
        assert grid(*args) == (-2, [0, 0, 0, 0]), args
    assert grid(ge.BF16, 256, 256, 6274, 2304, 255 * 64, 1)[0] == 0 and out[3] == 255
    assert grid(ge.BF16, 256, 128, 300, 255 * 128, 128, 0)[0] == 0
    assert lib.vitvs_op_linear_big_grid(ge.BF16, 256, 256, 300, 256, 128, 0, None) == -1
    assert grid(ge.BF16, 256, 256, 300, 256, 128, -1)[0] == -1
    for c in ge.REFUSED:
        if c.variant:
            rows, cols = ge.BIG_VARIANT[c.variant]
            assert grid(c.prec, rows, cols, c.M, c.N, c.K, c.slices)[0] == -2, ge.case_id(c)
