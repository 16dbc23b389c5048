"""CPU-side checks of the drop-in boundary: libvitvs_hip.so builds (hipcc cross-compiles gfx950
without a GPU), loads, and exports every symbol include/*.h declares.  No compute calls here."""
import ctypes
import os
import re

import pytest

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib
from op_support import host_lib as lib  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    with open(os.path.join(ROOT, "include", header)) as fh:
        text = fh.read()
    return set(re.findall(r"VITVS_API\s+[\w\s\*]+?\b(vitvs_\w+)\s*\(", text))


def test_headers_and_binding_agree(lib):
    declared = _declared("vitvs.h") | _declared("vitvs_ops.h")
    assert declared, "no prototypes found in include/"
    assert declared == set(_lib.PROTOTYPES), (declared ^ set(_lib.PROTOTYPES))


def test_every_declared_symbol_is_exported(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in _declared("vitvs.h") | _declared("vitvs_ops.h"):
        assert hasattr(raw, name), f"{name} not exported"


def test_abi_version_and_config_layout(lib):
    assert lib.vitvs_abi_version() == _lib.ABI_VERSION
    # struct vitvs_config: 8 int32, 7 float, 5 int32, double, 2 int32 -> 96 bytes (static_assert'ed in api.hip)
    assert ctypes.sizeof(_lib.VitvsConfig) == 96
    assert _lib.VitvsConfig.lambda_.offset == 80


def test_create_rejects_bad_config_without_touching_a_gpu(lib):
    cfg = _lib.VitvsConfig()
    cfg.abi_version = 999
    h = ctypes.c_void_p()
    assert lib.vitvs_create(ctypes.byref(cfg), ctypes.byref(h)) < 0
    assert b"abi_version" in lib.vitvs_last_error(None)


def test_engine_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from vitvs_amd import config
    from vitvs_amd.engine import Engine, VitvsError
    with pytest.raises(VitvsError):
        Engine(config.baseline_config("vits16_224"))


def test_bench_split_k_mirror_matches_the_library_plan():
    """bench.py prices the split-K GEMM with its own mirror of the slice plan; the plan itself is host arithmetic in the
    library (no device call), so the two can be compared without a GPU."""
    import importlib.util
    import os
    from vitvs_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    lib = _lib.load()
    for prec, bk in ((_lib.BF16, 64), (_lib.F16, 64), (_lib.F32, 32)):
        for m in (197, 394, 788, 1576, 3152, 970, 2740, 6274):
            for n, k in ((768, 768), (768, 3072), (384, 384), (384, 1536), (1024, 1024), (1024, 4096), (768, 640), (768, 192)):
                assert bench.split_k(m, n, k, bk) == lib.vitvs_op_splitk_slices(prec, m, n, k), (prec, m, n, k)
    # ... and under the plan hint of a handle whose updates run beside others (vitvs_set_option "in_flight")
    assert lib.vitvs_op_plan_in_flight(3) == 1
    try:
        for m in (197, 394, 788, 1576, 2364, 3152, 2740, 6274):
            for n, k in ((768, 768), (768, 3072), (384, 1536), (1024, 4096)):
                assert bench.split_k(m, n, k, 64, 3) == lib.vitvs_op_splitk_slices(_lib.BF16, m, n, k), (m, n, k)
        t = (ctypes.c_int32 * 3)()
        assert lib.vitvs_op_linear_tile(_lib.BF16, 394, 2304, 768, 0, t) == 0 and list(t) == [64, 64, 1]   # 4-wave workgroups
    finally:
        assert lib.vitvs_op_plan_in_flight(1) == 3
    t = (ctypes.c_int32 * 3)()
    assert lib.vitvs_op_linear_tile(_lib.BF16, 394, 2304, 768, 0, t) == 0 and list(t) == [64, 64, 2]


def test_linear_tile_plan_of_the_library():
    """The tile family per layer shape is host arithmetic (vitvs_op_linear_tile, no device call).  Pins the measured choices:
    64-row tiles while they cover the layer in one round of workgroups, 256-row tiles where they would need a second one, and
    between 256 x 256 and 256 x 128 the one that leaves the busiest CU the least work (profiles/r02_notes.md section 2)."""
    import ctypes
    from vitvs_amd import _lib
    lib = _lib.load()

    def plan(prec, m, n, k, slices=0):
        t = (ctypes.c_int32 * 3)()
        assert lib.vitvs_op_linear_tile(prec, m, n, k, slices, t) == 0
        return tuple(t)
    b = _lib.BF16
    assert plan(b, 394, 3072, 768) == (64, 96, 2)            # one frame pair: fc1, qkv, the K-sliced narrow layers
    assert plan(b, 394, 2304, 768) == (64, 64, 2)
    assert plan(b, 394, 768, 3072, 3) == (64, 64, 2)
    assert plan(b, 788, 2304, 768) == (64, 128, 2)           # two pairs: still one round of 64-row tiles
    assert plan(b, 788, 3072, 768) == (64, 128, 1)           # 312 workgroups on a 2-stage ring (3 per CU) against 120 tiles of 192 x 128
    assert plan(b, 985, 2304, 768) == (64, 128, 1)           # rotation search (5 images): 288 workgroups, still one round
    assert plan(b, 1182, 2304, 768) == (192, 128, 0)         # 342 workgroups: no gain in the forward, the persistent tiles keep it
    assert plan(b, 2364, 3072, 768) == (256, 128, 0)         # 120 tiles of 256 x 256 would leave half the CUs idle
    assert plan(b, 3152, 3072, 768) == (256, 192, 0)         # 8 pairs: 208 tiles of 256 x 192 in one round beat 156 of 256 x 256
    assert plan(b, 3152, 2304, 768) == (256, 128, 0)
    assert plan(b, 3152, 768, 3072, 3) == (256, 128, 0)
    assert plan(b, 3152, 768, 768, 1) == (64, 64, 1)
    assert plan(b, 6274, 2304, 768) == (256, 256, 0)         # ViT-B/8 448
    assert plan(b, 6274, 3072, 768) == (256, 192, 0)         # 400 tiles in two rounds beat 600 of 256 x 128 in three
    assert plan(b, 2740, 3072, 1024) == (256, 192, 0)        # ViT-L/14 518
    assert plan(b, 2740, 4096, 1024) == (192, 256, 0)        # 240 tiles against 176 of 256 x 256
    assert plan(b, 2740, 1024, 4096, 2) == (192, 128, 0)     # 240 tiles of 192 x 128 in one round against 176 of 256 x 128
    assert plan(b, 6274, 768, 3072, 1) == (192, 128, 0)
    assert plan(_lib.F32, 6274, 3072, 768) == (128, 128, 1)  # fp32 never takes the 256-row kernels
    t = (ctypes.c_int32 * 3)()
    assert lib.vitvs_op_linear_tile(b, 394, 768, 3072, 5, t) != 0   # 3072 is not a multiple of 5 k-tiles
    # The whole table: every linear shape of the BASELINE configs at 1 .. 16 images (patch-embed, qkv, proj, fc1, fc2) and the
    # shapes above, in the four precisions, under the hints 1 .. 4 of updates in flight, as vitvs_op_linear and as the partial-sum
    # form at the library's slice count.  Columns: hint, precision, M, N, K, slices (0: vitvs_op_linear), return code, tile[0..2];
    # recorded through this ABI.
    import numpy as np
    table = np.load(os.path.join(ROOT, "tests", "golden", "linear_plans.npz"))["plans"]
    assert len(table) > 15000
    prev = lib.vitvs_op_plan_in_flight(1)
    try:
        for hint, prec, m, n, k, slices, rc, *tile in table.tolist():
            lib.vitvs_op_plan_in_flight(hint)
            if slices:
                assert lib.vitvs_op_splitk_slices(prec, m, n, k) == slices, (hint, prec, m, n, k)
            got = lib.vitvs_op_linear_tile(prec, m, n, k, slices, t)
            assert (got, list(t)) == (rc, tile), (hint, prec, m, n, k, slices)
    finally:
        lib.vitvs_op_plan_in_flight(prev)


def test_linear_big_grid_of_the_library():
    """The grid of a launch on the 256- / 192-row tiles is host arithmetic on the launch side (vitvs_op_linear_big_grid, no device
    call): tiles, persistent workgroups, the XCD map of the tile walk, k-tiles per slice.  Pins the map rule at the shapes its
    comments name; tests/test_gemm_exact_host.py walks the product domain and checks the refusals."""
    lib = _lib.load()
    out = (ctypes.c_int32 * 4)()

    def grid(prec, rows, cols, m, n, k, slices=0):
        assert lib.vitvs_op_linear_big_grid(prec, rows, cols, m, n, k, slices, out) == 0
        return list(out)
    b = _lib.BF16
    assert grid(b, 256, 256, 6274, 2304, 768) == [225, 232, 0, 12]       # under one tile per CU: the balanced list
    assert grid(b, 256, 128, 6274, 3072, 768) == [600, 256, 4, 12]       # several tiles per CU: a 4 x 2 XCD grid
    assert grid(b, 256, 192, 6274, 3072, 768) == [400, 256, 4, 12]
    assert grid(b, 192, 128, 6274, 768, 3072, 3) == [594, 256, 8, 16]    # K slices count as rows of the grid
    assert grid(_lib.F16X2, 256, 256, 1542, 1024, 1024, 2) == [56, 56, 0, 16]   # f16x2: 32 logical k per k-tile
    assert grid(b, 256, 192, 5245, 4224, 128) == [462, 256, 1, 2]        # one row of eight column blocks


def test_attention_plan_of_the_library():
    """The attention launch per shape is host arithmetic too (vitvs_op_attention_plan, no device call): kernel, workgroups,
    threads, dynamic LDS bytes, key tiles per workgroup, divided.  Every attention kernel is exact for every shape it accepts,
    so the numeric tests pass whichever one is picked; this pins the pick."""
    import numpy as np
    lib = _lib.load()
    out = (ctypes.c_int32 * 6)()

    def plan(prec, n_img, n, h):
        assert lib.vitvs_op_attention_plan(prec, n_img, n, h, out) == 0
        return list(out)
    prev = lib.vitvs_op_plan_in_flight(1)
    try:
        # one ViT-B/16 224 pair: the 16-query kernel, 312 workgroups
        assert plan(_lib.BF16, 2, 197, 12) == [2, 312, 256, 4 * 8192 + 4 * 5 * 64 * 16, 0, 0]
        # one ViT-B/8 448 pair alone: the long kernel, key ranges of 25 tiles (half an item) merged through the workspace
        assert plan(_lib.BF16, 2, 3137, 12) == [5, 1200, 256, 3 * 2 * 64 * 128 + 16, 25, 1]
        # the same pair in f16x2: its own long kernel (from 2048 tokens), whole items
        assert plan(_lib.F16X2, 2, 3137, 12) == [5, 600, 256, 3 * 2 * 32 * 256, 50, 0]
        lib.vitvs_op_plan_in_flight(3)
        # beside other updates: whole items, no workspace
        assert plan(_lib.BF16, 2, 3137, 12) == [5, 600, 256, 3 * 2 * 64 * 128 + 16, 50, 0]
    finally:
        lib.vitvs_op_plan_in_flight(prev)
    assert lib.vitvs_op_attention_plan(_lib.BF16, 0, 197, 12, out) == -2 and out[0] == 0
    # The whole table: hints {1, 3} x the four precisions x H in {2, 4, 6, 12, 16} x n_img in {1 .. 16, 24, 32, 49, 96} x N on
    # both sides of every threshold and at every config's sequence length (with and without register tokens).  Columns: hint,
    # precision, n_img, N, H, return code, out[0..5]; recorded through this ABI and checked against the kernels the parent
    # library launched for every row.
    table = np.load(os.path.join(ROOT, "tests", "golden", "attention_plans.npz"))["plans"]
    assert len(table) == 2 * 4 * 5 * 20 * 23
    assert (table[table[:, 1] == _lib.F32, 6] == 1).all()   # fp32 is always the fp32 kernel
    prev = lib.vitvs_op_plan_in_flight(1)
    try:
        for hint, prec, n_img, n, h, rc, *want in table.tolist():
            lib.vitvs_op_plan_in_flight(hint)
            got = lib.vitvs_op_attention_plan(prec, n_img, n, h, out)
            assert (got, list(out)) == (rc, want), (hint, prec, n_img, n, h)
    finally:
        lib.vitvs_op_plan_in_flight(prev)


def test_gram_plan_of_the_library():
    """The correspondence stage per handle and call is host arithmetic as well (vitvs_op_gram_plan, no device call): form,
    tile rows, columns, k-groups, band rows, workgroups per XCD, split.  The table: every geometry of tools/plan_cover.py x the
    four precisions x binned off / on x max_pairs 1 .. 16 x n_pairs 1 .. max_pairs, then both sides of every switch point of
    tests/test_gram_cover_host.py (each also at n_pairs = max_pairs) and its refusals, in the four precisions.  Columns: precision, binned, T, D, n_pairs,
    max_pairs, return code, out[0..6]; recorded through this ABI before the stage was launched from its plan."""
    import numpy as np
    lib = _lib.load()
    out = (ctypes.c_int32 * 7)()
    table = np.load(os.path.join(ROOT, "tests", "golden", "gram_plans.npz"))["plans"]
    assert len(table) == 84 * 4 * 2 * 136 + 4 * 21
    assert set(np.unique(table[:, 7]).tolist()) == {0, 1, 2, 3, 4} and (table[:, 6] == -2).sum() >= 16
    at_capacity = {}
    for prec, binned, T, D, n, max_pairs, rc, *want in table.tolist():
        got = lib.vitvs_op_gram_plan(prec, binned, T, D, n, max_pairs, out)
        assert (got, list(out)) == (rc, want), (prec, binned, T, D, n, max_pairs)
        if n == max_pairs:
            at_capacity[(prec, binned, T, D, max_pairs)] = (want[0], want[6])
    # What the handle's workspaces rest on (it plans them at n_pairs = max_pairs): the form and the split of a call's plan do
    # not depend on its pairs, only the tile does.
    for prec, binned, T, D, n, max_pairs, rc, *want in table.tolist():
        if rc == 0:
            assert (want[0], want[6]) == at_capacity[(prec, binned, T, D, max_pairs)], (prec, binned, T, D, n, max_pairs)


def test_servo_plan_of_the_library():
    """The control law's launch is host arithmetic too (vitvs_op_servo_plan, no device call): the instantiation bits, the dynamic
    LDS bytes, the refinement's source and what the launch reads of the current depth image.  The kernel lays its LDS out by the
    same sizes, so a plan that came out too small would write past its allocation: the bytes are pinned here, against a
    restatement of the formula the launch used before it was planned and against literal anchors, before anything runs."""
    lib = _lib.load()
    out = (ctypes.c_int32 * 7)()
    ROWS = 128                                               # L rows kept in LDS (servo.hip kLdsRows)

    def lds_bytes(T, max_rows, robust, refine):
        words = 4 * T + (T if T <= 256 else 0) + max_rows + 16 + 4      # zraw [T]: the depth prefetch, T <= 256 only
        lds = ((words * 4 + 15) & ~15) + 7 * ROWS * 8 + (40 + 8 * 27) * 8
        if robust:
            lds += (7 * ROWS + ROWS // 2 + max_rows) * 8
        if refine:
            lds += max_rows * 2 * 4
        return lds

    def plan(T, max_rows, robust=0, source=0, interaction=0):
        rc = lib.vitvs_op_servo_plan(T, max_rows, robust, source, interaction, out)
        return rc, list(out)
    for T in (16, 196, 256, 289, 484, 1024, 3136, 4096, 5184, 6400):
        for max_rows in (24, 48, 130, T):
            for robust in (0, 1, 16):
                for source in (0, 1, 2, 3):
                    for interaction in (0, 1, 2):
                        want = lds_bytes(T, max_rows, robust > 0, source != 0)
                        rc, got = plan(T, max_rows, robust, source, interaction)
                        what = (T, max_rows, robust, source, interaction)
                        assert rc == (-3 if want > 160 * 1024 else 0), what
                        assert got == [int(robust > 0), int(source != 0), int(interaction != 0), want, source,
                                       int(interaction != 1), int(source != 0)], (what, got)
    # T, max_rows -> plain, refine, robust, robust + refine; T = 256 and 289 on either side of the depth-prefetch words; at
    # T = 3136 the plain and refine plans stay under 64 KiB (the per-instantiation opt-in) and both robust plans pass it
    anchors = {(196, 48): (13408, 13792, 21472, 21856), (256, 48): (14608, None, None, None), (289, 48): (14112, None, None, None),
               (3136, 48): (59664, 60048, 67728, 68112), (4096, 4096): (91216, 123984, 131664, 164432),
               (5184, 5184): (None, 154448, 162128, None)}
    for (T, max_rows), sizes in anchors.items():
        for (robust, source), want in zip(((0, 0), (0, 3), (2, 0), (2, 3)), sizes):
            if want is not None:
                rc, got = plan(T, max_rows, robust, source)
                assert (rc, got[3]) == (-3 if want > 160 * 1024 else 0, want), (T, max_rows, robust, source, got)
    assert 60048 < 64 * 1024 < 67728 and plan(5184, 5184, 2, 3)[0] == -3
    for bad in (dict(robust=17), dict(robust=-1), dict(interaction=3), dict(interaction=-1), dict(source=4), dict(source=-1)):
        assert plan(196, 48, **bad)[0] == -2, bad
    assert plan(0, 48)[0] == -2 and plan(196, 0)[0] == -2
