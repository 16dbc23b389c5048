"""Exact inputs for the GEMMs: operands, fp64 reference, case table and fault models (no GPU; used by
tests/test_gemm_exact_host.py and tests/test_gpu_gemm_exact.py).

Random operands leave a dropped or doubled term at a few elements far under the 16-bit bars of the linear tests (bf16 1.5e-2 of
the output scale is ~0.07 absolute at K = 384, one k-tile of one wave's sub-tile is ~0.05).  Here every operand is a small
integer, so that every precision computes the result EXACTLY (fp32 accumulation of integers below 2^24 in any order; bf16
outputs <= 256, fp16 and f16x2 outputs <= 2048, where the f16x2 low halves are zero) and the comparison is == per element:

  A     one non-zero entry (+-1) per `dens` consecutive k (dens = 8: one per 16-byte chunk of a 16-bit operand; 32 for long
        K); position and sign depend on (row, chunk): the low 16 bits of the row number are spelt out by the first four
        chunks, so rows are pairwise different whenever K >= 4 dens, the rest is hashed
  W     in {-2, -1, 1, 2}, hashed by (column, k)
  bias  integer in [-8, 8];  ls in {-1, 1, 2};  x0 integer in [-4, 4]

The reference is the fp64 product A @ W.T (per K slice for the partial sums).  GELU is not exact, and integer operands have no
f16x2 low halves: tests/epilogue_exact_ref.py makes the pre-activation and the hi / lo cross terms exact instead and
tests/test_gpu_epilogue_exact.py compares per element; LayerNorm is held per row by test_layernorm_stress_rows.

CASES is literal: every case declares the plan it must get, `key` = [big family, rows, columns, k-groups, ring stages, K slices >
1, XCD map] as tools/plan_cover.py keys a linear launch, and for the tiles of gemm_big.hip `grid` = [tiles, workgroups, XCD map
of the tile walk, k-tiles per slice] as vitvs_op_linear_big_grid reports it.  variant is vitvs_op_linear_variant's tile code
(0: the library's own plan through vitvs_op_linear / vitvs_op_linear_partial under the case's in-flight hint).  Families:

  map     the tile walk of linear_big_kernel: one case per (tile, epilogue, XCD map != 0) the product domain of
          tools/plan_cover.py reaches (PRODUCT_REACHED, the names product-*), XCD map 1, uneven splits of the XR x 8 / XR grid
          in both directions for every tile, one column tile, and the balanced list (map 0) at < 8, 9, 255 and 256 tiles
  kloop   k-tiles per k-group 1 .. 9 on the 4-, 3- and 2-stage rings and with two k-groups; 2 .. 5 and 255 on the big tiles
  slices  2, 3, 4, 6, 8 K slices on the 64-row tiles, 2, 3, 4 on the big ones, the 64-row XCD map at 4 / 8 / 12 column tiles
  keys    one small shape for every linear key of tests/golden/plan_cover.json no case above plans (six f16x2 partial keys have
          no small shape: their product representative)

SWEEPS are the row-edge sweeps: per (tile, precision, epilogue) every M = q BM + r of sweep_rows(BM); the 2- and 3-stage rings
of the 64-row launches with more than 256 workgroups sweep the same r behind 64 full row tiles (ring_rows()).
"""
import collections
import ctypes as C

import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib

F32, BF16, F16, F16X2 = _lib.F32, _lib.BF16, _lib.F16, _lib.F16X2
STORE, PARTIAL = 0, 1
PREC_NAMES = {F32: "fp32", BF16: "bf16", F16: "fp16", F16X2: "f16x2"}
DTYPES = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16, F16X2: torch.float16}
KTILE = {F32: 32, BF16: 64, F16: 64, F16X2: 32}              # logical k per 128-byte k-tile
STORE_LIMIT = {F32: 2 ** 24, BF16: 256, F16: 2048, F16X2: 2048}   # |store output| every integer up to which the type holds
RLN_WIDTHS = (128, 256, 384, 768, 1024)                       # widths vitvs_op_residual_ln has a kernel for
BIG_VARIANT = {256: (256, 256), 192: (256, 192), 128: (256, 128), 1192: (192, 128), 1256: (192, 256)}
# linear_big_kernel's waves: tile -> (wave rows WGM, wave columns WGN, rows of a wave, columns of a wave)
BIG_WAVES = {(256, 256): (2, 4, 128, 64), (256, 192): (4, 2, 64, 96), (256, 128): (4, 2, 64, 64), (192, 128): (2, 4, 96, 32),
             (192, 256): (2, 4, 96, 64)}

Case = collections.namedtuple("Case", "family name prec hint epi variant M N K slices dens key grid")
Sweep = collections.namedtuple("Sweep", "name prec hint epi variant BM BN kg N K slices stages rows", defaults=(0, None))

# (tile rows, tile columns, epilogue, XCD map of the tile walk) of every launch on a tile of gemm_big.hip that the product
# domain of tools/plan_cover.py makes, as vitvs_op_linear_big_grid reports them
PRODUCT_REACHED = frozenset([
    (192, 128, 0, 0), (192, 128, 0, 2), (192, 128, 0, 4), (192, 128, 1, 0), (192, 128, 1, 8),
    (192, 256, 0, 0), (192, 256, 0, 4), (192, 256, 1, 0), (192, 256, 1, 8),
    (256, 128, 0, 0), (256, 128, 0, 8), (256, 128, 1, 0), (256, 128, 1, 8),
    (256, 192, 0, 0), (256, 192, 0, 2), (256, 192, 0, 4), (256, 192, 0, 8), (256, 192, 1, 0), (256, 192, 1, 8),
    (256, 256, 0, 0), (256, 256, 0, 2), (256, 256, 0, 4), (256, 256, 0, 8), (256, 256, 1, 0), (256, 256, 1, 8)])

_TABLE = [
    # family, name, precision, hint, epilogue, variant, M, N, K, slices, dens, key, grid
    ('map', 'product-256x256-store-x2', 1, 1, 0, 256, 3709, 4608, 128, 0, 8, [1, 256, 256, 0, 0, 0, 0], [270, 256, 2, 2]),
    ('map', 'product-256x256-store-x4', 1, 1, 0, 256, 7293, 2304, 128, 0, 8, [1, 256, 256, 0, 0, 0, 0], [261, 256, 4, 2]),
    ('map', 'product-256x256-store-x8', 1, 1, 0, 256, 10877, 1536, 128, 0, 8, [1, 256, 256, 0, 0, 0, 0], [258, 256, 8, 2]),
    ('map', 'product-256x256-partial-x8', 1, 1, 1, 256, 10877, 512, 384, 3, 8, [1, 256, 256, 0, 0, 1, 0], [258, 256, 8, 2]),
    ('map', 'product-256x192-store-x2', 1, 1, 0, 192, 3197, 4032, 128, 0, 8, [1, 256, 192, 0, 0, 0, 0], [273, 256, 2, 2]),
    ('map', 'product-256x192-store-x4', 1, 1, 0, 192, 4477, 2880, 128, 0, 8, [1, 256, 192, 0, 0, 0, 0], [270, 256, 4, 2]),
    ('map', 'product-256x192-store-x8', 1, 1, 0, 192, 10877, 1152, 128, 0, 8, [1, 256, 192, 0, 0, 0, 0], [258, 256, 8, 2]),
    ('map', 'product-256x192-partial-x8', 1, 1, 1, 192, 10877, 384, 384, 3, 8, [1, 256, 192, 0, 0, 1, 0], [258, 256, 8, 2]),
    ('map', 'product-256x128-store-x8', 1, 1, 0, 128, 10877, 768, 128, 0, 8, [1, 256, 128, 0, 0, 0, 0], [258, 256, 8, 2]),
    ('map', 'product-256x128-partial-x8', 1, 1, 1, 128, 10877, 256, 384, 3, 8, [1, 256, 128, 0, 0, 1, 0], [258, 256, 8, 2]),
    ('map', 'product-192x128-store-x2', 1, 1, 0, 1192, 1629, 3712, 128, 0, 8, [1, 192, 128, 0, 0, 0, 0], [261, 256, 2, 2]),
    ('map', 'product-192x128-store-x4', 1, 1, 0, 1192, 3357, 1920, 128, 0, 8, [1, 192, 128, 0, 0, 0, 0], [270, 256, 4, 2]),
    ('map', 'product-192x128-partial-x8', 1, 1, 1, 1192, 8157, 256, 384, 3, 8, [1, 192, 128, 0, 0, 1, 0], [258, 256, 8, 2]),
    ('map', 'product-192x256-store-x4', 1, 1, 0, 1256, 5469, 2304, 128, 0, 8, [1, 192, 256, 0, 0, 0, 0], [261, 256, 4, 2]),
    ('map', 'product-192x256-partial-x8', 1, 1, 1, 1256, 8157, 512, 384, 3, 8, [1, 192, 256, 0, 0, 1, 0], [258, 256, 8, 2]),
    ('map', 'product-256x256-store-x8-fp16', 2, 1, 0, 256, 10877, 1536, 128, 0, 8, [1, 256, 256, 0, 0, 0, 0], [258, 256, 8, 2]),
    ('map', 'product-256x256-store-x8-f16x2', 3, 1, 0, 256, 10877, 1536, 64, 0, 8, [1, 256, 256, 0, 0, 0, 0], [258, 256, 8, 2]),
    ('map', 'product-256x256-partial-x8-f16x2', 3, 1, 1, 256, 10877, 512, 192, 3, 8, [1, 256, 256, 0, 0, 1, 0], [258, 256, 8, 2]),
    ('map', 'x1-256x192-store', 1, 1, 0, 192, 5245, 4224, 128, 0, 8, [1, 256, 192, 0, 0, 0, 0], [462, 256, 1, 2]),
    ('map', 'x1-256x128-store', 1, 1, 0, 128, 5245, 2816, 128, 0, 8, [1, 256, 128, 0, 0, 0, 0], [462, 256, 1, 2]),
    ('map', 'x1-192x128-store', 1, 1, 0, 1192, 3933, 2816, 128, 0, 8, [1, 192, 128, 0, 0, 0, 0], [462, 256, 1, 2]),
    ('map', 'uneven-256x128-store-x2', 1, 1, 0, 128, 2173, 3712, 128, 0, 8, [1, 256, 128, 0, 0, 0, 0], [261, 256, 2, 2]),
    ('map', 'uneven-256x128-store-x4', 1, 1, 0, 128, 3453, 2432, 128, 0, 8, [1, 256, 128, 0, 0, 0, 0], [266, 256, 4, 2]),
    ('map', 'uneven-192x256-store-x2', 1, 1, 0, 1256, 2781, 4608, 128, 0, 8, [1, 192, 256, 0, 0, 0, 0], [270, 256, 2, 2]),
    ('map', 'uneven-192x128-partial-x4', 1, 1, 1, 1192, 1437, 1408, 384, 3, 8, [1, 192, 128, 0, 0, 1, 0], [264, 256, 4, 2]),
    ('map', 'uneven-256x128-partial-x4', 2, 1, 1, 128, 2685, 1536, 256, 2, 8, [1, 256, 128, 0, 0, 1, 0], [264, 256, 4, 2]),
    ('map', 'onecol-192x128-partial-x8', 1, 1, 1, 1192, 16400, 128, 384, 3, 8, [1, 192, 128, 0, 0, 1, 0], [258, 256, 8, 2]),
    ('map', 'x0-3tiles-256x128', 1, 1, 0, 128, 600, 128, 128, 0, 8, [1, 256, 128, 0, 0, 0, 0], [3, 8, 0, 2]),
    ('map', 'x0-7tiles-192x128', 1, 1, 0, 1192, 1300, 128, 128, 0, 8, [1, 192, 128, 0, 0, 0, 0], [7, 8, 0, 2]),
    ('map', 'x0-9tiles-256x128', 1, 1, 0, 128, 700, 384, 128, 0, 8, [1, 256, 128, 0, 0, 0, 0], [9, 16, 0, 2]),
    ('map', 'x0-9tiles-256x256-partial', 1, 1, 1, 256, 700, 256, 384, 3, 8, [1, 256, 256, 0, 0, 1, 0], [9, 16, 0, 2]),
    ('map', 'x0-255tiles-256x128', 1, 1, 0, 128, 4300, 1920, 128, 0, 8, [1, 256, 128, 0, 0, 0, 0], [255, 256, 0, 2]),
    ('map', 'x0-256tiles-256x128', 1, 1, 0, 128, 4000, 2048, 128, 0, 8, [1, 256, 128, 0, 0, 0, 0], [256, 256, 0, 2]),
    ('map', 'x0-255tiles-192x128-partial', 1, 1, 1, 1192, 3200, 640, 384, 3, 8, [1, 192, 128, 0, 0, 1, 0], [255, 256, 0, 2]),
    ('map', 'x0-256tiles-256x256', 2, 1, 0, 256, 4000, 4096, 128, 0, 8, [1, 256, 256, 0, 0, 0, 0], [256, 256, 0, 2]),
    ('kloop', '64x64-st4-nk1', 1, 2, 0, 0, 70, 128, 64, 0, 8, [0, 64, 64, 1, 0, 0, 0], None),
    ('kloop', '64x64-st4-nk2', 1, 2, 0, 0, 70, 128, 128, 0, 8, [0, 64, 64, 1, 0, 0, 0], None),
    ('kloop', '64x64-st4-nk3', 1, 2, 0, 0, 70, 128, 192, 0, 8, [0, 64, 64, 1, 0, 0, 0], None),
    ('kloop', '64x64-st4-nk4', 1, 2, 0, 0, 70, 128, 256, 0, 8, [0, 64, 64, 1, 0, 0, 0], None),
    ('kloop', '64x64-st4-nk5', 1, 2, 0, 0, 70, 128, 320, 0, 8, [0, 64, 64, 1, 0, 0, 0], None),
    ('kloop', '64x64-st4-nk8', 1, 2, 0, 0, 70, 128, 512, 0, 8, [0, 64, 64, 1, 0, 0, 0], None),
    ('kloop', '64x64-st4-nk9', 1, 2, 0, 0, 70, 128, 576, 0, 8, [0, 64, 64, 1, 0, 0, 0], None),
    ('kloop', '64x64-st4-nk1-fp32', 0, 2, 0, 0, 70, 128, 32, 0, 8, [0, 64, 64, 1, 0, 0, 0], None),
    ('kloop', '64x64-st4-nk3-fp32', 0, 2, 0, 0, 70, 128, 96, 0, 8, [0, 64, 64, 1, 0, 0, 0], None),
    ('kloop', '64x64-st4-nk9-fp32', 0, 2, 0, 0, 70, 128, 288, 0, 8, [0, 64, 64, 1, 0, 0, 0], None),
    ('kloop', '64x64-st4-nk1-f16x2', 3, 2, 0, 0, 70, 128, 32, 0, 8, [0, 64, 64, 1, 0, 0, 0], None),
    ('kloop', '64x64-st4-nk3-f16x2', 3, 2, 0, 0, 70, 128, 96, 0, 8, [0, 64, 64, 1, 0, 0, 0], None),
    ('kloop', '64x64-st4-nk9-f16x2', 3, 2, 0, 0, 70, 128, 288, 0, 8, [0, 64, 64, 1, 0, 0, 0], None),
    ('kloop', '64x64-st4-nk1-fp16', 2, 2, 0, 0, 70, 128, 64, 0, 8, [0, 64, 64, 1, 0, 0, 0], None),
    ('kloop', '64x64-st4-nk3-fp16', 2, 2, 0, 0, 70, 128, 192, 0, 8, [0, 64, 64, 1, 0, 0, 0], None),
    ('kloop', '64x64-st4-nk9-fp16', 2, 2, 0, 0, 70, 128, 576, 0, 8, [0, 64, 64, 1, 0, 0, 0], None),
    ('kloop', '64x64-st3-nk1', 1, 1, 0, 0, 4097, 320, 64, 0, 8, [0, 64, 64, 1, 3, 0, 0], None),
    ('kloop', '64x64-st3-nk2', 1, 1, 0, 0, 4097, 320, 128, 0, 8, [0, 64, 64, 1, 3, 0, 0], None),
    ('kloop', '64x64-st3-nk3', 1, 1, 0, 0, 4097, 320, 192, 0, 8, [0, 64, 64, 1, 3, 0, 0], None),
    ('kloop', '64x64-st3-nk4', 1, 1, 0, 0, 4097, 320, 256, 0, 8, [0, 64, 64, 1, 3, 0, 0], None),
    ('kloop', '64x64-st3-nk5', 1, 1, 0, 0, 4097, 320, 320, 0, 8, [0, 64, 64, 1, 3, 0, 0], None),
    ('kloop', '64x64-st3-nk8', 1, 1, 0, 0, 4097, 320, 512, 0, 8, [0, 64, 64, 1, 3, 0, 0], None),
    ('kloop', '64x64-st3-nk9', 1, 1, 0, 0, 4097, 320, 576, 0, 8, [0, 64, 64, 1, 3, 0, 0], None),
    ('kloop', '64x64-st3-nk1-fp32', 0, 1, 0, 0, 4097, 320, 32, 0, 8, [0, 64, 64, 1, 3, 0, 0], None),
    ('kloop', '64x64-st3-nk3-fp32', 0, 1, 0, 0, 4097, 320, 96, 0, 8, [0, 64, 64, 1, 3, 0, 0], None),
    ('kloop', '64x64-st3-nk9-fp32', 0, 1, 0, 0, 4097, 320, 288, 0, 8, [0, 64, 64, 1, 3, 0, 0], None),
    ('kloop', '64x64-st3-nk1-f16x2', 3, 1, 0, 0, 4097, 320, 32, 0, 8, [0, 64, 64, 1, 3, 0, 0], None),
    ('kloop', '64x64-st3-nk3-f16x2', 3, 1, 0, 0, 4097, 320, 96, 0, 8, [0, 64, 64, 1, 3, 0, 0], None),
    ('kloop', '64x64-st3-nk9-f16x2', 3, 1, 0, 0, 4097, 320, 288, 0, 8, [0, 64, 64, 1, 3, 0, 0], None),
    ('kloop', '64x64-st3-nk1-fp16', 2, 1, 0, 0, 4097, 320, 64, 0, 8, [0, 64, 64, 1, 3, 0, 0], None),
    ('kloop', '64x64-st3-nk3-fp16', 2, 1, 0, 0, 4097, 320, 192, 0, 8, [0, 64, 64, 1, 3, 0, 0], None),
    ('kloop', '64x64-st3-nk9-fp16', 2, 1, 0, 0, 4097, 320, 576, 0, 8, [0, 64, 64, 1, 3, 0, 0], None),
    ('kloop', '64x64-st2-nk1', 1, 1, 0, 0, 4097, 576, 64, 0, 8, [0, 64, 64, 1, 2, 0, 0], None),
    ('kloop', '64x64-st2-nk2', 1, 1, 0, 0, 4097, 576, 128, 0, 8, [0, 64, 64, 1, 2, 0, 0], None),
    ('kloop', '64x64-st2-nk3', 1, 1, 0, 0, 4097, 576, 192, 0, 8, [0, 64, 64, 1, 2, 0, 0], None),
    ('kloop', '64x64-st2-nk4', 1, 1, 0, 0, 4097, 576, 256, 0, 8, [0, 64, 64, 1, 2, 0, 0], None),
    ('kloop', '64x64-st2-nk5', 1, 1, 0, 0, 4097, 576, 320, 0, 8, [0, 64, 64, 1, 2, 0, 0], None),
    ('kloop', '64x64-st2-nk8', 1, 1, 0, 0, 4097, 576, 512, 0, 8, [0, 64, 64, 1, 2, 0, 0], None),
    ('kloop', '64x64-st2-nk9', 1, 1, 0, 0, 4097, 576, 576, 0, 8, [0, 64, 64, 1, 2, 0, 0], None),
    ('kloop', '64x64-st2-nk1-fp32', 0, 1, 0, 0, 4097, 576, 32, 0, 8, [0, 64, 64, 1, 2, 0, 0], None),
    ('kloop', '64x64-st2-nk3-fp32', 0, 1, 0, 0, 4097, 576, 96, 0, 8, [0, 64, 64, 1, 2, 0, 0], None),
    ('kloop', '64x64-st2-nk9-fp32', 0, 1, 0, 0, 4097, 576, 288, 0, 8, [0, 64, 64, 1, 2, 0, 0], None),
    ('kloop', '64x64-st2-nk1-f16x2', 3, 1, 0, 0, 4097, 576, 32, 0, 8, [0, 64, 64, 1, 2, 0, 0], None),
    ('kloop', '64x64-st2-nk3-f16x2', 3, 1, 0, 0, 4097, 576, 96, 0, 8, [0, 64, 64, 1, 2, 0, 0], None),
    ('kloop', '64x64-st2-nk9-f16x2', 3, 1, 0, 0, 4097, 576, 288, 0, 8, [0, 64, 64, 1, 2, 0, 0], None),
    ('kloop', '64x64-st2-nk1-fp16', 2, 1, 0, 0, 4097, 576, 64, 0, 8, [0, 64, 64, 1, 2, 0, 0], None),
    ('kloop', '64x64-st2-nk3-fp16', 2, 1, 0, 0, 4097, 576, 192, 0, 8, [0, 64, 64, 1, 2, 0, 0], None),
    ('kloop', '64x64-st2-nk9-fp16', 2, 1, 0, 0, 4097, 576, 576, 0, 8, [0, 64, 64, 1, 2, 0, 0], None),
    ('kloop', '64x128-st2-nk1', 1, 1, 0, 0, 4097, 512, 64, 0, 8, [0, 64, 128, 1, 2, 0, 0], None),
    ('kloop', '64x96-st4-nk1', 1, 2, 0, 0, 70, 8448, 64, 0, 8, [0, 64, 96, 1, 0, 0, 0], None),
    ('kloop', '64x128-st2-nk2', 1, 1, 0, 0, 4097, 512, 128, 0, 8, [0, 64, 128, 1, 2, 0, 0], None),
    ('kloop', '64x96-st4-nk2', 1, 2, 0, 0, 70, 8448, 128, 0, 8, [0, 64, 96, 1, 0, 0, 0], None),
    ('kloop', '64x128-st2-nk3', 1, 1, 0, 0, 4097, 512, 192, 0, 8, [0, 64, 128, 1, 2, 0, 0], None),
    ('kloop', '64x96-st4-nk3', 1, 2, 0, 0, 70, 8448, 192, 0, 8, [0, 64, 96, 1, 0, 0, 0], None),
    ('kloop', '64x128-st2-nk5', 1, 1, 0, 0, 4097, 512, 320, 0, 8, [0, 64, 128, 1, 2, 0, 0], None),
    ('kloop', '64x96-st4-nk5', 1, 2, 0, 0, 70, 8448, 320, 0, 8, [0, 64, 96, 1, 0, 0, 0], None),
    ('kloop', '64x128-st2-nk9', 1, 1, 0, 0, 4097, 512, 576, 0, 8, [0, 64, 128, 1, 2, 0, 0], None),
    ('kloop', '64x96-st4-nk9', 1, 2, 0, 0, 70, 8448, 576, 0, 8, [0, 64, 96, 1, 0, 0, 0], None),
    ('kloop', '64x64-kg2-nk4-bf16', 1, 1, 0, 0, 70, 128, 256, 0, 8, [0, 64, 64, 2, 0, 0, 0], None),
    ('kloop', '64x64-kg2-partial-nk4-bf16', 1, 1, 1, 0, 70, 128, 512, 2, 8, [0, 64, 64, 2, 0, 1, 0], None),
    ('kloop', '64x64-kg2-nk4-fp32', 0, 1, 0, 0, 70, 128, 128, 0, 8, [0, 64, 64, 2, 0, 0, 0], None),
    ('kloop', '64x64-kg2-partial-nk4-fp32', 0, 1, 1, 0, 70, 128, 256, 2, 8, [0, 64, 64, 2, 0, 1, 0], None),
    ('kloop', '64x64-kg2-nk4-f16x2', 3, 1, 0, 0, 70, 128, 128, 0, 8, [0, 64, 64, 2, 0, 0, 0], None),
    ('kloop', '64x64-kg2-partial-nk4-f16x2', 3, 1, 1, 0, 70, 128, 256, 2, 8, [0, 64, 64, 2, 0, 1, 0], None),
    ('kloop', '64x96-kg2-nk4', 1, 1, 0, 0, 70, 8448, 256, 0, 8, [0, 64, 96, 2, 0, 0, 0], None),
    ('kloop', '64x128-kg2-nk4', 1, 1, 0, 0, 70, 8320, 256, 0, 8, [0, 64, 128, 2, 0, 0, 0], None),
    ('kloop', '64x64-kg2-nk6-bf16', 1, 1, 0, 0, 70, 128, 384, 0, 8, [0, 64, 64, 2, 0, 0, 0], None),
    ('kloop', '64x64-kg2-partial-nk6-bf16', 1, 1, 1, 0, 70, 128, 768, 2, 8, [0, 64, 64, 2, 0, 1, 0], None),
    ('kloop', '64x64-kg2-nk6-fp32', 0, 1, 0, 0, 70, 128, 192, 0, 8, [0, 64, 64, 2, 0, 0, 0], None),
    ('kloop', '64x64-kg2-partial-nk6-fp32', 0, 1, 1, 0, 70, 128, 384, 2, 8, [0, 64, 64, 2, 0, 1, 0], None),
    ('kloop', '64x64-kg2-nk6-f16x2', 3, 1, 0, 0, 70, 128, 192, 0, 8, [0, 64, 64, 2, 0, 0, 0], None),
    ('kloop', '64x64-kg2-partial-nk6-f16x2', 3, 1, 1, 0, 70, 128, 384, 2, 8, [0, 64, 64, 2, 0, 1, 0], None),
    ('kloop', '64x96-kg2-nk6', 1, 1, 0, 0, 70, 8448, 384, 0, 8, [0, 64, 96, 2, 0, 0, 0], None),
    ('kloop', '64x128-kg2-nk6', 1, 1, 0, 0, 70, 8320, 384, 0, 8, [0, 64, 128, 2, 0, 0, 0], None),
    ('kloop', '64x64-kg2-nk8-bf16', 1, 1, 0, 0, 70, 128, 512, 0, 8, [0, 64, 64, 2, 0, 0, 0], None),
    ('kloop', '64x64-kg2-partial-nk8-bf16', 1, 1, 1, 0, 70, 128, 1024, 2, 8, [0, 64, 64, 2, 0, 1, 0], None),
    ('kloop', '64x64-kg2-nk8-fp32', 0, 1, 0, 0, 70, 128, 256, 0, 8, [0, 64, 64, 2, 0, 0, 0], None),
    ('kloop', '64x64-kg2-partial-nk8-fp32', 0, 1, 1, 0, 70, 128, 512, 2, 8, [0, 64, 64, 2, 0, 1, 0], None),
    ('kloop', '64x64-kg2-nk8-f16x2', 3, 1, 0, 0, 70, 128, 256, 0, 8, [0, 64, 64, 2, 0, 0, 0], None),
    ('kloop', '64x64-kg2-partial-nk8-f16x2', 3, 1, 1, 0, 70, 128, 512, 2, 8, [0, 64, 64, 2, 0, 1, 0], None),
    ('kloop', '64x96-kg2-nk8', 1, 1, 0, 0, 70, 8448, 512, 0, 8, [0, 64, 96, 2, 0, 0, 0], None),
    ('kloop', '64x128-kg2-nk8', 1, 1, 0, 0, 70, 8320, 512, 0, 8, [0, 64, 128, 2, 0, 0, 0], None),
    ('kloop', 'big256x256-nk2', 1, 1, 1, 256, 293, 512, 256, 2, 8, [1, 256, 256, 0, 0, 1, 0], [8, 8, 0, 2]),
    ('kloop', 'big256x256-nk3', 1, 1, 1, 256, 293, 512, 384, 2, 8, [1, 256, 256, 0, 0, 1, 0], [8, 8, 0, 3]),
    ('kloop', 'big256x256-nk4', 1, 1, 1, 256, 293, 512, 512, 2, 8, [1, 256, 256, 0, 0, 1, 0], [8, 8, 0, 4]),
    ('kloop', 'big256x256-nk5', 1, 1, 1, 256, 293, 512, 640, 2, 8, [1, 256, 256, 0, 0, 1, 0], [8, 8, 0, 5]),
    ('kloop', 'big256x256-nk3-f16x2', 3, 1, 1, 256, 293, 512, 192, 2, 8, [1, 256, 256, 0, 0, 1, 0], [8, 8, 0, 3]),
    ('kloop', 'big256x192-nk2', 1, 1, 1, 192, 293, 384, 256, 2, 8, [1, 256, 192, 0, 0, 1, 0], [8, 8, 0, 2]),
    ('kloop', 'big256x192-nk3', 1, 1, 1, 192, 293, 384, 384, 2, 8, [1, 256, 192, 0, 0, 1, 0], [8, 8, 0, 3]),
    ('kloop', 'big256x192-nk4', 1, 1, 1, 192, 293, 384, 512, 2, 8, [1, 256, 192, 0, 0, 1, 0], [8, 8, 0, 4]),
    ('kloop', 'big256x192-nk5', 1, 1, 1, 192, 293, 384, 640, 2, 8, [1, 256, 192, 0, 0, 1, 0], [8, 8, 0, 5]),
    ('kloop', 'big256x192-nk3-f16x2', 3, 1, 1, 192, 293, 384, 192, 2, 8, [1, 256, 192, 0, 0, 1, 0], [8, 8, 0, 3]),
    ('kloop', 'big256x128-nk2', 1, 1, 1, 128, 293, 256, 256, 2, 8, [1, 256, 128, 0, 0, 1, 0], [8, 8, 0, 2]),
    ('kloop', 'big256x128-nk3', 1, 1, 1, 128, 293, 256, 384, 2, 8, [1, 256, 128, 0, 0, 1, 0], [8, 8, 0, 3]),
    ('kloop', 'big256x128-nk4', 1, 1, 1, 128, 293, 256, 512, 2, 8, [1, 256, 128, 0, 0, 1, 0], [8, 8, 0, 4]),
    ('kloop', 'big256x128-nk5', 1, 1, 1, 128, 293, 256, 640, 2, 8, [1, 256, 128, 0, 0, 1, 0], [8, 8, 0, 5]),
    ('kloop', 'big256x128-nk3-f16x2', 3, 1, 1, 128, 293, 256, 192, 2, 8, [1, 256, 128, 0, 0, 1, 0], [8, 8, 0, 3]),
    ('kloop', 'big192x128-nk2', 1, 1, 1, 1192, 229, 256, 256, 2, 8, [1, 192, 128, 0, 0, 1, 0], [8, 8, 0, 2]),
    ('kloop', 'big192x128-nk3', 1, 1, 1, 1192, 229, 256, 384, 2, 8, [1, 192, 128, 0, 0, 1, 0], [8, 8, 0, 3]),
    ('kloop', 'big192x128-nk4', 1, 1, 1, 1192, 229, 256, 512, 2, 8, [1, 192, 128, 0, 0, 1, 0], [8, 8, 0, 4]),
    ('kloop', 'big192x128-nk5', 1, 1, 1, 1192, 229, 256, 640, 2, 8, [1, 192, 128, 0, 0, 1, 0], [8, 8, 0, 5]),
    ('kloop', 'big192x128-nk3-f16x2', 3, 1, 1, 1192, 229, 256, 192, 2, 8, [1, 192, 128, 0, 0, 1, 0], [8, 8, 0, 3]),
    ('kloop', 'big192x256-nk2', 1, 1, 1, 1256, 229, 512, 256, 2, 8, [1, 192, 256, 0, 0, 1, 0], [8, 8, 0, 2]),
    ('kloop', 'big192x256-nk3', 1, 1, 1, 1256, 229, 512, 384, 2, 8, [1, 192, 256, 0, 0, 1, 0], [8, 8, 0, 3]),
    ('kloop', 'big192x256-nk4', 1, 1, 1, 1256, 229, 512, 512, 2, 8, [1, 192, 256, 0, 0, 1, 0], [8, 8, 0, 4]),
    ('kloop', 'big192x256-nk5', 1, 1, 1, 1256, 229, 512, 640, 2, 8, [1, 192, 256, 0, 0, 1, 0], [8, 8, 0, 5]),
    ('kloop', 'big192x256-nk3-f16x2', 3, 1, 1, 1256, 229, 512, 192, 2, 8, [1, 192, 256, 0, 0, 1, 0], [8, 8, 0, 3]),
    ('kloop', 'big256x128-nk255', 1, 1, 1, 128, 293, 256, 16320, 1, 32, [1, 256, 128, 0, 0, 0, 0], [4, 8, 0, 255]),
    ('kloop', 'big192x128-nk255-f16x2', 3, 1, 1, 1192, 229, 256, 8160, 1, 32, [1, 192, 128, 0, 0, 0, 0], [4, 8, 0, 255]),
    ('slices', '64x64-s2-bf16', 1, 1, 1, 0, 131, 128, 384, 2, 8, [0, 64, 64, 1, 0, 1, 0], None),
    ('slices', '64x64-s3-bf16', 1, 1, 1, 0, 131, 128, 576, 3, 8, [0, 64, 64, 1, 0, 1, 0], None),
    ('slices', '64x64-s4-bf16', 1, 1, 1, 0, 131, 128, 768, 4, 8, [0, 64, 64, 1, 0, 1, 0], None),
    ('slices', '64x64-s6-bf16', 1, 1, 1, 0, 131, 128, 1152, 6, 8, [0, 64, 64, 1, 0, 1, 0], None),
    ('slices', '64x64-s8-bf16', 1, 1, 1, 0, 131, 128, 1536, 8, 8, [0, 64, 64, 1, 0, 1, 0], None),
    ('slices', '64x64-s2-fp16', 2, 1, 1, 0, 131, 128, 384, 2, 8, [0, 64, 64, 1, 0, 1, 0], None),
    ('slices', '64x64-s3-fp16', 2, 1, 1, 0, 131, 128, 576, 3, 8, [0, 64, 64, 1, 0, 1, 0], None),
    ('slices', '64x64-s4-fp16', 2, 1, 1, 0, 131, 128, 768, 4, 8, [0, 64, 64, 1, 0, 1, 0], None),
    ('slices', '64x64-s6-fp16', 2, 1, 1, 0, 131, 128, 1152, 6, 8, [0, 64, 64, 1, 0, 1, 0], None),
    ('slices', '64x64-s8-fp16', 2, 1, 1, 0, 131, 128, 1536, 8, 8, [0, 64, 64, 1, 0, 1, 0], None),
    ('slices', '64x64-s2-f16x2', 3, 1, 1, 0, 131, 128, 192, 2, 8, [0, 64, 64, 1, 0, 1, 0], None),
    ('slices', '64x64-s3-f16x2', 3, 1, 1, 0, 131, 128, 288, 3, 8, [0, 64, 64, 1, 0, 1, 0], None),
    ('slices', '64x64-s4-f16x2', 3, 1, 1, 0, 131, 128, 384, 4, 8, [0, 64, 64, 1, 0, 1, 0], None),
    ('slices', '64x64-s6-f16x2', 3, 1, 1, 0, 131, 128, 576, 6, 8, [0, 64, 64, 1, 0, 1, 0], None),
    ('slices', '64x64-s8-f16x2', 3, 1, 1, 0, 131, 128, 768, 8, 8, [0, 64, 64, 1, 0, 1, 0], None),
    ('slices', '64x64-s2-fp32', 0, 1, 1, 0, 131, 128, 192, 2, 8, [0, 64, 64, 1, 0, 1, 0], None),
    ('slices', '64x64-s3-fp32', 0, 1, 1, 0, 131, 128, 288, 3, 8, [0, 64, 64, 1, 0, 1, 0], None),
    ('slices', '64x64-s4-fp32', 0, 1, 1, 0, 131, 128, 384, 4, 8, [0, 64, 64, 1, 0, 1, 0], None),
    ('slices', '64x64-s6-fp32', 0, 1, 1, 0, 131, 128, 576, 6, 8, [0, 64, 64, 1, 0, 1, 0], None),
    ('slices', '64x64-s8-fp32', 0, 1, 1, 0, 131, 128, 768, 8, 8, [0, 64, 64, 1, 0, 1, 0], None),
    ('slices', 'big256x256-s2', 1, 1, 1, 256, 317, 256, 256, 2, 8, [1, 256, 256, 0, 0, 1, 0], [4, 8, 0, 2]),
    ('slices', 'big256x256-s3', 1, 1, 1, 256, 317, 256, 384, 3, 8, [1, 256, 256, 0, 0, 1, 0], [6, 8, 0, 2]),
    ('slices', 'big256x256-s4', 1, 1, 1, 256, 317, 256, 512, 4, 8, [1, 256, 256, 0, 0, 1, 0], [8, 8, 0, 2]),
    ('slices', 'big256x256-s3-f16x2', 3, 1, 1, 256, 317, 256, 192, 3, 8, [1, 256, 256, 0, 0, 1, 0], [6, 8, 0, 2]),
    ('slices', 'big256x192-s2', 1, 1, 1, 192, 317, 384, 256, 2, 8, [1, 256, 192, 0, 0, 1, 0], [8, 8, 0, 2]),
    ('slices', 'big256x192-s3', 1, 1, 1, 192, 317, 384, 384, 3, 8, [1, 256, 192, 0, 0, 1, 0], [12, 16, 0, 2]),
    ('slices', 'big256x192-s4', 1, 1, 1, 192, 317, 384, 512, 4, 8, [1, 256, 192, 0, 0, 1, 0], [16, 16, 0, 2]),
    ('slices', 'big256x192-s3-f16x2', 3, 1, 1, 192, 317, 384, 192, 3, 8, [1, 256, 192, 0, 0, 1, 0], [12, 16, 0, 2]),
    ('slices', 'big256x128-s2', 1, 1, 1, 128, 317, 256, 256, 2, 8, [1, 256, 128, 0, 0, 1, 0], [8, 8, 0, 2]),
    ('slices', 'big256x128-s3', 1, 1, 1, 128, 317, 256, 384, 3, 8, [1, 256, 128, 0, 0, 1, 0], [12, 16, 0, 2]),
    ('slices', 'big256x128-s4', 1, 1, 1, 128, 317, 256, 512, 4, 8, [1, 256, 128, 0, 0, 1, 0], [16, 16, 0, 2]),
    ('slices', 'big256x128-s3-f16x2', 3, 1, 1, 128, 317, 256, 192, 3, 8, [1, 256, 128, 0, 0, 1, 0], [12, 16, 0, 2]),
    ('slices', 'big192x128-s2', 1, 1, 1, 1192, 253, 256, 256, 2, 8, [1, 192, 128, 0, 0, 1, 0], [8, 8, 0, 2]),
    ('slices', 'big192x128-s3', 1, 1, 1, 1192, 253, 256, 384, 3, 8, [1, 192, 128, 0, 0, 1, 0], [12, 16, 0, 2]),
    ('slices', 'big192x128-s4', 1, 1, 1, 1192, 253, 256, 512, 4, 8, [1, 192, 128, 0, 0, 1, 0], [16, 16, 0, 2]),
    ('slices', 'big192x128-s3-f16x2', 3, 1, 1, 1192, 253, 256, 192, 3, 8, [1, 192, 128, 0, 0, 1, 0], [12, 16, 0, 2]),
    ('slices', 'big192x256-s2', 1, 1, 1, 1256, 253, 256, 256, 2, 8, [1, 192, 256, 0, 0, 1, 0], [4, 8, 0, 2]),
    ('slices', 'big192x256-s3', 1, 1, 1, 1256, 253, 256, 384, 3, 8, [1, 192, 256, 0, 0, 1, 0], [6, 8, 0, 2]),
    ('slices', 'big192x256-s4', 1, 1, 1, 1256, 253, 256, 512, 4, 8, [1, 192, 256, 0, 0, 1, 0], [8, 8, 0, 2]),
    ('slices', 'big192x256-s3-f16x2', 3, 1, 1, 1256, 253, 256, 192, 3, 8, [1, 192, 256, 0, 0, 1, 0], [6, 8, 0, 2]),
    ('slices', 'xcd-nx4-ny1', 1, 2, 1, 0, 61, 256, 384, 2, 8, [0, 64, 64, 1, 0, 1, 1], None),
    ('slices', 'xcd-nx4-ny2', 1, 2, 1, 0, 100, 256, 384, 2, 8, [0, 64, 64, 1, 0, 1, 1], None),
    ('slices', 'xcd-nx4-ny3', 1, 2, 1, 0, 131, 256, 384, 2, 8, [0, 64, 64, 1, 0, 1, 1], None),
    ('slices', 'xcd-nx8-ny1', 1, 2, 1, 0, 61, 512, 384, 2, 8, [0, 64, 64, 1, 0, 1, 1], None),
    ('slices', 'xcd-nx8-ny2', 1, 2, 1, 0, 100, 512, 384, 2, 8, [0, 64, 64, 1, 0, 1, 1], None),
    ('slices', 'xcd-nx8-ny3', 1, 2, 1, 0, 131, 512, 384, 2, 8, [0, 64, 64, 1, 0, 1, 1], None),
    ('slices', 'xcd-nx12-ny1', 1, 2, 1, 0, 61, 768, 384, 2, 8, [0, 64, 64, 1, 0, 1, 1], None),
    ('slices', 'xcd-nx12-ny2', 1, 2, 1, 0, 100, 768, 384, 2, 8, [0, 64, 64, 1, 0, 1, 1], None),
    ('slices', 'xcd-nx12-ny3', 1, 2, 1, 0, 131, 768, 384, 2, 8, [0, 64, 64, 1, 0, 1, 1], None),
    ('slices', 'xcd-nx12-ny3-fp32', 0, 3, 1, 0, 131, 768, 256, 2, 8, [0, 64, 64, 1, 0, 1, 1], None),
    ('slices', 'xcd-nx12-ny3-fp16', 2, 3, 1, 0, 131, 768, 512, 2, 8, [0, 64, 64, 1, 0, 1, 1], None),
    ('slices', 'xcd-nx12-ny3-f16x2', 3, 3, 1, 0, 131, 768, 256, 2, 8, [0, 64, 64, 1, 0, 1, 1], None),
    ('keys', 'fp32-store-gemm64x96-kg1-st0-one', 0, 1, 0, 0, 700, 1536, 32, 0, 8, [0, 64, 96, 1, 0, 0, 0], None),
    ('keys', 'fp32-store-gemm64x96-kg2-st0-one', 0, 1, 0, 0, 700, 1536, 128, 0, 8, [0, 64, 96, 2, 0, 0, 0], None),
    ('keys', 'fp32-store-gemm64x128-kg1-st0-one', 0, 1, 0, 0, 4097, 256, 32, 0, 8, [0, 64, 128, 1, 0, 0, 0], None),
    ('keys', 'fp32-store-gemm64x128-kg1-st2-one', 0, 1, 0, 0, 4097, 512, 32, 0, 8, [0, 64, 128, 1, 2, 0, 0], None),
    ('keys', 'fp32-store-gemm64x128-kg2-st0-one', 0, 1, 0, 0, 4097, 256, 128, 0, 8, [0, 64, 128, 2, 0, 0, 0], None),
    ('keys', 'fp32-store-gemm128x128-kg1-st0-one', 0, 1, 0, 0, 1300, 3072, 32, 0, 8, [0, 128, 128, 1, 0, 0, 0], None),
    ('keys', 'fp32-partial-gemm64x64-kg1-st0-one', 0, 1, 1, 0, 1, 64, 32, 1, 8, [0, 64, 64, 1, 0, 0, 0], None),
    ('keys', 'fp32-partial-gemm64x64-kg1-st2-one', 0, 1, 1, 0, 4097, 512, 32, 1, 8, [0, 64, 64, 1, 2, 0, 0], None),
    ('keys', 'fp32-partial-gemm64x64-kg1-st3-one', 0, 1, 1, 0, 4097, 256, 32, 1, 8, [0, 64, 64, 1, 3, 0, 0], None),
    ('keys', 'fp32-partial-gemm64x64-kg2-st0-one', 0, 1, 1, 0, 1, 64, 128, 1, 8, [0, 64, 64, 2, 0, 0, 0], None),
    ('keys', 'fp32-partial-gemm128x128-kg1-st0-one', 0, 1, 1, 0, 1300, 3072, 32, 1, 8, [0, 128, 128, 1, 0, 0, 0], None),
    ('keys', 'bf16-store-gemm64x128-kg1-st0-one', 1, 1, 0, 0, 4097, 256, 64, 0, 8, [0, 64, 128, 1, 0, 0, 0], None),
    ('keys', 'bf16-store-big192x128-kg0-st0-one', 1, 1, 0, 0, 1100, 2304, 128, 0, 8, [1, 192, 128, 0, 0, 0, 0], [108, 112, 0, 2]),
    ('keys', 'bf16-store-big192x256-kg0-st0-one', 1, 1, 0, 0, 4097, 2048, 128, 0, 8, [1, 192, 256, 0, 0, 0, 0], [176, 176, 0, 2]),
    ('keys', 'bf16-store-big256x128-kg0-st0-one', 1, 1, 0, 0, 6145, 1024, 128, 0, 8, [1, 256, 128, 0, 0, 0, 0], [200, 200, 0, 2]),
    ('keys', 'bf16-store-big256x192-kg0-st0-one', 1, 1, 0, 0, 2561, 3072, 128, 0, 8, [1, 256, 192, 0, 0, 0, 0], [176, 176, 0, 2]),
    ('keys', 'bf16-store-big256x256-kg0-st0-one', 1, 2, 0, 0, 5121, 512, 128, 0, 8, [1, 256, 256, 0, 0, 0, 0], [42, 48, 0, 2]),
    ('keys', 'bf16-partial-gemm64x64-kg1-st0-one', 1, 1, 1, 0, 1, 64, 64, 1, 8, [0, 64, 64, 1, 0, 0, 0], None),
    ('keys', 'bf16-partial-gemm64x64-kg1-st2-one', 1, 1, 1, 0, 4097, 512, 64, 1, 8, [0, 64, 64, 1, 2, 0, 0], None),
    ('keys', 'bf16-partial-gemm64x64-kg1-st2-slices', 1, 1, 1, 0, 4097, 256, 1024, 2, 8, [0, 64, 64, 1, 2, 1, 0], None),
    ('keys', 'bf16-partial-gemm64x64-kg1-st2-slices-xcd', 1, 2, 1, 0, 4097, 256, 1024, 2, 8, [0, 64, 64, 1, 2, 1, 1], None),
    ('keys', 'bf16-partial-gemm64x64-kg1-st3-one', 1, 1, 1, 0, 4097, 256, 64, 1, 8, [0, 64, 64, 1, 3, 0, 0], None),
    ('keys', 'bf16-partial-gemm64x64-kg1-st3-slices', 1, 1, 1, 0, 4097, 128, 1024, 2, 8, [0, 64, 64, 1, 3, 1, 0], None),
    ('keys', 'bf16-partial-gemm64x64-kg2-st0-one', 1, 1, 1, 0, 1, 64, 256, 1, 8, [0, 64, 64, 2, 0, 0, 0], None),
    ('keys', 'bf16-partial-big192x128-kg0-st0-one', 1, 1, 1, 0, 513, 4096, 128, 1, 8, [1, 192, 128, 0, 0, 0, 0], [96, 96, 0, 2]),
    ('keys', 'bf16-partial-big192x128-kg0-st0-slices', 1, 1, 1, 0, 1300, 1024, 1024, 2, 8, [1, 192, 128, 0, 0, 1, 0], [112, 112, 0, 8]),
    ('keys', 'bf16-partial-big192x256-kg0-st0-one', 1, 1, 1, 0, 4097, 2048, 128, 1, 8, [1, 192, 256, 0, 0, 0, 0], [176, 176, 0, 2]),
    ('keys', 'bf16-partial-big256x128-kg0-st0-one', 1, 1, 1, 0, 6145, 1024, 128, 1, 8, [1, 256, 128, 0, 0, 0, 0], [200, 200, 0, 2]),
    ('keys', 'bf16-partial-big256x128-kg0-st0-slices', 1, 1, 1, 0, 4097, 512, 1536, 3, 8, [1, 256, 128, 0, 0, 1, 0], [204, 208, 0, 8]),
    ('keys', 'bf16-partial-big256x192-kg0-st0-one', 1, 1, 1, 0, 2561, 3072, 128, 1, 8, [1, 256, 192, 0, 0, 0, 0], [176, 176, 0, 2]),
    ('keys', 'bf16-partial-big256x256-kg0-st0-one', 1, 2, 1, 0, 6145, 512, 128, 1, 8, [1, 256, 256, 0, 0, 0, 0], [50, 56, 0, 2]),
    ('keys', 'bf16-partial-big256x256-kg0-st0-slices', 1, 2, 1, 0, 6145, 256, 1024, 2, 8, [1, 256, 256, 0, 0, 1, 0], [50, 56, 0, 8]),
    ('keys', 'fp16-store-gemm64x64-kg2-st0-one', 2, 1, 0, 0, 1, 64, 256, 0, 8, [0, 64, 64, 2, 0, 0, 0], None),
    ('keys', 'fp16-store-gemm64x96-kg1-st0-one', 2, 1, 0, 0, 700, 1536, 64, 0, 8, [0, 64, 96, 1, 0, 0, 0], None),
    ('keys', 'fp16-store-gemm64x96-kg2-st0-one', 2, 1, 0, 0, 700, 1536, 256, 0, 8, [0, 64, 96, 2, 0, 0, 0], None),
    ('keys', 'fp16-store-gemm64x128-kg1-st0-one', 2, 1, 0, 0, 4097, 256, 64, 0, 8, [0, 64, 128, 1, 0, 0, 0], None),
    ('keys', 'fp16-store-gemm64x128-kg1-st2-one', 2, 1, 0, 0, 4097, 512, 64, 0, 8, [0, 64, 128, 1, 2, 0, 0], None),
    ('keys', 'fp16-store-gemm64x128-kg2-st0-one', 2, 1, 0, 0, 4097, 256, 256, 0, 8, [0, 64, 128, 2, 0, 0, 0], None),
    ('keys', 'fp16-store-big192x128-kg0-st0-one', 2, 1, 0, 0, 1100, 2304, 128, 0, 8, [1, 192, 128, 0, 0, 0, 0], [108, 112, 0, 2]),
    ('keys', 'fp16-store-big192x256-kg0-st0-one', 2, 1, 0, 0, 4097, 2048, 128, 0, 8, [1, 192, 256, 0, 0, 0, 0], [176, 176, 0, 2]),
    ('keys', 'fp16-store-big256x128-kg0-st0-one', 2, 1, 0, 0, 6145, 1024, 128, 0, 8, [1, 256, 128, 0, 0, 0, 0], [200, 200, 0, 2]),
    ('keys', 'fp16-store-big256x192-kg0-st0-one', 2, 1, 0, 0, 2561, 3072, 128, 0, 8, [1, 256, 192, 0, 0, 0, 0], [176, 176, 0, 2]),
    ('keys', 'fp16-store-big256x256-kg0-st0-one', 2, 2, 0, 0, 5121, 512, 128, 0, 8, [1, 256, 256, 0, 0, 0, 0], [42, 48, 0, 2]),
    ('keys', 'fp16-partial-gemm64x64-kg1-st0-one', 2, 1, 1, 0, 1, 64, 64, 1, 8, [0, 64, 64, 1, 0, 0, 0], None),
    ('keys', 'fp16-partial-gemm64x64-kg1-st2-one', 2, 1, 1, 0, 4097, 512, 64, 1, 8, [0, 64, 64, 1, 2, 0, 0], None),
    ('keys', 'fp16-partial-gemm64x64-kg1-st2-slices', 2, 1, 1, 0, 4097, 256, 1024, 2, 8, [0, 64, 64, 1, 2, 1, 0], None),
    ('keys', 'fp16-partial-gemm64x64-kg1-st2-slices-xcd', 2, 2, 1, 0, 4097, 256, 1024, 2, 8, [0, 64, 64, 1, 2, 1, 1], None),
    ('keys', 'fp16-partial-gemm64x64-kg1-st3-one', 2, 1, 1, 0, 4097, 256, 64, 1, 8, [0, 64, 64, 1, 3, 0, 0], None),
    ('keys', 'fp16-partial-gemm64x64-kg1-st3-slices', 2, 1, 1, 0, 4097, 128, 1024, 2, 8, [0, 64, 64, 1, 3, 1, 0], None),
    ('keys', 'fp16-partial-gemm64x64-kg2-st0-one', 2, 1, 1, 0, 1, 64, 256, 1, 8, [0, 64, 64, 2, 0, 0, 0], None),
    ('keys', 'fp16-partial-gemm64x64-kg2-st0-slices', 2, 1, 1, 0, 1, 64, 512, 2, 8, [0, 64, 64, 2, 0, 1, 0], None),
    ('keys', 'fp16-partial-big192x128-kg0-st0-one', 2, 1, 1, 0, 513, 4096, 128, 1, 8, [1, 192, 128, 0, 0, 0, 0], [96, 96, 0, 2]),
    ('keys', 'fp16-partial-big192x128-kg0-st0-slices', 2, 1, 1, 0, 1300, 1024, 1024, 2, 8, [1, 192, 128, 0, 0, 1, 0], [112, 112, 0, 8]),
    ('keys', 'fp16-partial-big192x256-kg0-st0-one', 2, 1, 1, 0, 4097, 2048, 128, 1, 8, [1, 192, 256, 0, 0, 0, 0], [176, 176, 0, 2]),
    ('keys', 'fp16-partial-big256x128-kg0-st0-one', 2, 1, 1, 0, 6145, 1024, 128, 1, 8, [1, 256, 128, 0, 0, 0, 0], [200, 200, 0, 2]),
    ('keys', 'fp16-partial-big256x128-kg0-st0-slices', 2, 1, 1, 0, 4097, 512, 1536, 3, 8, [1, 256, 128, 0, 0, 1, 0], [204, 208, 0, 8]),
    ('keys', 'fp16-partial-big256x192-kg0-st0-one', 2, 1, 1, 0, 2561, 3072, 128, 1, 8, [1, 256, 192, 0, 0, 0, 0], [176, 176, 0, 2]),
    ('keys', 'fp16-partial-big256x256-kg0-st0-one', 2, 2, 1, 0, 6145, 512, 128, 1, 8, [1, 256, 256, 0, 0, 0, 0], [50, 56, 0, 2]),
    ('keys', 'fp16-partial-big256x256-kg0-st0-slices', 2, 2, 1, 0, 6145, 256, 1024, 2, 8, [1, 256, 256, 0, 0, 1, 0], [50, 56, 0, 8]),
    ('keys', 'f16x2-store-gemm64x96-kg1-st0-one', 3, 1, 0, 0, 700, 1536, 32, 0, 8, [0, 64, 96, 1, 0, 0, 0], None),
    ('keys', 'f16x2-store-gemm64x96-kg2-st0-one', 3, 1, 0, 0, 700, 1536, 128, 0, 8, [0, 64, 96, 2, 0, 0, 0], None),
    ('keys', 'f16x2-store-gemm64x128-kg1-st0-one', 3, 1, 0, 0, 4097, 256, 32, 0, 8, [0, 64, 128, 1, 0, 0, 0], None),
    ('keys', 'f16x2-store-gemm64x128-kg1-st2-one', 3, 1, 0, 0, 4097, 512, 32, 0, 8, [0, 64, 128, 1, 2, 0, 0], None),
    ('keys', 'f16x2-store-gemm64x128-kg2-st0-one', 3, 1, 0, 0, 4097, 256, 128, 0, 8, [0, 64, 128, 2, 0, 0, 0], None),
    ('keys', 'f16x2-store-big192x128-kg0-st0-one', 3, 1, 0, 0, 1100, 2304, 64, 0, 8, [1, 192, 128, 0, 0, 0, 0], [108, 112, 0, 2]),
    ('keys', 'f16x2-store-big192x256-kg0-st0-one', 3, 1, 0, 0, 4097, 2048, 64, 0, 8, [1, 192, 256, 0, 0, 0, 0], [176, 176, 0, 2]),
    ('keys', 'f16x2-store-big256x128-kg0-st0-one', 3, 1, 0, 0, 6145, 1024, 64, 0, 8, [1, 256, 128, 0, 0, 0, 0], [200, 200, 0, 2]),
    ('keys', 'f16x2-store-big256x192-kg0-st0-one', 3, 1, 0, 0, 2561, 3072, 64, 0, 8, [1, 256, 192, 0, 0, 0, 0], [176, 176, 0, 2]),
    ('keys', 'f16x2-store-big256x256-kg0-st0-one', 3, 2, 0, 0, 5121, 512, 64, 0, 8, [1, 256, 256, 0, 0, 0, 0], [42, 48, 0, 2]),
    ('keys', 'f16x2-partial-gemm64x64-kg1-st0-one', 3, 1, 1, 0, 1, 64, 32, 1, 8, [0, 64, 64, 1, 0, 0, 0], None),
    ('keys', 'f16x2-partial-gemm64x64-kg1-st2-one', 3, 1, 1, 0, 4097, 512, 32, 1, 8, [0, 64, 64, 1, 2, 0, 0], None),
    ('keys', 'f16x2-partial-gemm64x64-kg1-st2-slices-product', 3, 1, 1, 0, 1799, 384, 1536, 3, 8, [0, 64, 64, 1, 2, 1, 0], None),
    ('keys', 'f16x2-partial-gemm64x64-kg1-st2-slices-xcd-product', 3, 2, 1, 0, 1025, 1024, 1024, 2, 8, [0, 64, 64, 1, 2, 1, 1], None),
    ('keys', 'f16x2-partial-gemm64x64-kg1-st3-one', 3, 1, 1, 0, 4097, 256, 32, 1, 8, [0, 64, 64, 1, 3, 0, 0], None),
    ('keys', 'f16x2-partial-gemm64x64-kg1-st3-slices-product', 3, 1, 1, 0, 1025, 384, 1536, 3, 8, [0, 64, 64, 1, 3, 1, 0], None),
    ('keys', 'f16x2-partial-gemm64x64-kg2-st0-one', 3, 1, 1, 0, 1, 64, 128, 1, 8, [0, 64, 64, 2, 0, 0, 0], None),
    ('keys', 'f16x2-partial-big192x128-kg0-st0-one', 3, 1, 1, 0, 513, 4096, 64, 1, 8, [1, 192, 128, 0, 0, 0, 0], [96, 96, 0, 2]),
    ('keys', 'f16x2-partial-big192x128-kg0-st0-slices-product', 3, 1, 1, 0, 1285, 1024, 1024, 2, 8, [1, 192, 128, 0, 0, 1, 0], [112, 112, 0, 16]),
    ('keys', 'f16x2-partial-big192x256-kg0-st0-one', 3, 1, 1, 0, 4097, 2048, 64, 1, 8, [1, 192, 256, 0, 0, 0, 0], [176, 176, 0, 2]),
    ('keys', 'f16x2-partial-big256x128-kg0-st0-one', 3, 1, 1, 0, 6145, 1024, 64, 1, 8, [1, 256, 128, 0, 0, 0, 0], [200, 200, 0, 2]),
    ('keys', 'f16x2-partial-big256x128-kg0-st0-slices-product', 3, 1, 1, 0, 5379, 384, 1536, 3, 8, [1, 256, 128, 0, 0, 1, 0], [198, 200, 0, 16]),
    ('keys', 'f16x2-partial-big256x192-kg0-st0-one', 3, 1, 1, 0, 2561, 3072, 64, 1, 8, [1, 256, 192, 0, 0, 0, 0], [176, 176, 0, 2]),
    ('keys', 'f16x2-partial-big256x256-kg0-st0-one', 3, 2, 1, 0, 6145, 512, 64, 1, 8, [1, 256, 256, 0, 0, 0, 0], [50, 56, 0, 2]),
    ('keys', 'f16x2-partial-big256x256-kg0-st0-slices-product', 3, 2, 1, 0, 1542, 1024, 1024, 2, 8, [1, 256, 256, 0, 0, 1, 0], [56, 56, 0, 16]),
]
CASES = [Case(*t) for t in _TABLE]

# 256 k-tiles per slice: one more than the launch arguments hold.  The call must refuse and write nothing.
REFUSED = [
    Case("refused", "64x64-nk256", BF16, 1, STORE, 0, 70, 128, 256 * 64, 0, 32, None, None),
    Case("refused", "64x64-partial-nk256", BF16, 2, PARTIAL, 0, 70, 128, 2 * 256 * 64, 2, 32, None, None),
    Case("refused", "64x64-nk256-fp32", F32, 1, STORE, 0, 70, 128, 256 * 32, 0, 32, None, None),
    Case("refused", "big256x128-nk256", BF16, 1, PARTIAL, 128, 293, 256, 256 * 64, 1, 32, None, None),
    Case("refused", "big256x256-store-nk256", F16, 1, STORE, 256, 293, 256, 256 * 64, 0, 32, None, None),
    Case("refused", "big192x128-nk256-f16x2", F16X2, 1, PARTIAL, 1192, 229, 256, 2 * 256 * 32, 2, 32, None, None),
]


def sweep_rows(BM):
    """M = q BM + r: both sides of every 8-row copy group, 16-row MFMA block and half tile of a last tile, one and two row tiles"""
    rs = sorted({1, 7, 8, 9, 15, 16, 17, BM // 2 - 1, BM // 2, BM // 2 + 1, BM - 17, BM - 16, BM - 1, BM})
    return [q * BM + r for q in (0, 1) for r in rs]


def ring_rows():
    """the tails of sweep_rows(64) behind 64 full row tiles"""
    return [64 * 64 + r for r in sweep_rows(64)[:14]]


def _sweeps():
    out = []
    # 64-row tiles: the library's own plan.  One k-group under hint 2, two under hint 1 at 4 k-tiles; the width is the one with the
    # most workgroups that still fit 256, so 96 and 128 columns need N past 256 tiles of 64: N per q (one or two row tiles)
    wide = {64: (128, 128), 96: (16704, 8448), 128: (16640, 8320)}
    for prec in (F32, BF16, F16, F16X2):
        kt = KTILE[prec]
        for kg, hint in ((1, 2), (2, 1)):
            for bn in (64, 96, 128):
                out.append(Sweep(f"64x{bn}-kg{kg}-store-{PREC_NAMES[prec]}", prec, hint, STORE, 0, 64, bn, kg, wide[bn], 4 * kt, 0))
            out.append(Sweep(f"64x64-kg{kg}-partial-{PREC_NAMES[prec]}", prec, hint, PARTIAL, 0, 64, 64, kg, (128, 128), 8 * kt, 2))
    for prec in (BF16, F16):       # the 128 x 128 tile on small shapes: vitvs_op_linear_variant 2 (plain 16-bit types)
        out.append(Sweep(f"128x128-store-{PREC_NAMES[prec]}", prec, 1, STORE, 2, 128, 128, 1, (256, 256), 128, 0))
        out.append(Sweep(f"128x128-partial-{PREC_NAMES[prec]}", prec, 1, PARTIAL, 2, 128, 128, 1, (256, 256), 256, 2))
    # ... and as the library plans it in every precision: one slice, N a multiple of 128, 256 tiles or more (N per q), and for
    # the 16-bit types one k-tile, which the tiles of gemm_big.hip do not take
    for prec in (F32, BF16, F16, F16X2):
        kt = KTILE[prec]
        out.append(Sweep(f"128x128-planned-store-{PREC_NAMES[prec]}", prec, 1, STORE, 0, 128, 128, 1, (32768, 16384), kt, 0))
        out.append(Sweep(f"128x128-planned-partial-{PREC_NAMES[prec]}", prec, 1, PARTIAL, 0, 128, 128, 1, (32768, 16384), kt, 1))
    # the shallower rings of the 64-row launches with more than 256 workgroups (65 row tiles): 3 stages up to 512 workgroups,
    # 2 beyond and on 128 columns
    for prec in (F32, BF16, F16, F16X2):
        kt = KTILE[prec]
        for bn, stages, epi, n in ((64, 3, STORE, 320), (64, 2, STORE, 576), (128, 2, STORE, 512), (64, 3, PARTIAL, 256),
                                   (64, 2, PARTIAL, 512)):
            out.append(Sweep(f"64x{bn}-st{stages}-{'partial' if epi else 'store'}-{PREC_NAMES[prec]}", prec, 1, epi, 0, 64, bn, 1,
                             (n, n), 2 * kt, epi, stages, tuple(ring_rows())))
    for variant, (bm, bn) in BIG_VARIANT.items():
        for prec in (BF16, F16, F16X2):
            kt = KTILE[prec]
            out.append(Sweep(f"big{bm}x{bn}-store-{PREC_NAMES[prec]}", prec, 1, STORE, variant, bm, bn, 0, (2 * bn, 2 * bn), 2 * kt, 0))
            out.append(Sweep(f"big{bm}x{bn}-partial-{PREC_NAMES[prec]}", prec, 1, PARTIAL, variant, bm, bn, 0, (2 * bn, 2 * bn), 4 * kt, 2))
    return out


SWEEPS = _sweeps()


def sweep_cases(s):
    """the launches of a sweep as cases (key: what the library must plan for the 64-row tiles; forced tiles have none to ask)"""
    multi = int(s.slices > 1)
    for M in s.rows or sweep_rows(s.BM):
        N = s.N[0] if M <= s.BM else s.N[1]
        key = [int(s.kg == 0), s.BM, s.BN, s.kg, s.stages, multi, 0]
        grid = None
        if s.kg == 0:
            tiles = -(-M // s.BM) * (N // s.BN) * max(s.slices, 1)
            grid = [tiles, 8 * -(-tiles // 8), 0, s.K // max(s.slices, 1) // KTILE[s.prec]]
        yield Case("rows", f"{s.name}-M{M}", s.prec, s.hint, s.epi, s.variant, M, N, s.K, s.slices, 8, key, grid)


def case_id(c):
    """family-name-precision (names that already carry the precision keep it once)"""
    tagged = c.family == "keys" or c.name.rsplit("-", 1)[-1] in PREC_NAMES.values()
    return f"{c.family}-{c.name}" if tagged else f"{c.family}-{c.name}-{PREC_NAMES[c.prec]}"


# ------------------------------------------------------------------------------------------------ plans
def plan_of(lib, c):
    """(rc, key, slices) the library plans for a case under the calling thread's hint; forced tiles answer for themselves"""
    if c.variant != 0:
        return 0, list(c.key), max(c.slices, 1)
    out = (C.c_int32 * 7)()
    rc = lib.vitvs_op_linear_plan(c.prec, c.epi, c.M, c.N, c.K, c.slices if c.epi == PARTIAL else 0, out)
    big, rows, cols, kg, stages, slices, xcd = list(out)
    return rc, [big, rows, cols, kg, stages, int(slices > 1), xcd], slices


def grid_of(lib, c):
    """(rc, [tiles, workgroups, XCD map, k-tiles per slice]) of a case on a tile of gemm_big.hip"""
    out = (C.c_int32 * 4)()
    rc = lib.vitvs_op_linear_big_grid(c.prec, c.key[1], c.key[2], c.M, c.N, c.K, c.slices if c.epi == PARTIAL else 0, out)
    return rc, list(out)


def assert_plan(lib, c):
    """The case launches what it declares, under its hint (restored).  For the GPU tests before they launch, and the host test."""
    prev = lib.vitvs_op_plan_in_flight(c.hint)
    try:
        rc, key, slices = plan_of(lib, c)
        assert rc == 0 and key == c.key and slices == max(c.slices, 1), \
            f"{case_id(c)}: the library plans {key} x {slices} slices here (rc {rc}), not the case's {c.key} x {max(c.slices, 1)}"
        if c.key[0]:
            rc, grid = grid_of(lib, c)
            assert rc == 0 and grid == c.grid, f"{case_id(c)}: the grid hook reports {grid} (rc {rc}), not the case's {c.grid}"
    finally:
        lib.vitvs_op_plan_in_flight(prev)


def tile_walk(nx, ny, nz, slots, xmap, shift=0):
    """linear_big_kernel's tile list per workgroup, restated: [(slice, row tile, column tile), ...] for each of `slots` workgroups.
    shift != 0 is the fault model "an XCD block boundary off by one tile": every block but the first starts `shift` tiles later."""
    tiles, stride = nx * ny * nz, slots // 8
    walk = []
    for wg in range(slots):
        xcd, local = wg & 7, wg >> 3
        mine = []
        if xmap == 0:
            per = (tiles + 7) >> 3
            for it in range(local, min(per, tiles - xcd * per), stride):
                lin = xcd * per + it + (shift if xcd else 0)
                tz, rem = divmod(lin, nx * ny)
                mine.append((tz, rem // nx, rem % nx))
        else:
            xc_n = 8 // xmap
            xr_i, xc_i, R = xcd // xc_n, xcd % xc_n, ny * nz
            r0, c0 = (R * xr_i) // xmap, (nx * xc_i) // xc_n
            cols = (nx * (xc_i + 1)) // xc_n - c0
            if xmap > 1 and xr_i:
                r0 += shift
            elif xmap == 1 and xc_i:
                c0 += shift          # (one block of rows: the boundaries are between column blocks)
            for it in range(local, ((R * (xr_i + 1)) // xmap - r0) * cols, stride):
                rr = r0 + it // cols
                mine.append((rr // ny, rr % ny, c0 + it % cols))
        walk.append(mine)
    return walk


# ------------------------------------------------------------------------------------------------ operands
def _mix(a, b, seed):
    """a 32-bit hash of two integer tensors (int64 arithmetic, the same on every device)"""
    m = 0xffffffff
    h = (a * 0x9E3779B1 + b * 0x85EBCA77 + seed * 0xC2B2AE3D + 0x27D4EB2F) & m
    h = ((h ^ (h >> 15)) * 0x2C1B3C6D) & m
    h = ((h ^ (h >> 12)) * 0x297A2D39) & m
    return h ^ (h >> 15)


def make_a(M, K, dens, device="cpu"):
    """fp32 [M, K]: one +-1 per `dens` consecutive k"""
    chunks = K // dens
    r = torch.arange(M, dtype=torch.int64, device=device)[:, None]
    c = torch.arange(chunks, dtype=torch.int64, device=device)[None, :]
    h = _mix(r, c, 1)
    # chunks 0 .. 3 spell the row's low 16 bits (4 bits each, offset per chunk): distinct rows stay distinct
    digit = ((r >> (4 * c.clamp(max=3))) + 5 * c) & 15
    state = torch.where(c < 4, digit | ((h & (2 * dens // 16 - 1)) << 4), h) % (2 * dens)
    pos, sign = state >> 1, 1 - 2 * (state & 1)
    A = torch.zeros(M, chunks, dens, dtype=torch.float32, device=device)
    A.scatter_(2, pos[:, :, None], sign[:, :, None].float())
    return A.reshape(M, K)


def make_w(N, K, device="cpu"):
    """fp32 [N, K] in {-2, -1, 1, 2}"""
    n = torch.arange(N, dtype=torch.int64, device=device)[:, None]
    k = torch.arange(K, dtype=torch.int64, device=device)[None, :]
    return torch.tensor([-2.0, -1.0, 1.0, 2.0], device=device)[_mix(n, k, 2) & 3]


def make_cols(N, device="cpu"):
    """bias in [-8, 8], ls in {-1, 1, 2} (fp32 [N])"""
    n = torch.arange(N, dtype=torch.int64, device=device)
    z = torch.zeros_like(n)
    return (_mix(n, z, 3) % 17 - 8).float(), torch.tensor([-1.0, 1.0, 2.0], device=device)[_mix(n, z, 4) % 3]


def make_x0(M, N, device="cpu"):
    r = torch.arange(M, dtype=torch.int64, device=device)[:, None]
    n = torch.arange(N, dtype=torch.int64, device=device)[None, :]
    return (_mix(r, n, 5) % 9 - 4).float()


def to_x2(t):
    """fp32 [R, C] -> fp16 [R, 2 C]: per 32 columns [hi | lo] (csrc/common.h); the integers here have no low half"""
    r, c = t.shape
    hi = t.half()
    lo = (t - hi.float()).half()
    return torch.stack([hi.view(r, c // 32, 32), lo.view(r, c // 32, 32)], dim=2).reshape(r, 2 * c).contiguous()


def from_x2(t):
    """fp16 [R, 2 C] -> (hi, lo) fp64 [R, C]"""
    r, c2 = t.shape
    v = t.reshape(r, c2 // 64, 2, 32).double()
    return v[:, :, 0].reshape(r, c2 // 2), v[:, :, 1].reshape(r, c2 // 2)


def pack(prec, t):
    """what the kernel is given for the fp32 integer matrix t"""
    return to_x2(t) if prec == F16X2 else t.to(DTYPES[prec]).contiguous()


def reference(A, W, slices=1):
    """fp64 [slices, M, N]: slice z holds the products of ITS K range"""
    ks = A.shape[1] // slices
    return torch.stack([A[:, z * ks:(z + 1) * ks].double() @ W[:, z * ks:(z + 1) * ks].double().t() for z in range(slices)])


def tile_geometry(c):
    """(BM, BN, wave rows, wave columns) of the case's tile; wave (wr, wc) owns rows wr * wave rows .. and columns wc * wave columns .."""
    bm, bn = c.key[1], c.key[2]
    if c.key[0]:
        return (bm, bn) + BIG_WAVES[(bm, bn)][2:]
    return bm, bn, bm // 2, bn // 2


def locate(c, m, n):
    """where element (m, n) is computed, for a failure report"""
    bm, bn, wr, wc = tile_geometry(c)
    ml, nl = m % bm, n % bn
    if c.key[0]:
        wave = (ml // wr) * BIG_WAVES[(bm, bn)][1] + nl // wc
    else:
        wave = (ml // wr) + 2 * (nl // wc)
    return f"({m}, {n}): tile ({m // bm}, {n // bn}) wave {wave} 16-row block {ml // 16}"


def describe_mismatch(c, got, ref, what):
    """count and the first few differing elements of two [M, N] tensors"""
    bad = (got != ref).nonzero()
    first = "; ".join(f"{locate(c, int(m), int(n))} got {float(got[m, n]):g} want {float(ref[m, n]):g}" for m, n in bad[:6].tolist())
    return f"{case_id(c)} {what}: {len(bad)} of {ref.numel()} elements differ: {first}"


# ------------------------------------------------------------------------------------------------ conditions and fault models
def check_conditions(c, A, W, bias, ref, weights_checked=False):
    """The conditions under which every precision is exact, on the case's own operands.  weights_checked: W and bias are the ones
    an earlier call of a sweep has already checked (the conditions on W alone are not repeated)."""
    who = case_id(c)
    assert c.K % (c.dens * max(c.slices, 1)) == 0 and c.N % 64 == 0
    nz = (A.reshape(c.M, c.K // c.dens, c.dens) != 0).sum(2)
    assert bool((nz == 1).all()) and bool((A.abs() <= 1).all()), f"{who}: A is not one +-1 per {c.dens} k"
    if not weights_checked:
        assert set(W.unique().tolist()) <= {-2.0, -1.0, 1.0, 2.0}
        assert len(torch.unique(W, dim=0)) == c.N, f"{who}: two columns' weights are equal"
    if c.K >= 4 * c.dens and c.M <= 65536:
        assert len(torch.unique(A, dim=0)) == c.M, f"{who}: two rows of A are equal"
    # every partial sum in any order: bounded by sum_k |a| |w| <= 2 K / dens
    assert float((A.abs().double() @ W.abs().double().t()).max()) + 8 < 2 ** 24
    assert bool((ref == ref.round()).all())
    if c.epi == STORE:
        out = ref[0] + bias.double()
        assert float(out.abs().max()) <= STORE_LIMIT[c.prec], f"{who}: |output| {float(out.abs().max()):g} > {STORE_LIMIT[c.prec]}"
        for t in (A, W, out.float()):      # and what the kernel is given is what the reference multiplies
            assert torch.equal(pack(c.prec, t).double() if c.prec != F16X2 else from_x2(pack(c.prec, t))[0], t.double())
    if c.prec == F16X2:
        assert not bool(from_x2(pack(c.prec, A))[1].any()) and not bool(from_x2(pack(c.prec, W))[1].any())


def _tiles_any(x, bm, bn):
    """[row tiles, column tiles] bool: the tile holds a non-zero of x [M, N]"""
    M, N = x.shape
    ny = -(-M // bm)
    pad = torch.zeros(ny * bm, N, dtype=torch.bool)
    pad[:M] = x != 0
    return pad.reshape(ny, bm, N // bn, bn).any(3).any(1)


def check_faults(c, A, W, bias, ref):
    """Each fault model changes at least one element of every tile it touches (on the reference alone)."""
    who = case_id(c)
    bm, bn, wr, wc = tile_geometry(c)
    s = max(c.slices, 1)
    kt, ks = KTILE[c.prec], c.K // s
    nk = ks // kt
    ny, nx = -(-c.M // bm), c.N // bn
    Ad, Wd = A.double(), W.double()
    # a k-tile or a 16-byte k-chunk dropped or doubled in one (row tile, column tile): the term itself must show in the tile
    for z in sorted({0, s - 1}):
        for j in sorted({0, 1 % nk, nk // 2, nk - 1}):
            k0 = z * ks + j * kt
            term = Ad[:, k0:k0 + kt] @ Wd[:, k0:k0 + kt].t()
            assert bool(_tiles_any(term, bm, bn).all()), f"{who}: k-tile {j} of slice {z} vanishes in a tile"
            for ch in sorted({0, kt // 8 - 1}):
                term = Ad[:, k0 + 8 * ch:k0 + 8 * ch + 8] @ Wd[:, k0 + 8 * ch:k0 + 8 * ch + 8].t()
                assert bool(_tiles_any(term, bm, bn).all()), f"{who}: chunk {ch} of k-tile {j} of slice {z} vanishes in a tile"
    # two slices swapped
    for z in range(1, s):
        assert bool(_tiles_any(ref[z] - ref[z - 1], bm, bn).all()), f"{who}: slices {z - 1} and {z} agree on a tile"
    out = ref + (bias.double() if c.epi == STORE else 0)
    for z in sorted({0, s - 1}):
        o = out[z]
        # two row tiles swapped (neighbours, and first with last): over the rows both hold
        for a, b in {(t, t + 1) for t in range(ny - 1)} | ({(0, ny - 1)} if ny > 2 else set()):
            rows = min(bm, c.M - b * bm)
            d = o[a * bm:a * bm + rows] - o[b * bm:b * bm + rows]
            assert bool(_tiles_any(d, bm, bn).all()), f"{who}: row tiles {a} and {b} agree on a column tile"
        # two column tiles swapped (neighbours: always inside one XCD block or across its edge)
        for a in range(nx - 1):
            d = o[:, a * bn:(a + 1) * bn] - o[:, (a + 1) * bn:(a + 2) * bn]
            assert bool(_tiles_any(d, bm, bn).all()), f"{who}: column tiles {a} and {a + 1} agree on a row tile"
        # row M - 1 (the row clamped loads replicate) copied into another row of the last tile
        last = o[(ny - 1) * bm:c.M - 1]
        if len(last):
            d = (last - o[c.M - 1]).reshape(len(last), nx, bn)
            assert bool((d != 0).any(2).all()), f"{who}: a row of the last tile equals row M - 1 over a column tile"
        # one wave's sub-tile skipped: its products must not all be zero (bias alone would then be right)
        p = ref[z]
        pad = torch.zeros(ny * bm, c.N, dtype=torch.bool)
        pad[:c.M] = p != 0
        rows_live = torch.zeros(ny * bm, dtype=torch.bool)
        rows_live[:c.M] = True
        sub = pad.reshape(ny * bm // wr, wr, c.N // wc, wc).any(3).any(1)
        live = rows_live.reshape(ny * bm // wr, wr).any(1)
        assert bool(sub[live].all()), f"{who}: a wave's sub-tile is all zero"
    if c.key[0]:
        # an XCD block boundary shifted by one tile: a tile is computed twice and another never (it stays NaN)
        walk = tile_walk(nx, ny, s, c.grid[1], c.grid[2])
        seen = collections.Counter(t for wg in walk for t in wg)
        assert len(seen) == nx * ny * s and set(seen.values()) == {1}, f"{who}: the restated walk does not cover the tile list once"
        if nx * ny * s >= 2:
            off = collections.Counter(t for wg in tile_walk(nx, ny, s, c.grid[1], c.grid[2], shift=1) for t in wg)
            lost = [t for t in seen if t not in off]
            assert lost, f"{who}: a shifted block boundary loses no tile"      # (a lost tile stays NaN in the output)
