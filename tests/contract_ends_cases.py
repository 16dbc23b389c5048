"""The ends of the ranges include/vitvs_ops.h states, as one table (tests/test_contract_ends_host.py checks it on the CPU,
tests/test_gpu_contract_ends.py runs it on the device).

A ``Case`` is run here: the hook, the end it sits on ("smallest", "largest" or "first_refused"; a size on the way to the largest,
such as 255 cameras, counts as "largest"), its arguments, the return code the header promises and the sentence of the header it
tests, quoted.  A ``Cited`` end is one an existing test already sits on: it is named, not run again.  Sizes that come from a
launch plan are never typed: an argument "@name.largest" / "@name.first_refused" is looked up in ``bounds()``, which bisects
the plan hook (host arithmetic); the host test asserts the pair against the header's formula.

The inputs and fp64 references are built by ``build(case_id)`` from the helpers of the neighbouring op tests (their seeded
case makers, packers and references), once per case and never modified."""
import functools
from collections import namedtuple

import numpy as np
import torch

import homography_consensus_ref as hcr
import pose_consensus_ref as pcr
import rig_ref as rg
import select_ref as sref

Case = namedtuple("Case", "id hook end args rc sentence")
Cited = namedtuple("Cited", "hook end test sentence")

LDS_160K = 160 * 1024
LAM = 0.35

# ---- the header's sentences (whitespace-normalised substrings of include/vitvs_ops.h) ------------------------------------------------
S_RIG = "Returns 0, -1 (a null required pointer), -2 (n_cams outside 1 .. 256, ld < 1)."
S_RIG_BLOCK = "a block may serve calls of other n_cams and ld that fit it"
S_RIG_TWO = "Same results bit for bit."
S_ROBUST = "-2 (n_cams outside 1 .. 256, ld < 1, n_iter outside 1 .. 16), -3 (the plan's)."
S_ROBUST_PAIRS = "a camera's rows count in pairs (an odd last row is dropped)"
S_ROBUST_PLAN = "= 8 (260 + (resident ? 7 * 384 : 0) + 2 pairs)"
S_POSE = "-2 (n_pairs or ld < 1, n_iter outside 0 .. 16), -3 (the plan's)."
S_POSE_PLAN = "out[0] the dynamic LDS bytes = 8 (320 + (n_iter > 0 ? 2 max_rows : 0))"
S_POSE_CONS = "n_hyp 0 .. 4096 three-point hypotheses drawn from `seed`"
S_POSE_CONS_PLAN = "8 (320 + (n_iter > 0 ? 2 max_rows : n_hyp > 0 ? max_rows : 0) + (n_hyp > 0 ? 8 + (max_rows + 1) / 2 : 0))"
S_HOMOGRAPHY = "-2 (n_pairs or ld < 1, n_iter outside 0 .. 16, depth_scale <= 0 or not finite), -3 (the plan's)."
S_HOMOGRAPHY_PLAN = "out[0] the dynamic LDS bytes = 8 (752 + (n_iter > 0 ? 2 max_rows : 0))"
S_HOMOGRAPHY_CONS = "n_hyp 0 .. 4096 four-point hypotheses drawn from `seed`"
S_HOMOGRAPHY_CONS_PLAN = "8 (752 + (n_iter > 0 ? 2 max_rows : 0) + (n_hyp > 0 ? 8 + (max_rows + 1) / 2 : 0))"
S_POSE_RIG = "Returns 0, -1 (a null required pointer), -2 (n_cams or ld < 1, n_iter outside 0 .. 16), -3 (the plan's)."
S_POSE_RIG_PLAN = "out[0] the dynamic LDS bytes = 8 (320 + (n_iter > 0 ? 2 n_cams ld : 0))"
S_SERVO_PLAN = "-3 past 160 KiB of LDS (out filled)"
S_BEST = "-3, without a launch, when T keys do not fit in 160 KiB of LDS"
S_BEST_CELLS = "for `cells` in 1 .. 16 image cells per side"
S_STENCIL = "grid * grid = T"
S_ARGMAX = "the plan of vitvs_op_gram_plan(precision, 0, T, Dp, n_pairs, n_pairs)"
S_TURNS = "copy k = numpy.rot90(frame, k), for any S >= 1"
S_NORMALIZE = "fp32 rows of any width Dp >= 1"
S_SALIENCY_HEADS = "a HOST array, 1 .. 16 entries in 0 .. H - 1"
S_SALIENCY_LDS = "-3 when 2 T + P floats pass 64 KiB of LDS"
S_SLICES = "(1 .. 8 slices, summed in index order)"
S_ATTENTION = "out[n_img*N][H*64] = softmax(q k^T / 8) v per (image, head)"

# hook -> the ends its sentence gives it (a hook "for any S >= 1" has no largest and refuses nothing)
ENDS = {
    "vitvs_op_rig_law": ("smallest", "largest", "first_refused"),
    "vitvs_op_rig_robust_law": ("smallest", "largest", "first_refused"),
    "vitvs_op_pose_rig_law": ("smallest", "largest", "first_refused"),
    "vitvs_op_pose_law": ("smallest", "largest", "first_refused"),
    "vitvs_op_pose_consensus_law": ("smallest", "largest", "first_refused"),
    "vitvs_op_homography_law": ("smallest", "largest", "first_refused"),
    "vitvs_op_homography_consensus_law": ("smallest", "largest", "first_refused"),
    "vitvs_op_best_order_dev": ("smallest", "largest", "first_refused"),
    "vitvs_op_gram_stencil": ("smallest",),
    "vitvs_op_gram_argmax": ("smallest",),
    "vitvs_op_quarter_turns": ("smallest", "largest"),
    "vitvs_op_normalize_rows": ("smallest", "largest"),
    "vitvs_op_saliency": ("smallest", "largest", "first_refused"),
    "vitvs_op_embed_ln": ("smallest", "largest", "first_refused"),
    "vitvs_op_residual_ln": ("smallest", "largest"),
    "vitvs_op_residual_desc": ("smallest", "largest", "first_refused"),
    "vitvs_op_attention": ("smallest",),
}

# the other hooks of the header: plans and settings without a device launch, and launches whose sizes are tile, K-slice and
# key-range matters with edge tests of their own; hook -> the test that covers it
EXCLUDED = {
    "vitvs_op_linear": "tests/test_gpu_gemm_exact.py::test_case_is_exact",
    "vitvs_op_linear_variant": "tests/test_gpu_gemm_exact.py::test_case_is_exact",
    "vitvs_op_linear_residual": "tests/test_gpu_ops.py::test_linear_residual",
    "vitvs_op_linear_partial": "tests/test_gpu_gemm_exact.py::test_row_edges_are_exact",
    "vitvs_op_layernorm": "tests/test_gpu_ends_cover.py::test_layernorm_stress_rows",
    "vitvs_op_attention_q": "tests/test_gpu_attention_keys.py::test_attention_keys_against_fp64",
    "vitvs_op_patchify": "tests/test_gpu_ends_cover.py::test_patch_rows_are_the_fp32_statement",
    "vitvs_op_descriptors": "tests/test_gpu_ends_cover.py::test_descriptors",
    "vitvs_op_facet": "tests/test_gpu_ends_cover.py::test_facet_is_the_fp32_statement",
    "vitvs_op_roll_pick": "tests/test_gpu_roll_op.py::test_pick_and_carry_back",
    "vitvs_op_touch": None, "vitvs_op_splitk_slices": None, "vitvs_op_weight_exponent": None, "vitvs_op_plan_in_flight": None,
    "vitvs_op_linear_tile": None, "vitvs_op_linear_plan": None, "vitvs_op_linear_big_grid": None, "vitvs_op_attention_plan": None,
    "vitvs_op_gram_plan": None, "vitvs_op_rig_two_launches": None,
    # host arithmetic: bisected by tests/test_contract_ends_host.py, or the byte counts beside a law's hook
    "vitvs_op_servo_plan": None, "vitvs_op_rig_robust_plan": None, "vitvs_op_pose_plan": None, "vitvs_op_pose_consensus_plan": None,
    "vitvs_op_homography_plan": None, "vitvs_op_homography_consensus_plan": None, "vitvs_op_pose_rig_plan": None,
    "vitvs_op_rig_scratch_bytes": None, "vitvs_op_rig_robust_scratch_bytes": None, "vitvs_op_pose_scratch_bytes": None,
    "vitvs_op_homography_scratch_bytes": None, "vitvs_op_pose_rig_scratch_bytes": None,
}

CASES = [
    # ---- the rig law: one workgroup per camera, a running row offset over all cameras before it, the fan-in in camera order
    Case("rig-1cam-1row", "vitvs_op_rig_law", "smallest", dict(n=1, ld=1, kind="mixed"), 0, S_RIG),
    Case("rig-10cams", "vitvs_op_rig_law", "largest", dict(n=10, ld=48, kind="mixed"), 0, S_RIG),
    Case("rig-65cams", "vitvs_op_rig_law", "largest", dict(n=65, ld=48, kind="mixed"), 0, S_RIG),
    Case("rig-255cams", "vitvs_op_rig_law", "largest", dict(n=255, ld=48, kind="mixed"), 0, S_RIG),
    Case("rig-256cams", "vitvs_op_rig_law", "largest", dict(n=256, ld=48, kind="mixed"), 0, S_RIG),
    Case("rig-256cams-ld1", "vitvs_op_rig_law", "largest", dict(n=256, ld=1, kind="mixed"), 0, S_RIG),
    Case("rig-256cams-ld2", "vitvs_op_rig_law", "largest", dict(n=256, ld=2, kind="mixed"), 0, S_RIG),
    Case("rig-256cams-ld4", "vitvs_op_rig_law", "largest", dict(n=256, ld=4, kind="mixed"), 0, S_RIG),
    Case("rig-256cams-jacobi", "vitvs_op_rig_law", "largest", dict(n=256, ld=4, kind="turning"), 0, S_RIG),
    Case("rig-256cams-equal-bits", "vitvs_op_rig_law", "largest", dict(n=256, ld=48, kind="mixed", bits=True), 0, S_RIG_TWO),
    Case("rig-256-3-256-one-block", "vitvs_op_rig_law", "largest", dict(n=256, ld=48, kind="mixed", block=True), 0, S_RIG_BLOCK),
    Case("rig-257cams", "vitvs_op_rig_law", "first_refused", dict(n=257, ld=48, kind="mixed"), -2, S_RIG),
    # ---- the robust rig law: the same launch shape; rho and w of every pair in LDS, past 64 KiB from 4096 pairs on
    Case("robust-1cam-1pair", "vitvs_op_rig_robust_law", "smallest", dict(n=1, ld=2), 0, S_ROBUST),
    Case("robust-256cams-ld1", "vitvs_op_rig_robust_law", "smallest", dict(n=256, ld=1), 0, S_ROBUST_PAIRS),
    Case("robust-10cams", "vitvs_op_rig_robust_law", "largest", dict(n=10, ld=48), 0, S_ROBUST),
    Case("robust-65cams", "vitvs_op_rig_robust_law", "largest", dict(n=65, ld=48), 0, S_ROBUST),
    Case("robust-255cams", "vitvs_op_rig_robust_law", "largest", dict(n=255, ld=48), 0, S_ROBUST),
    Case("robust-256cams", "vitvs_op_rig_robust_law", "largest", dict(n=256, ld=48), 0, S_ROBUST),
    Case("robust-256cams-ld2", "vitvs_op_rig_robust_law", "largest", dict(n=256, ld=2), 0, S_ROBUST),
    Case("robust-256cams-ld4", "vitvs_op_rig_robust_law", "largest", dict(n=256, ld=4), 0, S_ROBUST),
    Case("robust-256cams-jacobi", "vitvs_op_rig_robust_law", "largest", dict(n=256, ld=4, kind="turning"), 0, S_ROBUST),
    Case("robust-256cams-equal-bits", "vitvs_op_rig_robust_law", "largest", dict(n=256, ld=48, bits=True), 0, S_ROBUST),
    Case("robust-256cams-largest-ld", "vitvs_op_rig_robust_law", "largest", dict(n=256, ld="@rig_robust.largest"), 0, S_ROBUST_PLAN),
    Case("robust-256cams-past-160k", "vitvs_op_rig_robust_law", "first_refused", dict(n=256, ld="@rig_robust.first_refused"), -3,
         S_ROBUST_PLAN),
    # ---- the pose rig law: one workgroup over the stack of all cameras
    Case("poserig-1cam-1row", "vitvs_op_pose_rig_law", "smallest", dict(n=1, ld=1, n_iter=4), 0, S_POSE_RIG),
    Case("poserig-256cams-ld1", "vitvs_op_pose_rig_law", "smallest", dict(n=256, ld=1, n_iter=4), 0, S_POSE_RIG),
    Case("poserig-10cams", "vitvs_op_pose_rig_law", "largest", dict(n=10, ld=48, n_iter=4), 0, S_POSE_RIG),
    Case("poserig-65cams", "vitvs_op_pose_rig_law", "largest", dict(n=65, ld=48, n_iter=4), 0, S_POSE_RIG),
    Case("poserig-255cams", "vitvs_op_pose_rig_law", "largest", dict(n=255, ld=4, n_iter=4), 0, S_POSE_RIG),
    Case("poserig-256cams", "vitvs_op_pose_rig_law", "largest", dict(n=256, ld=2, n_iter=4), 0, S_POSE_RIG),
    Case("poserig-256cams-largest-ld", "vitvs_op_pose_rig_law", "largest", dict(n=256, ld="@pose_rig.largest", n_iter=4), 0,
         S_POSE_RIG_PLAN),
    Case("poserig-256cams-past-160k", "vitvs_op_pose_rig_law", "first_refused", dict(n=256, ld="@pose_rig.first_refused", n_iter=4),
         -3, S_POSE_RIG_PLAN),
    # ---- the pose law and its consensus start: the LDS opt-in runs at the plan's largest max_rows
    Case("pose-1row", "vitvs_op_pose_law", "smallest", dict(pairs=1, ld=1, n_iter=(0, 16)), 0, S_POSE),
    Case("pose-64pairs", "vitvs_op_pose_law", "largest", dict(pairs=64, ld=24, n_iter=(0, 16)), 0, S_POSE),
    Case("pose-largest-ld", "vitvs_op_pose_law", "largest", dict(pairs=1, ld="@pose.largest", n_iter=(1, 16)), 0, S_POSE_PLAN),
    Case("pose-past-160k", "vitvs_op_pose_law", "first_refused", dict(pairs=1, ld="@pose.first_refused", n_iter=(1,)), -3, S_POSE_PLAN),
    Case("posecons-1row", "vitvs_op_pose_consensus_law", "smallest", dict(pairs=1, ld=1, n_iter=(0, 4), n_hyp=(1, 64)), 0, S_POSE_CONS),
    Case("posecons-3rows", "vitvs_op_pose_consensus_law", "smallest", dict(pairs=1, ld=3, n_iter=(0, 4), n_hyp=(1, 64)), 0, S_POSE_CONS),
    Case("posecons-1hyp", "vitvs_op_pose_consensus_law", "smallest", dict(pairs=2, ld=40, n_iter=(0, 4), n_hyp=(1,)), 0, S_POSE_CONS),
    Case("posecons-64pairs", "vitvs_op_pose_consensus_law", "largest", dict(pairs=64, ld=24, n_iter=(0, 4), n_hyp=(64,)), 0, S_POSE_CONS),
    Case("posecons-4096hyp", "vitvs_op_pose_consensus_law", "largest", dict(pairs=2, ld=40, n_iter=(0, 16), n_hyp=(4096,)), 0, S_POSE_CONS),
    Case("posecons-largest-ld", "vitvs_op_pose_consensus_law", "largest",
         dict(pairs=1, ld="@pose_consensus.largest", n_iter=(1,), n_hyp=(64,)), 0, S_POSE_CONS_PLAN),
    Case("posecons-past-160k", "vitvs_op_pose_consensus_law", "first_refused",
         dict(pairs=1, ld="@pose_consensus.first_refused", n_iter=(1,), n_hyp=(64,)), -3, S_POSE_CONS_PLAN),
    # ---- the homography law and its consensus start
    Case("homography-1row", "vitvs_op_homography_law", "smallest", dict(pairs=1, ld=1, n_iter=(0, 16)), 0, S_HOMOGRAPHY),
    Case("homography-64pairs", "vitvs_op_homography_law", "largest", dict(pairs=64, ld=24, n_iter=(0, 16)), 0, S_HOMOGRAPHY),
    Case("homography-largest-ld", "vitvs_op_homography_law", "largest", dict(pairs=1, ld="@homography.largest", n_iter=(1, 16)), 0,
         S_HOMOGRAPHY_PLAN),
    Case("homography-past-160k", "vitvs_op_homography_law", "first_refused", dict(pairs=1, ld="@homography.first_refused", n_iter=(1,)),
         -3, S_HOMOGRAPHY_PLAN),
    Case("homcons-1row", "vitvs_op_homography_consensus_law", "smallest", dict(pairs=1, ld=1, n_iter=(0, 4), n_hyp=(1, 64)), 0,
         S_HOMOGRAPHY_CONS),
    Case("homcons-4rows", "vitvs_op_homography_consensus_law", "smallest", dict(pairs=1, ld=4, n_iter=(0, 4), n_hyp=(1, 64)), 0,
         S_HOMOGRAPHY_CONS),
    Case("homcons-1hyp", "vitvs_op_homography_consensus_law", "smallest", dict(pairs=2, ld=40, n_iter=(0, 4), n_hyp=(1,)), 0,
         S_HOMOGRAPHY_CONS),
    Case("homcons-64pairs", "vitvs_op_homography_consensus_law", "largest", dict(pairs=64, ld=24, n_iter=(0, 4), n_hyp=(64,)), 0,
         S_HOMOGRAPHY_CONS),
    Case("homcons-4096hyp", "vitvs_op_homography_consensus_law", "largest", dict(pairs=2, ld=40, n_iter=(0, 16), n_hyp=(4096,)), 0,
         S_HOMOGRAPHY_CONS),
    Case("homcons-largest-ld", "vitvs_op_homography_consensus_law", "largest",
         dict(pairs=1, ld="@homography_consensus.largest", n_iter=(1,), n_hyp=(64,)), 0, S_HOMOGRAPHY_CONS_PLAN),
    Case("homcons-past-160k", "vitvs_op_homography_consensus_law", "first_refused",
         dict(pairs=1, ld="@homography_consensus.first_refused", n_iter=(1,), n_hyp=(64,)), -3, S_HOMOGRAPHY_CONS_PLAN),
    # ---- the best order: 14-bit ids and 15-bit ranks
    Case("best-T1", "vitvs_op_best_order_dev", "smallest", dict(T=1, cells=(1, 2, 16), kind="random"), 0, S_BEST_CELLS),
    Case("best-T4", "vitvs_op_best_order_dev", "smallest", dict(T=4, cells=(1, 2, 3, 16), kind="random"), 0, S_BEST_CELLS),
    Case("best-T9", "vitvs_op_best_order_dev", "smallest", dict(T=9, cells=(1, 2, 3, 4, 16), kind="random"), 0, S_BEST_CELLS),
    Case("best-largest-all-equal", "vitvs_op_best_order_dev", "largest", dict(T="@best_order.largest", cells=(16, 1), kind="flat"), 0,
         S_BEST),
    # ---- the stencil arg-max of binned descriptors
    Case("stencil-g1", "vitvs_op_gram_stencil", "smallest", dict(grid=1, D=64, kind="perm"), 0, S_STENCIL),
    Case("stencil-g2", "vitvs_op_gram_stencil", "smallest", dict(grid=2, D=64, kind="perm"), 0, S_STENCIL),
    Case("stencil-g3", "vitvs_op_gram_stencil", "smallest", dict(grid=3, D=64, kind="perm"), 0, S_STENCIL),
    Case("stencil-g5", "vitvs_op_gram_stencil", "smallest", dict(grid=5, D=64, kind="perm"), 0, S_STENCIL),
    Case("stencil-g9-ties", "vitvs_op_gram_stencil", "smallest", dict(grid=9, D=64, kind="ties"), 0, S_STENCIL),
    Case("stencil-g9-negative", "vitvs_op_gram_stencil", "smallest", dict(grid=9, D=64, kind="neg"), 0, S_STENCIL),
    Case("stencil-g9-zero-neighbourhood", "vitvs_op_gram_stencil", "smallest", dict(grid=9, D=64, kind="zero"), 0, S_STENCIL),
    Case("stencil-g9-high-norm", "vitvs_op_gram_stencil", "smallest", dict(grid=9, D=64, kind="norm"), 0, S_STENCIL),
    # ---- the fused arg-max below one tile
    Case("argmax-T1", "vitvs_op_gram_argmax", "smallest", dict(T=1), 0, S_ARGMAX),
    Case("argmax-T2", "vitvs_op_gram_argmax", "smallest", dict(T=2), 0, S_ARGMAX),
    Case("argmax-T31", "vitvs_op_gram_argmax", "smallest", dict(T=31), 0, S_ARGMAX),
    Case("argmax-T33", "vitvs_op_gram_argmax", "smallest", dict(T=33), 0, S_ARGMAX),
    # ---- the elementwise ends
    Case("turns-S1", "vitvs_op_quarter_turns", "smallest", dict(S=1), 0, S_TURNS),
    Case("turns-S2", "vitvs_op_quarter_turns", "smallest", dict(S=2), 0, S_TURNS),
    Case("turns-S31", "vitvs_op_quarter_turns", "smallest", dict(S=31), 0, S_TURNS),
    Case("turns-S33", "vitvs_op_quarter_turns", "smallest", dict(S=33), 0, S_TURNS),
    Case("normalize-Dp4097", "vitvs_op_normalize_rows", "largest", dict(Dp=4097), 0, S_NORMALIZE),
    Case("saliency-1head", "vitvs_op_saliency", "smallest", dict(T=5, P=1, H=3, heads=(2,)), 0, S_SALIENCY_HEADS),
    Case("saliency-16heads", "vitvs_op_saliency", "largest", dict(T=5, P=1, H=3, heads=(0, 1, 2, 2, 1, 0, 0, 2, 1, 1, 2, 0, 2, 2, 0, 1)), 0,
         S_SALIENCY_HEADS),
    Case("saliency-P1-largest-T", "vitvs_op_saliency", "largest", dict(T="@saliency_p1.largest", P=1, H=1, heads=(0,)), 0, S_SALIENCY_LDS),
    Case("saliency-P5-largest-T", "vitvs_op_saliency", "largest", dict(T="@saliency_p5.largest", P=5, H=1, heads=(0,)), 0, S_SALIENCY_LDS),
    Case("saliency-P1-past-64k", "vitvs_op_saliency", "first_refused", dict(T="@saliency_p1.first_refused", P=1, H=1, heads=(0,)), -3,
         S_SALIENCY_LDS),
    Case("saliency-P5-past-64k", "vitvs_op_saliency", "first_refused", dict(T="@saliency_p5.first_refused", P=5, H=1, heads=(0,)), -3,
         S_SALIENCY_LDS),
    Case("embed-1token-1slice", "vitvs_op_embed_ln", "smallest", dict(slices=1), 0, S_SLICES),
    Case("embed-1token-8slices", "vitvs_op_embed_ln", "largest", dict(slices=8), 0, S_SLICES),
    Case("residual-ln-1row-1slice", "vitvs_op_residual_ln", "smallest", dict(slices=1), 0, S_SLICES),
    Case("residual-ln-1row-8slices", "vitvs_op_residual_ln", "largest", dict(slices=8), 0, S_SLICES),
    Case("residual-desc-1token-1slice", "vitvs_op_residual_desc", "smallest", dict(slices=1), 0, S_SLICES),
    Case("residual-desc-1token-8slices", "vitvs_op_residual_desc", "largest", dict(slices=8), 0, S_SLICES),
]

CITED = [
    Cited("vitvs_op_rig_robust_law", "first_refused",
          "tests/test_gpu_rig_robust_op.py::test_optional_outputs_may_be_null_and_bad_arguments_are_refused", S_ROBUST),   # 257 cameras
    Cited("vitvs_op_pose_rig_law", "first_refused", "tests/test_gpu_pose_rig_op.py::test_null_outputs_and_error_returns", S_POSE_RIG),
    Cited("vitvs_op_pose_law", "smallest", "tests/test_gpu_pose_op.py::test_kernel_equals_the_reference", S_POSE),          # 1 x 3 rows
    Cited("vitvs_op_pose_consensus_law", "first_refused", "tests/test_gpu_pose_consensus_op.py::test_error_returns", S_POSE_CONS),   # 4097
    Cited("vitvs_op_pose_consensus_law", "smallest",                                                                     # n_hyp = 0
          "tests/test_gpu_pose_consensus_op.py::test_no_hypotheses_is_the_law_without_consensus_bit_for_bit", S_POSE_CONS),
    Cited("vitvs_op_homography_consensus_law", "smallest",
          "tests/test_gpu_homography_consensus_op.py::test_no_hypotheses_is_the_law_without_consensus_bit_for_bit", S_HOMOGRAPHY_CONS),
    Cited("vitvs_op_homography_law", "smallest", "tests/test_gpu_homography_op.py::test_kernel_equals_the_reference", S_HOMOGRAPHY),
    Cited("vitvs_op_homography_consensus_law", "first_refused", "tests/test_gpu_homography_consensus_op.py::test_error_returns",
          S_HOMOGRAPHY_CONS),
    # T = 128 x 128 on random tables with cells = 16, and 129 x 129 refused without a launch
    Cited("vitvs_op_best_order_dev", "largest", "tests/test_gpu_select_op.py::test_refusals_without_a_launch", S_BEST),
    Cited("vitvs_op_best_order_dev", "first_refused", "tests/test_gpu_select_op.py::test_refusals_without_a_launch", S_BEST),
    Cited("vitvs_op_quarter_turns", "largest", "tests/test_gpu_roll_op.py::test_quarter_turns_are_rot90", S_TURNS),        # S = 224
    Cited("vitvs_op_normalize_rows", "smallest", "tests/test_gpu_ends_cover.py::test_normalize_rows", S_NORMALIZE),        # Dp 1, 63, 65
    Cited("vitvs_op_saliency", "first_refused", "tests/test_gpu_ends_cover.py::test_saliency_refusals", S_SALIENCY_HEADS),  # head H, 17
    Cited("vitvs_op_embed_ln", "first_refused", "tests/test_gpu_ends_cover.py::test_embedding_epilogue_refusals", S_SLICES),   # 0, 9
    Cited("vitvs_op_residual_desc", "first_refused", "tests/test_gpu_ends_cover.py::test_descriptor_epilogue_refusals", S_SLICES),
    Cited("vitvs_op_attention", "smallest", "tests/test_gpu_attention_keys.py::test_attention_keys_against_fp64", S_ATTENTION),   # N = 1
]

BY_ID = {c.id: c for c in CASES}


# ---- the plans' ends --------------------------------------------------------------------------------------------------------------
def _bisect(refused, lo=1, hi=1 << 22):
    """(the last size `refused` is False for, the first it is True for); `refused` is monotone, False at lo and True at hi."""
    assert not refused(lo) and refused(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if refused(mid) else (mid, hi)
    return lo, hi


@functools.lru_cache(maxsize=None)
def _bounds():
    from vitvs_amd import _lib
    import ctypes as C
    lib = _lib.load()
    out4 = (C.c_int32 * 8)()

    def plan(fn, *args):
        rc = fn(*args, out4)
        assert rc in (0, -3), (fn, args, rc)
        return rc == -3
    b = {
        "pose": _bisect(lambda r: plan(lib.vitvs_op_pose_plan, r, 1)),
        "pose_consensus": _bisect(lambda r: plan(lib.vitvs_op_pose_consensus_plan, r, 1, 64)),
        "homography": _bisect(lambda r: plan(lib.vitvs_op_homography_plan, r, 1)),
        "homography_consensus": _bisect(lambda r: plan(lib.vitvs_op_homography_consensus_plan, r, 1, 64)),
        "pose_rig": _bisect(lambda ld: plan(lib.vitvs_op_pose_rig_plan, 256, ld, 1), hi=1 << 16),
        "rig_robust": _bisect(lambda ld: plan(lib.vitvs_op_rig_robust_plan, 256, ld), hi=1 << 16),
        "servo": _bisect(lambda r: plan(lib.vitvs_op_servo_plan, 196, r, 4, 0, 0)),
    }
    # no plan hook: the header's own sentence.  A sort of T keys runs on the next power of two of 8-byte keys (and 2 KiB of group
    # heads); the grid is square.
    g = 1
    while best_order_lds((g + 1) * (g + 1)) <= LDS_160K:
        g += 1
    b["best_order"] = (g * g, (g + 1) * (g + 1))
    for P in (1, 5):                  # 2 T + P floats within 64 KiB
        T = (65536 // 4 - P) // 2
        b[f"saliency_p{P}"] = (T, T + 1)
    return b


def best_order_lds(T):
    """select.hip's plan_best_order restated (the library has no plan hook for it): keep in step with the launcher.  The library
    itself confirms the refused side on the host, and the device test the admitted one."""
    n = 2
    while n < T:
        n <<= 1
    return n * 8 * (2 if T <= 256 else 1) + 512 * 4


def bounds():
    """name -> (largest admitted, first refused)"""
    return dict(_bounds())


def resolve(args):
    out = {}
    for k, v in args.items():
        if isinstance(v, str) and v.startswith("@"):
            name, end = v[1:].split(".")
            v = bounds()[name][("largest", "first_refused").index(end)]
        out[k] = v
    return out


# ---- inputs and references ------------------------------------------------------------------------------------------------------------
def _seed(case):
    import zlib
    return zlib.crc32(case.id.encode()) % (2 ** 31)


def mixed_rows(n, ld, even=False):
    """A row count per camera: 0, ld, 2, 4, ld, 7, ... with an empty camera first, in the middle and last."""
    pattern = [0, ld, 2, 4, ld, 7, ld // 2, ld, 4, 2]
    rows = [min(pattern[i % len(pattern)], ld) for i in range(n)]
    if n > 2:
        rows[n // 2] = 0
        rows[-1] = 0
    if n == 1:
        rows[0] = ld
    if even:
        rows = [r & ~1 for r in rows]
    return rows


def _rig(case, a):
    import test_gpu_rig_op as ro
    n, ld = min(a["n"], 256), a["ld"]
    if a["kind"] == "turning":        # rows of pure rotation (the three translation columns of every L_i are zero): W_i's lower left
        rng = np.random.default_rng(_seed(case))            # block is zero, so M's first three columns are exact zeros and its rank
        Ws = [rg.twist_matrix(*rg.random_extrinsic(rng)) for _ in range(n)]              # is 3 whatever the rounding: the Jacobi path
        Ls = [ro._system(rng, ld) * np.array([0.0, 0.0, 0.0, 1.0, 1.0, 1.0]) for _ in range(n)]
        c = dict(Ls=Ls, es=[0.05 * rng.standard_normal(ld) for _ in range(n)], Ws=Ws, ld=ld)
        solver = "jacobi"
    else:
        rows = mixed_rows(n, ld)
        c = ro._random_case(_seed(case), rows, ld=ld)
        solver = "jacobi" if sum(rows) < 6 else "ldlt"
    d = dict(case=c, solver=solver, ref=ro._reference(c))
    if a.get("block"):
        d["small"] = ro._random_case(_seed(case) + 1, [48, 0, 7], ld=48)
        d["small_ref"] = ro._reference(d["small"])
    return d


def _robust(case, a):
    import test_gpu_rig_robust_op as rro
    n, ld = a["n"], a["ld"]
    if ld == 1:                        # no pair at all: the odd last row is dropped, nobody contributes
        rng = np.random.default_rng(_seed(case))
        c = dict(Ls=[np.zeros((0, 6))] * n, es=[np.zeros(0)] * n, Ws=[rg.twist_matrix(*rg.random_extrinsic(rng)) for _ in range(n)],
                 lives=None, ld=1, smin=0.03, rows_given=[1] * n)
        return dict(case=c, solver="none", n_iter=4, ref=dict(status=2, worst=2))
    if a.get("kind") == "turning":     # _rig's rank-3 stack: the translation columns of every L_i zero, e following one rig twist
        rows = [ld] * n
        c = rro._case(_seed(case), rows, ld=ld, smin=0.01, out_share=0.0)
        rng = np.random.default_rng(_seed(case) + 1)
        v = rng.standard_normal(6) * 0.1
        c["Ls"] = [L * np.array([0.0, 0.0, 0.0, 1.0, 1.0, 1.0]) for L in c["Ls"]]
        c["es"] = [L @ W @ v + rng.uniform(-0.003, 0.003, ld) for L, W in zip(c["Ls"], c["Ws"])]
        solver = "jacobi"
    else:
        rows = mixed_rows(n, ld, even=True)
        c = rro._case(_seed(case), rows, ld=ld, smin=0.01)
        solver = "jacobi" if sum(rows) < 6 else "ldlt"
    ref = rro._ref_of(c, 4)
    ref.update(cameras=sum(1 for r in rows if r), worst=2 if 0 in rows else 0)
    return dict(case=c, solver=solver, n_iter=4, ref=ref)


def _pose_rig(case, a):
    import test_gpu_pose_rig_op as pro
    import pose_rig_ref as prr
    n, ld = a["n"], a["ld"]
    rows = mixed_rows(n, ld)
    usable = np.zeros((n, ld), np.int32)
    for i, r in enumerate(rows):
        usable[i, :r] = 1
        if r > 8:
            usable[i, 3] = -1          # a hole
    status = np.zeros(n, np.int32)
    if n > 4:
        status[1], status[n // 3] = 2, 1          # cameras that do not contribute: their rows are NaN
    c = pro._case(_seed(case), n, ld, 0.7, usable, status=status)
    rng = np.random.default_rng(_seed(case) + 1)
    for i in range(n):                 # a few outliers in every contributing camera with rows to spare
        if status[i] == 0 and rows[i] >= 24:
            bad = rng.choice(np.nonzero(usable[i] > 0)[0], 3, replace=False)
            c["P"][i, bad] += rng.uniform(0.1, 0.3, (3, 3)) * rng.choice([-1.0, 1.0], (3, 3))
    with np.errstate(all="ignore"):
        refs = {}
        for n_iter in (0, a["n_iter"]):
            ref = prr.pose_rig_law(c["P"], c["Q"], c["usable"], c["rig"], c["status"], LAM, n_iter, pro.SMIN)
            Ps, Qs, _, _, _ = prr.stack_points(c["P"], c["Q"], c["usable"], c["rig"], c["status"])
            ref["moments_abs"] = prr.moments(np.abs(Ps), np.abs(Qs), ref["weights"].reshape(-1))
            refs[n_iter] = ref
    return dict(case=c, refs=refs)


def _flags(rows, b):
    """usable flags of pair b: a fraction of the rows unusable (padded rows and holes) first, in the middle and last; how many, and
    where the middle run starts, differ from pair to pair"""
    u = np.ones(rows, np.int32)
    if rows >= 24:
        k = rows // 12 + b % 3
        u[:k - b % 2] = 0
        mid = rows // 2 + (b % 5) - 2
        u[mid:mid + k] = -1
        u[rows - k:] = 0
    return u


def pairs_law_conditioned(hook, a, refs):
    """None when every solve of every pair keeps its margins (an eigen-gap >= 1e-6 / a second eigenvalue >= 1e-4 of the trace, no
    residual within 1e-6 of a rejection edge or of the consensus cut-off, a winner's cost >= 1e-6 below any other row set's), so
    that neither a status, a weight nor a winner can flip; else what fails."""
    pose = "pose" in hook
    few = a["ld"] < (3 if pose else 4)
    for (n_hyp, n_iter), per_pair in refs.items():
        for b, ref in enumerate(per_pair):
            where = (n_hyp, n_iter, b)
            for g in (ref["gaps"] if pose else ref["ratios"]):
                if not (g >= (1e-6 if pose else 1e-4) or (few and g <= 1e-10)):
                    return where, "gap", g
            if not ref["edge"] >= 1e-6:
                return where, "edge", ref["edge"]
            if few:
                if ref["status"] != 2:
                    return where, "status", ref["status"]
                continue
            if ref["status"] != 0 or ref["info"][2] != n_iter:
                return where, "status", ref["status"], ref["info"]
            if n_hyp and not (ref["info"][6] >= 1 and ref["cgap" if pose else "gap"] >= 1e-6 and ref["edge_T"] >= 1e-6):
                return where, "consensus", ref["info"], ref["cgap" if pose else "gap"], ref["edge_T"]
    return None


PAIR_SALTS = 10


def _pairs_law(case, a, make, law, smin):
    """The first salt of the seed under which the references alone keep their margins (pairs_law_conditioned)."""
    pairs = a["pairs"]
    for salt in range(PAIR_SALTS):
        c = make(_seed(case) + 7919 * salt)
        refs = {}
        with np.errstate(all="ignore"):
            for n_hyp in a.get("n_hyp", (0,)):
                for n_iter in a["n_iter"]:
                    refs[(n_hyp, n_iter)] = [law(c, b, n_iter, n_hyp) for b in range(pairs)]
        if pairs_law_conditioned(case.hook, a, refs) is None:
            break
    return dict(case=c, refs=refs, smin=smin, salt=salt)


def _pose(case, a):
    import test_gpu_pose_op as po
    pairs, ld = a["pairs"], a["ld"]
    smin = po.SMIN if "n_hyp" not in a else 0.019

    def make(seed):
        return po._case(*[po._pair(seed + b, ld, 0.3 + 2.5 * b / max(pairs, 2), _flags(ld, b), outliers=ld // 20 if ld >= 24 else 0)
                          for b in range(pairs)], degenerate=ld < 3)
    return _pairs_law(case, a, make, lambda c, b, n_iter, n_hyp: pcr.pose_consensus_law(c["P"][b], c["Q"][b], c["usable"][b], LAM, n_iter,
                                                                                        smin, n_hyp, 1), smin)


def _homography(case, a):
    import test_gpu_homography_op as ho
    pairs, ld = a["pairs"], a["ld"]

    def make(seed):
        return ho._case(*[ho._pair(seed + b, ld, _flags(ld, b), outliers=ld // 20 if ld >= 24 else 0, rot=0.1 + 0.3 * b / max(pairs, 2))
                          for b in range(pairs)], degenerate=ld < 4)
    return _pairs_law(case, a, make, lambda c, b, n_iter, n_hyp: hcr.homography_consensus_law(c["m"][b], c["ms"][b], c["usable"][b], LAM,
                                                                                              ho.ZHAT, n_iter, ho.SMIN, n_hyp, 1), ho.SMIN)


def sorted_ranks(nn_1, nn_2, sim_1, cells):
    """select_ref.ranks by one sort instead of an n x n comparison per group (tests/test_contract_ends_host.py proves them equal)."""
    sim = np.asarray(sim_1, np.float32)
    T = sim.shape[0]
    cls = np.where(sref.mutual_mask(nn_1, nn_2), 0, 1).astype(np.int64)
    cell, _ = sref.cells_of(T, cells)
    group = cls * 256 + cell
    ids = np.arange(T)
    order = np.lexsort((ids, -(sim.astype(np.float64) + 0.0), group))       # group, then larger sim first, then smaller id
    g_sorted = group[order]
    head = np.r_[True, g_sorted[1:] != g_sorted[:-1]]
    start = np.maximum.accumulate(np.where(head, np.arange(T), 0))
    rho = np.zeros(T, np.int64)
    rho[order] = np.arange(T) - start
    return cls, cell, rho


def sorted_best_order(nn_1, nn_2, sim_1, cells):
    sim = np.asarray(sim_1, np.float32)
    cls, _, rho = sorted_ranks(nn_1, nn_2, sim, cells)
    return np.lexsort((np.arange(sim.shape[0]), -sim.astype(np.float64), rho, cls)).astype(np.int32)


def _best(case, a):
    T = a["T"]
    rng = np.random.default_rng(_seed(case))
    ident = np.arange(T)
    if a["kind"] == "flat":            # all similarities equal, nothing mutual: only the id field orders the keys
        tab = ((ident + 1) % T, (ident + 2) % T, np.full(T, 0.5, np.float32))
    else:
        nn1 = rng.integers(0, T, T)
        nn2 = rng.integers(0, T, T)
        if T > 1:
            nn2[nn1[0]] = 0            # token 0 is mutual
        tab = (nn1, nn2, rng.uniform(0.1, 0.9, T).astype(np.float32))
    return dict(tables=tab, want={c: sorted_best_order(*tab, c) for c in a["cells"]})


STENCIL_P = (1, 5)


def _block(centre, g):
    y, x = divmod(centre, g)
    return [(y + dy) * g + (x + dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]


def stencil_tokens(case, a, P, salt=0):
    """(x [2][P + T][D], the planted exact ties {desired row: current token}, {current column: desired token}).  The desired
    frame, then the current one: the desired tokens moved one column to the left, cyclically (a permutation under which an inner
    token's whole 3 x 3 neighbourhood moves with it) plus small noise; prefix rows NaN."""
    g, D, kind = a["grid"], a["D"], a["kind"]
    T = g * g
    gen = torch.Generator().manual_seed(_seed(case) + 100 * salt + P)
    des = torch.randn(T, D, generator=gen)
    ties_r, ties_c = {}, {}
    if kind == "neg":                  # every token of one frame in a cone, of the other in the opposite one
        axis = torch.randn(D, generator=gen)
        des = 8.0 * axis / axis.norm() + des
    if kind == "ties":                 # g = 9: the neighbourhoods of desired tokens (1, 2), (1, 6) (the same 32-row tile) and (6, 4)
        des[_block(15, g)] = des[_block(11, g)]                 # (the next tile) hold the same nine tokens
        des[_block(58, g)] = des[_block(11, g)]
    if kind == "zero":                 # one all-zero 3 x 3 neighbourhood, around (4, 4)
        des[_block(40, g)] = 0.0
        ties_r[40] = 0                 # every similarity of the row is 0: the first index
    if kind == "norm":                 # artefact tokens: a few with 100 x the norm of the others
        des[[7, 33, 34, 70]] *= 100.0
    ys, xs = np.divmod(np.arange(T), g)
    moved = torch.from_numpy(ys * g + (xs + 1) % g)
    cur = des[moved] + 0.02 * torch.randn(T, D, generator=gen)
    if kind == "neg":
        cur = -cur
    if kind == "ties":                 # ... and of current tokens (1, 1), (1, 5) and (6, 3), which are where those three went
        cur[_block(14, g)] = cur[_block(10, g)]
        cur[_block(57, g)] = cur[_block(10, g)]
        ties_r.update({11: 10, 15: 10, 58: 10})                 # columns 10, 14 and 57 tie at the maximum of these rows
        ties_c.update({10: 11, 14: 11, 57: 11})                 # rows 11, 15 and 58 tie at the maximum of these columns
        # (0, 2) and (0, 6) above the first two blocks, and (0, 1) and (0, 5) of the current frame: their neighbourhoods, clamped
        # at the upper edge, lie inside the equal blocks too
        ties_r.update({2: 1, 6: 1})
        ties_c.update({1: 2, 5: 2})
    if kind == "zero":                 # ... and around (2, 6) of the current frame
        cur[_block(24, g)] = 0.0
        ties_c[24] = 0
    if kind == "norm":
        cur[[2, 40, 41, 79]] *= 100.0
    x = torch.full((2, P + T, D), float("nan"))
    x[0, P:], x[1, P:] = des, cur
    return x, ties_r, ties_c


def margins(S):
    """top-1 minus top-2 of every row and of every column (inf with one candidate)"""
    if S.shape[0] < 2:
        return np.full(1, np.inf), np.full(1, np.inf)
    r, c = np.sort(S, axis=1), np.sort(S, axis=0)
    return r[:, -1] - r[:, -2], c[-1] - c[-2]


def clear_everywhere(S, margin, ties_r=(), ties_c=()):
    """every row and column has a top-1 / top-2 margin above `margin`, or is a planted exact tie"""
    mr, mc = margins(S)
    ok_r = [m > margin or (i in ties_r and m == 0.0) for i, m in enumerate(mr)]
    ok_c = [m > margin or (j in ties_c and m == 0.0) for j, m in enumerate(mc)]
    return all(ok_r) and all(ok_c)


MARGIN = 4e-6                        # tests/test_gpu_correspond_cover.py's (tests/test_contract_ends_host.py asserts they agree)
SALTS = 20


def _stencil(case, a):
    """per P: x, S (fp64, of the concatenated 9 D-wide descriptors) and the planted ties.  The seed's salt is the first under
    which the reference alone has a clear maximum in every row and column."""
    from test_gpu_correspond_cover import _binned_fp64
    g = a["grid"]
    out = {}
    for P in STENCIL_P:
        for salt in range(SALTS):
            x, ties_r, ties_c = stencil_tokens(case, a, P, salt)
            ref = _binned_fp64(x, g * g, P, g)
            S = (ref[0] @ ref[1].T).numpy()
            if clear_everywhere(S, MARGIN, ties_r, ties_c):
                break
        out[P] = dict(x=x, S=S, ties_r=ties_r, ties_c=ties_c, salt=salt)
    return out


ARGMAX_DP = (32, 64)
ARGMAX_FORMS = ((1, False), (3, False), (3, True))       # pairs, a shared goal


def argmax_descriptors(case, T, Dp, pairs, shared, salt=0):
    """fp32 unit rows [n_des + pairs][T][Dp]: every current frame a permutation of its goal's rows plus small noise"""
    gen = torch.Generator().manual_seed(_seed(case) + 1000 * Dp + 10 * pairs + int(shared) + 100000 * salt)
    n_des = 1 if shared else pairs
    des = torch.randn(n_des, T, Dp, generator=gen)
    cur = torch.stack([des[0 if shared else b][torch.randperm(T, generator=gen)] + 0.02 * torch.randn(T, Dp, generator=gen)
                       for b in range(pairs)])
    d = torch.cat([des, cur])
    return (d / d.norm(dim=-1, keepdim=True)).float()


def _argmax(case, a):
    out = {}
    for Dp in ARGMAX_DP:
        for pairs, shared in ARGMAX_FORMS:
            n_des = 1 if shared else pairs
            for salt in range(SALTS):
                dn = argmax_descriptors(case, a["T"], Dp, pairs, shared, salt)
                ref = dn.double()
                S = [(ref[0 if shared else b] @ ref[n_des + b].T).numpy() for b in range(pairs)]
                if all(clear_everywhere(s, MARGIN) for s in S):
                    break
            out[(Dp, pairs, shared)] = dict(dn=dn, S=S, salt=salt)
    return out


def saliency_inputs(case, a):
    """qkv fp32 [2 * (P + T)][3 * 64 H]: peaked rows, differently per image (tests/test_gpu_ends_cover.py's)"""
    T, P, H = a["T"], a["P"], a["H"]
    gen = torch.Generator().manual_seed(_seed(case))
    q = torch.randn(2, P + T, 3 * 64 * H, generator=gen)
    for img, s in enumerate((4.0, 2.0)):
        q[img, :, :64 * H] *= s
    return q.view(2 * (P + T), -1).contiguous()


def _saliency(case, a):
    import test_gpu_ends_cover as ec
    qkv = saliency_inputs(case, a)
    kw = dict(H=a["H"], n_img=2)
    return dict(qkv=qkv, ref=ec.saliency_ref(qkv, a["T"], a["P"], list(a["heads"]), 0, **kw),
                f32=ec.saliency_f32(qkv, a["T"], a["P"], list(a["heads"]), 0, **kw))


# ---- the bar table (the procedure of tests/test_gpu_ends_cover.py) -----------------------------------------------------------------
# MEASURED[k]: the worst error of a plain torch fp32 statement of the operator against the fp64 reference on this module's own
# inputs, measured on the CPU (tests/test_contract_ends_host.py re-measures every figure and fails when one is understated).
# A bar is 8 x that, for another valid summation order and expf within a couple of ulps, and never above its cap.
MEASURED = {
    "saliency": 8.2e-7,            # absolute (the map lies in [0, 1]); the four saliency cases, T up to 8191
    "stencil_norm_sim": 4.0e-7,    # stencil-g9-high-norm: |row maximum - fp64's|
    "stencil_norm_argmax": 0.0,    # ... and how far below fp64's maximum the fp32 statement's arg-max sits
    "normalize": 1.1e-7,           # normalize-Dp4097, relative to max |ref|
}
NORMALIZE_CAP = 2e-5               # tests/test_gpu_ends_cover.py's CAP["normalize"]
NORMALIZE_ROWS = 5
SALIENCY_CAP = 2e-4                # tests/test_gpu_ends_cover.py's CAP["saliency"]
ARGMAX_TOL, SIM_TOL = 1e-6, 2e-6   # tests/test_gpu_correspond_cover.py's (the host test asserts they agree)


def saliency_bar():
    return min(8 * MEASURED["saliency"], SALIENCY_CAP)


def normalize_bar():
    return min(8 * MEASURED["normalize"], NORMALIZE_CAP)


def normalize_f32_error():
    import test_gpu_ends_cover as ec
    from op_support import rel_max
    src = ec.normalize_inputs(NORMALIZE_ROWS, BY_ID["normalize-Dp4097"].args["Dp"], True)
    return rel_max(ec.dn_f32(src), ec.dn_ref(src))


def stencil_norm_bars():
    """(arg-max bar, sim_1 bar) of the high-norm case: 8 x measured, at most 10 x the bar the case would otherwise use"""
    return min(8 * MEASURED["stencil_norm_argmax"], 10 * ARGMAX_TOL), min(8 * MEASURED["stencil_norm_sim"], 10 * SIM_TOL)


def stencil_f32(x, P, g):
    """The plain torch fp32 statement of the binned similarities from the raw token Gram: nine terms G[nb_o(i)][nb_o(j)] added in
    (dy, dx) row-major order, times 1 / max(|b|, 1e-8) of both neighbourhoods."""
    T = g * g
    des, cur = x[0, P:].float(), x[1, P:].float()
    G = des @ cur.T
    ys, xs = np.divmod(np.arange(T), g)
    nb = [torch.from_numpy(np.clip(ys + o // 3 - 1, 0, g - 1) * g + np.clip(xs + o % 3 - 1, 0, g - 1)) for o in range(9)]
    acc = torch.zeros(T, T)
    for o in range(9):
        acc = acc + G[nb[o]][:, nb[o]]
    rn = []
    for t in (des, cur):
        sq = (t * t).sum(-1)
        tot = torch.zeros(T)
        for o in range(9):
            tot = tot + sq[nb[o]]
        rn.append(1.0 / tot.sqrt().clamp_min(1e-8))
    return acc * rn[0][:, None] * rn[1][None, :]


def stencil_f32_errors():
    """(sim, arg-max) errors of stencil_f32 on the high-norm case, both prefixes"""
    case = BY_ID["stencil-g9-high-norm"]
    g = case.args["grid"]
    sim = arg = 0.0
    for P, e in build(case.id).items():
        S32, S = stencil_f32(e["x"], P, g).double().numpy(), e["S"]
        T = S.shape[0]
        sim = max(sim, float(np.abs(S32.max(1) - S.max(1)).max()))
        arg = max(arg, float((S.max(1) - S[np.arange(T), S32.argmax(1)]).max()), float((S.max(0) - S[S32.argmax(0), np.arange(T)]).max()))
    return sim, arg


_BUILDERS = {
    "vitvs_op_rig_law": _rig, "vitvs_op_rig_robust_law": _robust, "vitvs_op_pose_rig_law": _pose_rig, "vitvs_op_pose_law": _pose,
    "vitvs_op_pose_consensus_law": _pose, "vitvs_op_homography_law": _homography, "vitvs_op_homography_consensus_law": _homography,
    "vitvs_op_best_order_dev": _best, "vitvs_op_gram_stencil": _stencil, "vitvs_op_gram_argmax": _argmax, "vitvs_op_saliency": _saliency,
}


@functools.lru_cache(maxsize=None)
def build(case_id):
    """The case's inputs and fp64 reference (None for a refused call and for the hooks whose driver makes its own)."""
    case = BY_ID[case_id]
    if case.rc != 0 or case.hook not in _BUILDERS:
        return None
    return _BUILDERS[case.hook](case, resolve(case.args))
