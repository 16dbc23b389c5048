"""The bar table of tests/test_gpu_ends_cover.py, re-measured on the CPU.

Every figure that module records is the error of a plain torch fp32 statement against the module's fp64 reference on the
module's own inputs.  This walks the same cases, measures the same statements, and fails when a recorded figure is understated
(a bar would then be tighter than its derivation allows) or grossly overstated (looser), when a bar is not 8 x its figure
capped by the end-to-end bar it replaces, or when the LayerNorm bar of the offset rows no longer separates the two-pass
statement from a one-pass variance.  No kernel runs here."""
import torch

import test_gpu_ends_cover as ec
from op_support import rel_max
from vitvs_amd import _lib


def _worst():
    w = dict.fromkeys(ec.MEASURED, 0.0)
    for D in ec.WIDTHS:
        for n_img, T, P in ec.EPILOGUE_SHAPES:
            for slices in (1, 5):
                t = ec.epilogue_inputs(D, n_img, T, P, slices)
                for use_ls in (False, True):
                    rows = ec.patch_rows_of(ec.epilogue_x(t, use_ls)[1].float(), n_img, T, P)
                    w["epilogue_dn"] = max(w["epilogue_dn"], rel_max(ec.dn_f32(rows), ec.dn_ref(rows)))
                    w["epilogue_sq"] = max(w["epilogue_sq"], rel_max(ec.sq_f32(rows), ec.sq_ref(rows)))
    for grid in (1, 2, 3, 5):
        for D in (128, 384, 1024):
            for P in (1, 5):
                for n_img in (1, 3):
                    for zero_image in (False, True):
                        x = ec.descriptor_inputs(grid, P, n_img, D, zero_image)
                        rows = ec.patch_rows_of(x.view(-1, D), n_img, grid * grid, P)
                        wide = ec.binned_gather(rows, n_img, grid)
                        if rows.any():
                            w["plain_dn"] = max(w["plain_dn"], rel_max(ec.dn_f32(rows), ec.dn_ref(rows)))
                            w["binned_dn"] = max(w["binned_dn"], rel_max(ec.dn_f32(wide), ec.dn_ref(wide)))
    for Dp in (1, 63, 64, 65, 1152):
        for rows in (1, 5):
            for zero_row in (True, False):
                src = ec.normalize_inputs(rows, Dp, zero_row)
                if src.any():
                    w["normalize"] = max(w["normalize"], rel_max(ec.dn_f32(src), ec.dn_ref(src)))
    return w


def test_recorded_statement_errors_and_bars():
    w = _worst()
    for k, got in w.items():
        if k != "saliency":
            assert ec.MEASURED[k] / 2 <= got <= ec.MEASURED[k], (k, got, ec.MEASURED[k])
    for k in ec.MEASURED:
        assert ec.BAR[k] == min(8 * ec.MEASURED[k], ec.CAP[k]), k
    assert ec.CAP["saliency"] == 2e-4 and all(ec.CAP[k] == 2e-5 for k in ec.CAP if k != "saliency")


def test_recorded_saliency_statement_error_and_peaks():
    worst, margin = 0.0, 1.0
    for _, prec in ec.SALIENCY_PRECS:
        for T in (5, 255, 256, 257, 600):
            for P in (1, 5):
                for prescaled in (0, 1):
                    qkv = ec.saliency_inputs(prec, T, P, prescaled)
                    for heads in ec.SALIENCY_HEADS:
                        ref = ec.saliency_ref(qkv, T, P, heads, prescaled)
                        worst = max(worst, float((ec.saliency_f32(qkv, T, P, heads, prescaled).double() - ref).abs().max()))
                        assert float(ref.min()) == 0.0 and float(ref.max()) == 1.0
                        margin = min(margin, float((1.0 - ref.topk(2, dim=-1).values[:, 1]).min()))
    assert ec.MEASURED["saliency"] / 2 <= worst <= ec.MEASURED["saliency"], worst
    # the GPU test asserts the arg-max: the reference's runner-up is further below the peak than two bars in every case
    assert margin > 2 * ec.BAR["saliency"], margin


def test_offset_row_bar_separates_two_pass_from_one_pass():
    two, one = 0.0, float("inf")
    for D in ec.WIDTHS:
        x, gamma, beta = ec.ln_stress_rows(D)
        ref = ec.layer_norm64(x, gamma, beta)
        y2, y1 = ec.ln_f32(x, gamma, beta), ec.ln_f32(x, gamma, beta, one_pass=True)
        for r in ec.OFFSET:
            two = max(two, rel_max(y2[r], ref[r]))
            e1 = rel_max(y1[r], ref[r])
            one = min(one, e1 if e1 == e1 else float("inf"))             # a negative one-pass variance gives NaN: no better
        for r in ec.ORDINARY + ec.SPIKE:
            assert rel_max(y2[r], ref[r]) <= ec.BAR_LN[_lib.F32] / 8
        assert torch.equal(y2[ec.CONSTANT], beta.view(1, -1))           # exact in the statement too
        # the 16-bit check of the value before the cast: the two-pass statement passes it, the one-pass variance does not
        for prec in (_lib.BF16, _lib.F16):
            dt = ec.DTYPES[prec]
            assert ec.cast_excess(y2.to(dt).double(), ref, prec) <= 1.0, (D, prec)
            bad = y1[ec.OFFSET]
            assert not torch.isfinite(bad).all() or ec.cast_excess(bad.to(dt).double(), ref[ec.OFFSET], prec) > 1.0, (D, prec)
    assert ec.LN_TWO_PASS_WORST / 2 <= two <= ec.LN_TWO_PASS_WORST, two
    assert ec.LN_ONE_PASS_BEST <= one <= 2 * ec.LN_ONE_PASS_BEST, one
    assert 4 * ec.LN_TWO_PASS_WORST <= ec.BAR_LN_OFFSET and ec.BAR_LN_OFFSET * 50 <= ec.LN_ONE_PASS_BEST
