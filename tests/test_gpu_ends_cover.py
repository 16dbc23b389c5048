"""The forward's first and last launches, kernel by kernel, against fp64 (GPU).

Everything of csrc/elementwise.hip that tests/test_gpu_plan_cover.py does not reach: the patch-row builders (plain and fused
with the resize), the embedding epilogue, the descriptor epilogue of the last residual add, the plain and binned descriptor
kernels, the row normalisation, the facet and saliency kernels, and LayerNorm on the rows a trained ViT produces (a mean that
dwarfs the spread, one massive channel, a constant row).  Each kernel is driven through its pointer-only hook of
include/vitvs_ops.h, at every width D in {128, 256, 384, 768, 1024}, with 1 .. 8 K slices and register tokens (P > 1).

Conventions of tests/test_gpu_plan_cover.py: operands are rounded once to the precision (the f16x2 hi / lo layout of its
to_x2 / from_x2), the reference is a plain torch fp64 (or, where the result is exact, fp32) statement of the operator written
here, outputs start as NaN with GUARD rows (or words) around them that no launch may write, and each case records its worst
error as a junit property (`--junitxml=FILE -o junit_family=legacy`).

Bars.  x and LayerNorm: BAR_X / BAR_LN of test_gpu_plan_cover.py.  Patch rows, facet, raw descriptors and the constant LayerNorm
row are exact (equality).  The others are in the table below: the error of a plain torch fp32 statement of the same formula
against the fp64 reference on this module's own inputs, measured on the CPU (tests/test_ends_cover_host.py re-measures every
figure and fails when one is understated), times 8 for a different but equally valid summation order and expf / exp2f within
a couple of ulps, and never above the end-to-end bar the check replaces.  No bar comes from what a kernel produced."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
from oracle import resize_ref
from vitvs_amd import _lib
from op_support import gpu_lib as lib  # noqa: F401
from op_support import DTYPES, mk, nan_like, ptr, rel_max, stream, to_x2, values

pytestmark = pytest.mark.gpu

GUARD = 3                 # rows (or words) around every output that no launch may write
LOG2E = 1.4426950408889634
Q_SCALE = float(np.float32(0.125) * np.float32(1.44269504088896340736))   # kAttnQScale (csrc/kernels.h), as the compiler folds it
Q_UNSCALE = float(np.float32(1.0) / np.float32(Q_SCALE))
WIDTHS = (128, 256, 384, 768, 1024)
PRECS = [("fp32", _lib.F32), ("bf16", _lib.BF16), ("fp16", _lib.F16), ("f16x2", _lib.F16X2)]
# tests/test_gpu_plan_cover.py
BAR_X = {_lib.F32: 2e-5, _lib.BF16: 2e-6 + 1e-3, _lib.F16: 2e-6 + 1e-3, _lib.F16X2: 2e-5}
BAR_LN = {_lib.F32: 2e-5, _lib.BF16: 1e-2, _lib.F16: 2e-3, _lib.F16X2: 2e-5}
# tests/test_gpu_ops.py test_layernorm, the 16-bit outputs
BAR_LN16 = {_lib.BF16: 8e-3, _lib.F16: 1e-3}

# ---- the bar table -------------------------------------------------------------------------------------------------------
# MEASURED[k]: worst error, over every case of this module, of the torch fp32 statement (the *_f32 functions below) against the
# fp64 reference; relative to max |ref| (saliency: absolute, the map lies in [0, 1]).  CAP[k]: the end-to-end bar replaced
# (descriptors 2e-5: tests/test_gpu_path.py; saliency SALIENCY_BARS["fp32"] = 2e-4 in every precision, the inputs being shared).
MEASURED = {
    "epilogue_dn": 1.4e-7,    # dn of the descriptor epilogue
    "epilogue_sq": 1.4e-7,    # its squared norms
    "plain_dn": 1.2e-7,       # vitvs_op_descriptors, plain
    "binned_dn": 1.5e-7,      # ... binned (9 D wide)
    "normalize": 1.0e-7,      # vitvs_op_normalize_rows
    "saliency": 9.5e-7,       # both exponent forms, three precisions
}
CAP = {"epilogue_dn": 2e-5, "epilogue_sq": 2e-5, "plain_dn": 2e-5, "binned_dn": 2e-5, "normalize": 2e-5, "saliency": 2e-4}
BAR = {k: min(8 * MEASURED[k], CAP[k]) for k in MEASURED}
# LayerNorm rows `+-1000 + randn`, fp32 / f16x2 outputs, relative to the row's max |ref|.  The bar was set as 8 x the worst error
# of the fp32 two-pass statement on such rows (1.3e-5), about 100 x below the best a one-pass variance E[x^2] - E[x]^2 does
# (9.7e-3).  Re-measured with this module's seeds at the five widths, 64-lane partial sums (ln_f32 below): two-pass 2.1e-5 at
# worst (D = 768, the row around -1000), one-pass 7.7e-3 at best (D = 256, the row around +1000).
BAR_LN_OFFSET = 1e-4
LN_TWO_PASS_WORST = 2.1e-5
LN_ONE_PASS_BEST = 7.7e-3


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 17) % (2 ** 31)
    return torch.Generator().manual_seed(seed)


def _dyadic(t, denom):
    """values of t rounded to multiples of 1 / denom (a power of two): their fp32 sums are exact in any order"""
    return (torch.round(t.double() * denom) / denom).float()


# the f16x2 layout (csrc/common.h; the same helpers as tests/test_gpu_plan_cover.py)


def _operand(prec, t):
    """fp32 [R, C] -> what the kernel is given in the precision (CPU)"""
    return to_x2(t) if prec == _lib.F16X2 else t.to(DTYPES[prec]).contiguous()


def _nan32(rows, cols):
    return torch.full((rows, cols), float("nan"), dtype=torch.float32, device="cuda")


def _bits(t):
    """the bit patterns of t, for equality that tells +0 from -0"""
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _all_nan(t):
    return bool(torch.isnan(t.float()).all())


def _check(record, what, err, bar):
    record(what, f"{err:.3e}")
    assert err <= bar, f"{what}: worst error {err:.3e} > {bar:g}"


def layer_norm64(x, gamma, beta, eps=1e-6):
    return torch.nn.functional.layer_norm(x.double(), (x.shape[-1],), gamma.double(), beta.double(), eps)


# =========================================================================================================== patch rows
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
PATCH_GEOMETRIES = [(64, 16, 16), (64, 16, 8), (56, 14, 14), (56, 14, 7), (32, 8, 4)]      # S, patch, stride
FRAME_COUNTS = [(1, 1), (1, 3), (2, 2), (0, 2), (2, 0)]                                    # n_des, n_cur
# camera (in_h, in_w) -> (S, patch, stride)
FUSED = [((100, 37), (64, 16, 16)), ((120, 160), (64, 16, 8)), ((64, 160), (64, 16, 16)), ((270, 480), (32, 8, 4))]
FRAME_SLACK = 16          # bytes behind every frame buffer


def handle_kp(patch):
    return (3 * patch * patch + 63) // 64 * 64


def camera_frames(n, h, w, seed):
    """the frames of tests/test_gpu_resize.py: random pixels, the last frame with saturating structure"""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    f[-1, ::3, ::5] = 255
    f[-1, 1::3, ::4] = 0
    return f


def patch_rows_ref(frames, patch, stride, Kp):
    """frames u8 [n, S, S, 3] -> fp32 [n * T, Kp]: ((u8 / 255) - mean) / std, every step rounded to nearest in fp32, column
    k = c p^2 + py p + px; +0 from 3 p^2 on."""
    f = torch.from_numpy(np.ascontiguousarray(frames)).float()
    v = ((f / torch.tensor(255.0)) - torch.tensor(MEAN, dtype=torch.float32)) / torch.tensor(STD, dtype=torch.float32)
    n = v.shape[0]
    u = v.permute(0, 3, 1, 2).unfold(2, patch, stride).unfold(3, patch, stride)             # [n, 3, g, g, py, px]
    g = u.shape[2]
    rows = u.permute(0, 2, 3, 1, 4, 5).reshape(n * g * g, 3 * patch * patch)
    out = torch.zeros((n * g * g, Kp), dtype=torch.float32)
    out[:, :3 * patch * patch] = rows
    return out, g


def _run_patchify(lib, prec, frames, small, n_des, n_cur, geom, prefix, D, in_hw):
    """One launch: `frames` are what the kernel reads (camera frames in the fused form), `small` the S x S frames the rows are of."""
    S, patch, stride = geom
    Kp = handle_kp(patch)
    n = n_des + n_cur
    want, grid = patch_rows_ref(small[:n], patch, stride, Kp)
    T = grid * grid
    g = _gen(S, patch, stride, prefix, D)
    cls, pos = mk((D,), g), mk((1 + T, D), g, 0.5)

    def upload(part):
        if part.shape[0] == 0:
            return None
        flat = torch.zeros(part.size + FRAME_SLACK, dtype=torch.uint8)
        flat[:part.size] = torch.from_numpy(np.ascontiguousarray(part)).reshape(-1)
        return flat.cuda()
    des, cur = upload(frames[:n_des]), upload(frames[n_des:n])
    ape = nan_like(prec, n * T + GUARD, Kp)
    x = _nan32(n * (T + prefix) + GUARD, D)
    mean, std = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    clsd, posd = cls.cuda(), pos.cuda()
    rc = lib.vitvs_op_patchify(prec, ptr(des), n_des, ptr(cur), n_cur, S, patch, stride, Kp, D, prefix, mean, std, ptr(clsd), ptr(posd),
                               in_hw[0], in_hw[1], ptr(ape), ptr(x), stream())
    assert rc == 0
    torch.cuda.synchronize()
    what = f"frames {n_des}+{n_cur} prefix {prefix} D {D}"
    ape, x = ape.cpu(), x.cpu()
    assert _all_nan(ape[n * T:]), f"{what}: patch rows beyond the last token were written"
    assert torch.equal(_bits(ape[:n * T]), _bits(_operand(prec, want))), f"{what}: patch rows differ from the fp32 statement"
    if Kp > 3 * patch * patch and prec != _lib.F16X2:       # (f16x2: the hi and lo halves of the padding are part of the rows above)
        assert not _bits(ape[:n * T, 3 * patch * patch:]).any(), f"{what}: padding columns are not +0"
    cls_rows = torch.arange(n) * (T + prefix)
    assert torch.equal(_bits(x[cls_rows]), _bits((cls + pos[0]).expand(n, D))), f"{what}: class rows are not cls + pos[0]"
    other = torch.ones(x.shape[0], dtype=torch.bool)
    other[cls_rows] = False
    assert _all_nan(x[other]), f"{what}: rows of x other than the class rows were written"


@pytest.mark.parametrize("name,prec", PRECS)
@pytest.mark.parametrize("geom", PATCH_GEOMETRIES, ids=lambda g: "S%d_p%d_s%d" % g)
def test_patch_rows_are_the_fp32_statement(lib, record_property, name, prec, geom):
    frames = camera_frames(4, geom[0], geom[0], sum(geom))
    for n_des, n_cur in FRAME_COUNTS:
        for prefix in (1, 5):
            for D in (128, 384):
                _run_patchify(lib, prec, frames, frames, n_des, n_cur, geom, prefix, D, (0, 0))
    record_property("patch_rows", "0.000e+00")       # equality held in every launch


@pytest.mark.parametrize("name,prec", PRECS)
@pytest.mark.parametrize("camera,geom", FUSED, ids=["%dx%d" % c for c, _ in FUSED])
def test_fused_resize_patch_rows_are_the_rows_of_the_resized_frames(lib, record_property, name, prec, camera, geom):
    frames = camera_frames(4, camera[0], camera[1], camera[0] * 7 + camera[1])
    small = np.stack([resize_ref.resize_bicubic_u8(f, geom[0]) for f in frames])
    for i, (n_des, n_cur) in enumerate(FRAME_COUNTS):
        prefix, D = ((1, 128), (5, 384))[i % 2]
        _run_patchify(lib, prec, frames, small, n_des, n_cur, geom, prefix, D, camera)
    record_property("patch_rows", "0.000e+00")       # equality held in every launch


def test_patchify_refuses_what_it_cannot_launch(lib):
    S, patch = 64, 16
    frames = torch.zeros(6000 * 64 * 3 + FRAME_SLACK, dtype=torch.uint8, device="cuda")
    cls, pos = torch.zeros(128, device="cuda"), torch.zeros((17, 128), device="cuda")
    ape, x = nan_like(_lib.F32, 16 + GUARD, 768), _nan32(17 + GUARD, 128)
    mean, std = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)

    def call(Kp=768, in_h=0, in_w=0):
        return lib.vitvs_op_patchify(_lib.F32, None, 0, ptr(frames), 1, S, patch, patch, Kp, 128, 1, mean, std, ptr(cls), ptr(pos),
                                     in_h, in_w, ptr(ape), ptr(x), stream())
    assert call(Kp=704) == -2                     # Kp below 3 p^2
    assert call(in_h=0, in_w=5) == -2             # half a geometry
    assert call(in_h=6000, in_w=64) == -3         # one patch draws on ~1900 camera rows: 1900 * 16 * 3 bytes pass 64 KiB of LDS
    torch.cuda.synchronize()
    assert _all_nan(ape) and _all_nan(x)


# ==================================================================================================== embedding epilogue
EMBED_SHAPES = [(1, 1, 1, 4), (5, 3, 3, 7), (2, 8, 2, 1)]         # P, slices, n_img, T


def embed_inputs(D, P, slices, n_img, T):
    g = _gen(D, P, slices, n_img, T)
    # the buffer is as large as slices of n_img * (T + P) rows would be; the slices are its first slices * n_img * T rows
    buf = mk((slices * n_img * (T + P) * D,), g, 0.5)
    part = buf[:slices * n_img * T * D].view(slices, n_img * T, D)
    t = dict(buf=buf, part=part, reg=mk((max(P - 1, 1), D), g, 2.0), cls=mk((D,), g), pos=mk((1 + T, D), g, 0.7),
             bias=mk((D,), g, 0.3), gamma=1.0 + 0.1 * mk((D,), g), beta=0.1 * mk((D,), g))
    x = torch.empty((n_img, T + P, D), dtype=torch.float64)
    x[:, 0] = t["cls"].double() + t["pos"][0].double()                   # class row
    x[:, 1:P] = t["reg"][:P - 1].double()                                # register rows as given: no position, no bias
    x[:, P:] = t["pos"][1:].double() + part.double().sum(0).view(n_img, T, D) + t["bias"].double()
    t["x_ref"] = x.view(n_img * (T + P), D)
    return t


@pytest.mark.parametrize("name,prec", PRECS)
@pytest.mark.parametrize("P,slices,n_img,T", EMBED_SHAPES)
@pytest.mark.parametrize("D", WIDTHS)
def test_embedding_epilogue(lib, record_property, name, prec, D, P, slices, n_img, T):
    t = embed_inputs(D, P, slices, n_img, T)
    M = n_img * (T + P)
    d = {k: v.cuda() for k, v in t.items() if k not in ("part", "x_ref")}
    x, out = _nan32(M + GUARD, D), nan_like(prec, M + GUARD, D)              # x is write-only: a read of it would spread the NaN
    rc = lib.vitvs_op_embed_ln(prec, ptr(x), ptr(d["buf"]), slices, ptr(d["bias"]), ptr(d["pos"]), ptr(d["cls"]),
                               ptr(d["reg"]) if P > 1 else None, ptr(d["gamma"]), ptr(d["beta"]), ptr(out), n_img, T, P, D, 1e-6,
                               stream())
    assert rc == 0
    torch.cuda.synchronize()
    x, out = x.cpu(), out.cpu()
    assert _all_nan(x[M:]) and _all_nan(out[M:]), "rows beyond M were written"
    got = values(prec, out[:M])
    assert torch.isfinite(x[:M]).all() and torch.isfinite(got).all()
    _check(record_property, "x", rel_max(x[:M], t["x_ref"]), BAR_X[prec])
    _check(record_property, "layernorm", rel_max(got, layer_norm64(t["x_ref"], t["gamma"], t["beta"])), BAR_LN[prec])


def test_embedding_epilogue_refusals(lib):
    z = torch.zeros((64, 128), device="cuda")

    def call(slices=1, P=1, reg=None, D=128):
        return lib.vitvs_op_embed_ln(_lib.F32, ptr(z), ptr(z), slices, ptr(z), ptr(z), ptr(z), reg, ptr(z), ptr(z), ptr(z), 1, 4, P, D, 1e-6,
                                     stream())
    assert call(slices=0) == -2 and call(slices=9) == -2 and call(P=0) == -2 and call(P=2, reg=None) == -2 and call(D=192) == -2


# =================================================================================================== descriptor epilogue
EPILOGUE_SHAPES = [(2, 9, 1), (3, 4, 5)]       # n_img, T, P
KEY_FILL = 0x5A5A5A5A5A5A5A5A
SAME_LANES = (256, 768, 1024)                  # widths at which a lane owns the same float4s as in desc_plain_kernel (LANES = 64)


def epilogue_inputs(D, n_img, T, P, slices):
    """part, bias, ls, x0 and the row built to come out all zero: its terms, the bias and ls are short dyadic numbers, so
    x0 = -(ls * (sum part + bias)) is an fp32 number and every sum on the way is exact in any order."""
    g = _gen(D, n_img, T, P, slices, 5)
    M = n_img * (T + P)
    part = mk((slices, M, D), g, 0.5)
    bias = _dyadic(mk((D,), g, 0.3), 256)
    ls = torch.randint(2, 7, (D,), generator=g).float() / 4            # 0.5 .. 1.5
    x0 = mk((M, D), g)
    zero_row = (n_img - 1) * (T + P) + P + 1
    part[:, zero_row] = _dyadic(part[:, zero_row], 256)
    return dict(part=part, bias=bias, ls=ls, x0=x0, zero_row=zero_row)


def epilogue_x(t, use_ls):
    """(x0 with the zero row's start filled in, the fp64 x the launch must leave)"""
    acc = t["part"].double().sum(0) + t["bias"].double()
    if use_ls:
        acc = acc * t["ls"].double()
    x0 = t["x0"].clone()
    x0[t["zero_row"]] = (-acc[t["zero_row"]]).float()
    assert torch.equal(x0[t["zero_row"]].double(), -acc[t["zero_row"]])
    return x0, x0.double() + acc


def patch_rows_of(x, n_img, T, P):
    return x.view(n_img, T + P, -1)[:, P:].reshape(n_img * T, -1)


def dn_ref(rows):
    r = rows.double()
    return r / r.norm(dim=-1, keepdim=True).clamp_min(1e-8)


def dn_f32(rows):
    """the plain torch fp32 statement of the same formula"""
    r = rows.float()
    return r / (r * r).sum(-1, keepdim=True).sqrt().clamp_min(1e-8)


def sq_ref(rows):
    return (rows.double() ** 2).sum(-1)


def sq_f32(rows):
    return (rows.float() * rows.float()).sum(-1)


def _keys(words):
    return torch.full((words + GUARD,), KEY_FILL, dtype=torch.int64, device="cuda")


def _check_keys(za, zb, count, what):
    for z in (za.cpu(), zb.cpu()):
        assert not z[:count].any(), f"{what}: the first {count} key words are not all cleared"
        assert (z[count:] == KEY_FILL).all(), f"{what}: key words from {count} on were written"


@pytest.mark.parametrize("name,prec", PRECS)
@pytest.mark.parametrize("slices", [1, 5])
@pytest.mark.parametrize("n_img,T,P", EPILOGUE_SHAPES)
@pytest.mark.parametrize("D", WIDTHS)
def test_descriptor_epilogue(lib, record_property, name, prec, D, n_img, T, P, slices):
    t = epilogue_inputs(D, n_img, T, P, slices)
    M, toks = n_img * (T + P), n_img * T
    part, bias, ls = t["part"].cuda(), t["bias"].cuda(), t["ls"].cuda()
    grid = math.isqrt(T)
    worst = dict(x=0.0, dn=0.0, sq=0.0)
    counts = (0, 1, T, M * 64)
    for use_ls in (False, True):
        x0, x_ref = epilogue_x(t, use_ls)
        for emit in ("dn", "sq", "both"):
            for zero_count in counts:
                what = f"ls {use_ls} emit {emit} zero_count {zero_count}"
                x = torch.cat([x0, torch.full((GUARD, D), float("nan"))]).cuda()
                # guard rows (words) in front as well: a class row that wrote would land just before its image's rows
                dn = _nan32(GUARD + toks + GUARD, D) if emit != "sq" else None
                sq = _nan32(1, GUARD + toks + GUARD)[0] if emit != "dn" else None
                za, zb = _keys(M * 64), _keys(M * 64)
                rc = lib.vitvs_op_residual_desc(prec, ptr(x), ptr(part), slices, ptr(bias), ptr(ls) if use_ls else None,
                                                ptr(dn[GUARD:]) if dn is not None else None, ptr(sq[GUARD:]) if sq is not None else None,
                                                ptr(za), ptr(zb), zero_count, T, P, M, D, stream())
                assert rc == 0, what
                torch.cuda.synchronize()
                _check_keys(za, zb, zero_count, what)
                xc = x.cpu()
                assert _all_nan(xc[M:]), f"{what}: rows of x beyond M were written"
                assert torch.isfinite(xc[:M]).all(), what
                worst["x"] = max(worst["x"], rel_max(xc[:M], x_ref))
                assert not xc[t["zero_row"]].any(), f"{what}: the cancelling row did not come out zero"
                rows = patch_rows_of(xc[:M], n_img, T, P)                        # the x the launch left, patch rows only
                zr = t["zero_row"] - (n_img - 1) * P - P                         # the zero row among the patch rows
                if dn is not None:
                    dc = dn.cpu()
                    assert _all_nan(dc[:GUARD]) and _all_nan(dc[GUARD + toks:]), \
                        f"{what}: dn was written outside its {toks} patch rows (class / register rows write nothing)"
                    got = dc[GUARD:GUARD + toks]
                    assert torch.isfinite(got).all() and not got[zr].any(), f"{what}: dn of the zero row is not finite zeros"
                    worst["dn"] = max(worst["dn"], rel_max(got, dn_ref(rows)))
                    if D in SAME_LANES:   # "the same arithmetic and summation order as desc_plain_kernel" where the lanes agree
                        plain = _nan32(toks + GUARD, D)
                        assert lib.vitvs_op_descriptors(ptr(x), ptr(plain), None, None, n_img, T, P, grid, D, 0, None, None, 0,
                                                        stream()) == 0
                        torch.cuda.synchronize()
                        assert torch.equal(_bits(plain.cpu()[:toks]), _bits(got)), f"{what}: dn differs from desc_plain_kernel's"
                if sq is not None:
                    sc = sq.cpu()
                    assert _all_nan(sc[:GUARD]) and _all_nan(sc[GUARD + toks:]), f"{what}: sq was written outside its {toks} words"
                    got = sc[GUARD:GUARD + toks]
                    assert torch.isfinite(got).all() and float(got[zr]) == 0.0, what
                    worst["sq"] = max(worst["sq"], rel_max(got, sq_ref(rows)))
    _check(record_property, "x", worst["x"], BAR_X[prec])
    _check(record_property, "dn", worst["dn"], BAR["epilogue_dn"])
    _check(record_property, "sq", worst["sq"], BAR["epilogue_sq"])


def test_descriptor_epilogue_refusals(lib):
    n_img, T, P, D = 2, 9, 1, 128
    M = n_img * (T + P)
    x, part = torch.zeros((M, D), device="cuda"), torch.zeros((1, M, D), device="cuda")
    bias, dn = torch.zeros(D, device="cuda"), _nan32(n_img * T + GUARD, D)
    za, zb = _keys(M * 64 + 1), _keys(M * 64 + 1)

    def call(zero_count=0, dn=dn, T=T, M=M, slices=1):
        return lib.vitvs_op_residual_desc(_lib.F32, ptr(x), ptr(part), slices, ptr(bias), None, ptr(dn), None, ptr(za), ptr(zb), zero_count,
                                          T, P, M, D, stream())
    assert call(zero_count=M * 64 + 1) == -2
    assert call(dn=None) == -2 and call(T=7) == -2 and call(slices=9) == -2 and call(zero_count=-1) == -2
    torch.cuda.synchronize()
    _check_keys(za, zb, 0, "refused launches")
    assert _all_nan(dn)


# ============================================================================================================ descriptors
def binned_gather(rows, n_img, grid):
    """rows [n_img * T, D] -> [n_img * T, 9 D]: the 3 x 3 replicate-clamped neighbourhood, row-major (dy, dx)"""
    D = rows.shape[-1]
    r = rows.view(n_img, grid, grid, D)
    idx = torch.arange(grid)
    cols = []
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            yy, xx = (idx + dy).clamp(0, grid - 1), (idx + dx).clamp(0, grid - 1)
            cols.append(r[:, yy][:, :, xx])
    return torch.cat(cols, dim=-1).reshape(n_img * grid * grid, 9 * D)


def descriptor_inputs(grid, P, n_img, D, zero_image):
    """x [n_img, P + T, D]; zero_image: the patch rows of image 0 are zero (every neighbourhood there is), its prefix rows not"""
    x = mk((n_img, P + grid * grid, D), _gen(grid, P, n_img, D))
    if zero_image:
        x[0, P:] = 0.0
    return x


@pytest.mark.parametrize("binned", [0, 1], ids=["plain", "binned"])
@pytest.mark.parametrize("D", [128, 384, 1024])
@pytest.mark.parametrize("grid", [1, 2, 3, 5])
def test_descriptors(lib, record_property, binned, grid, D):
    T = grid * grid
    Dp = 9 * D if binned else D
    key = "binned_dn" if binned else "plain_dn"
    worst = 0.0
    for P in (1, 5):
        for n_img in (1, 3):
            toks = n_img * T
            counts = (0, 1, T, toks * 64)
            for i, zero_image in enumerate((False, True)):
                what = f"P {P} n_img {n_img} zero image {zero_image}"
                xh = descriptor_inputs(grid, P, n_img, D, zero_image)
                rows = patch_rows_of(xh.view(-1, D), n_img, T, P)
                want_raw = binned_gather(rows, n_img, grid) if binned else rows
                x = xh.cuda()
                dn, raw = _nan32(toks + GUARD, Dp), _nan32(toks + GUARD, Dp)
                ws = _nan32(1, toks + GUARD)[0] if binned else None
                for zero_count in counts[2 * i:2 * i + 2]:
                    dn.fill_(float("nan"))
                    za, zb = _keys(toks * 64), _keys(toks * 64)
                    assert lib.vitvs_op_descriptors(ptr(x), ptr(dn), ptr(raw), ptr(ws), n_img, T, P, grid, D, binned, ptr(za), ptr(zb),
                                                    zero_count, stream()) == 0, what
                    torch.cuda.synchronize()
                    _check_keys(za, zb, zero_count, what)
                dc, rc_ = dn.cpu(), raw.cpu()
                assert _all_nan(dc[toks:]) and _all_nan(rc_[toks:]), f"{what}: rows beyond the last token were written"
                assert ws is None or _all_nan(ws.cpu()[toks:]), f"{what}: squared norms beyond the last token were written"
                assert torch.equal(_bits(rc_[:toks]), _bits(want_raw)), f"{what}: raw is not the gathered rows"
                assert torch.isfinite(dc[:toks]).all()
                if zero_image:
                    assert not dc[:T].any(), f"{what}: all-zero neighbourhoods do not give zeros"
                worst = max(worst, rel_max(dc[:toks], dn_ref(want_raw)))
                if binned:                       # the form of vitvs_extract_descriptors_ex_dev: raw only
                    raw.fill_(float("nan"))
                    assert lib.vitvs_op_descriptors(ptr(x), None, ptr(raw), ptr(ws), n_img, T, P, grid, D, 1, None, None, 0,
                                                    stream()) == 0, what
                    torch.cuda.synchronize()
                    rc_ = raw.cpu()
                    assert _all_nan(rc_[toks:]) and torch.equal(_bits(rc_[:toks]), _bits(want_raw)), f"{what}: raw-only form"
    _check(record_property, "dn", worst, BAR[key])


def test_descriptors_refusals(lib):
    x, dn, ws = torch.zeros((2 * 10, 128), device="cuda"), _nan32(18 + GUARD, 9 * 128), _nan32(1, 18 + GUARD)[0]
    za, zb = _keys(18 * 64 + 1), _keys(18 * 64 + 1)

    def call(binned, grid=3, zero_count=0, dn=dn):
        return lib.vitvs_op_descriptors(ptr(x), ptr(dn), None, ptr(ws), 2, 9, 1, grid, 128, binned, ptr(za), ptr(zb), zero_count, stream())
    for binned in (0, 1):
        assert call(binned, grid=2) == -2 and call(binned, grid=4) == -2          # grid * grid != T
        assert call(binned, zero_count=18 * 64 + 1) == -2
        assert call(binned, dn=None) == -2                                        # nothing to write
    torch.cuda.synchronize()
    _check_keys(za, zb, 0, "refused launches")
    assert _all_nan(dn) and _all_nan(ws)


def normalize_inputs(rows, Dp, zero_row):
    src = mk((rows, Dp), _gen(rows, Dp, zero_row), 3.0)
    if zero_row:
        src[rows // 2] = 0.0           # a zero row gives zeros
    return src


@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("Dp", [1, 63, 64, 65, 1152])
def test_normalize_rows(lib, record_property, Dp, rows):
    worst = 0.0
    for keep_zero_row in (True, False):
        src = normalize_inputs(rows, Dp, keep_zero_row)
        dst = _nan32(rows + GUARD, Dp)
        srcd = src.cuda()
        assert lib.vitvs_op_normalize_rows(ptr(srcd), ptr(dst), rows, Dp, stream()) == 0
        torch.cuda.synchronize()
        got = dst.cpu()
        assert _all_nan(got[rows:]), "rows beyond the last were written"
        assert torch.isfinite(got[:rows]).all()
        if keep_zero_row:
            assert not got[rows // 2].any(), "a zero row does not give zeros"
        if src.any():
            worst = max(worst, rel_max(got[:rows], dn_ref(src)))
    _check(record_property, "normalize", worst, BAR["normalize"])
    assert lib.vitvs_op_normalize_rows(ptr(srcd), ptr(dst), 0, Dp, stream()) == -2


# ================================================================================================================== facet
def facet_ref(v, n_img, T, P, H, which, unscale, keep_cls):
    """v fp32 [n_img * (P + T), 3 * 64 H] (the values of qkv) -> fp32 [n_img * (keep_cls + T), 64 H], index d * H + h"""
    D = 64 * H
    t = v.view(n_img, P + T, 3, H, 64)[:, :, which]                     # [n_img, P + T, H, 64]
    t = torch.cat([t[:, :1], t[:, P:]], dim=1) if keep_cls else t[:, P:]
    return (t.transpose(2, 3).reshape(-1, D) * torch.tensor(unscale, dtype=torch.float32)).contiguous()


@pytest.mark.parametrize("name,prec", PRECS)
@pytest.mark.parametrize("keep_cls", [0, 1])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_facet_is_the_fp32_statement(lib, record_property, name, prec, which, keep_cls):
    for P in (1, 5):
        for H in (2, 3):
            for T in (1, 9):
                for n_img in (1, 2):
                    D = 64 * H
                    qkv = _operand(prec, mk((n_img * (P + T), 3 * D), _gen(P, H, T, n_img)))
                    if prec == _lib.F16X2:       # load_x2: hi + lo, one fp32 addition
                        v = qkv.view(-1, 3 * D // 32, 2, 32)
                        vals = (v[:, :, 0].float() + v[:, :, 1].float()).reshape(-1, 3 * D)
                    else:
                        vals = qkv.float()
                    qd = qkv.cuda()
                    for unscale in (1.0, Q_UNSCALE):
                        rows = n_img * (T + keep_cls)
                        out = _nan32(rows + GUARD, D)
                        assert lib.vitvs_op_facet(prec, ptr(qd), ptr(out), n_img, T, P, H, which, unscale, keep_cls, stream()) == 0
                        torch.cuda.synchronize()
                        got = out.cpu()
                        what = f"P {P} H {H} T {T} n_img {n_img} unscale {unscale}"
                        assert _all_nan(got[rows:]), f"{what}: rows beyond the last were written"
                        assert torch.equal(_bits(got[:rows]), _bits(facet_ref(vals, n_img, T, P, H, which, unscale, keep_cls))), what
    record_property("facet", "0.000e+00")            # equality held in every launch
    assert lib.vitvs_op_facet(prec, ptr(qd), ptr(out), 1, 9, 1, 2, 3, 1.0, 0, stream()) == -2


# =============================================================================================================== saliency
SALIENCY_PRECS = PRECS[:3]
SALIENCY_H = 3
SALIENCY_HEADS = ([1], [0, 2], [2, 2, 0])
SCORE_SCALES = (4.0, 2.0)        # per image: the rows are peaked, and differently, so the per-image normalisation is visible


def saliency_inputs(prec, T, P, prescaled):
    """qkv [2 * (P + T), 3 * 64 H] in the precision: what the kernel reads and what the reference sees"""
    H, N = SALIENCY_H, P + T
    q = mk((2, N, 3 * 64 * H), _gen(T, P))
    for img, s in enumerate(SCORE_SCALES):
        q[img, :, :64 * H] *= s * (0.125 * LOG2E if prescaled else 1.0)
    return q.view(2 * N, -1).to(DTYPES[prec]).contiguous()


def _saliency(qkv, T, P, heads, prescaled, dt, H=SALIENCY_H, n_img=2):
    N = P + T
    v = qkv.to(dt).view(n_img, N, 3, H, 64)
    maps = []
    for img in range(n_img):
        acc = torch.zeros(T, dtype=dt)
        for h in heads:
            s = (v[img, :, 1, h] * v[img, 0, 0, h]).sum(-1)             # q_cls . k over all P + T keys
            s = s * math.log(2.0) if prescaled else s * 0.125           # 2^s = e^(s ln 2)
            acc = acc + s.softmax(0)[P:]                                # patch columns kept
        m = acc / len(heads)
        maps.append((m - m.min()) / (m.max() - m.min()))
    return torch.stack(maps)


def saliency_ref(qkv, T, P, heads, prescaled, **shape):
    return _saliency(qkv, T, P, heads, prescaled, torch.float64, **shape)


def saliency_f32(qkv, T, P, heads, prescaled, **shape):
    return _saliency(qkv, T, P, heads, prescaled, torch.float32, **shape)


@pytest.mark.parametrize("name,prec", SALIENCY_PRECS)
@pytest.mark.parametrize("P", [1, 5])
@pytest.mark.parametrize("T", [5, 255, 256, 257, 600])
def test_saliency(lib, record_property, name, prec, T, P):
    worst = 0.0
    for prescaled in (0, 1):
        qkv = saliency_inputs(prec, T, P, prescaled)
        qd = qkv.cuda()
        for heads in SALIENCY_HEADS:
            what = f"heads {heads} prescaled {prescaled}"
            out = _nan32(2 + GUARD, T)
            idx = (C.c_int32 * len(heads))(*heads)
            assert lib.vitvs_op_saliency(prec, ptr(qd), ptr(out), 2, T, P, SALIENCY_H, idx, len(heads), prescaled, stream()) == 0, what
            torch.cuda.synchronize()
            got = out.cpu()
            assert _all_nan(got[2:]), f"{what}: rows beyond the last image were written"
            ref = saliency_ref(qkv, T, P, heads, prescaled)
            for img in range(2):
                assert float(got[img].min()) == 0.0 and float(got[img].max()) == 1.0, f"{what}: image {img} is not min-max normalised"
                assert int(got[img].argmax()) == int(ref[img].argmax()), f"{what}: image {img} peaks elsewhere"
            worst = max(worst, float((got[:2].double() - ref).abs().max()))
    _check(record_property, "saliency", worst, BAR["saliency"])


def test_saliency_refusals(lib):
    T, P, H = 5, 1, SALIENCY_H
    qkv = torch.zeros((2 * (P + T), 3 * 64 * H), device="cuda")
    out = _nan32(2 + GUARD, T)

    def call(prec, heads, n=None):
        idx = (C.c_int32 * len(heads))(*heads)
        return lib.vitvs_op_saliency(prec, ptr(qkv), ptr(out), 2, T, P, H, idx, len(heads) if n is None else n, 0, stream())
    assert call(_lib.F16X2, [1]) == -2
    assert call(_lib.F32, [H]) == -2 and call(_lib.F32, [0, -1]) == -2          # a head outside 0 .. H - 1
    assert call(_lib.F32, [0] * 17) == -2 and call(_lib.F32, [0], n=0) == -2    # 1 .. 16 heads
    torch.cuda.synchronize()
    assert _all_nan(out)


# ================================================================================================== LayerNorm stress rows
LN_ROWS = 6
ORDINARY, OFFSET, SPIKE, CONSTANT = [0, 1], [2, 3], [4], [5]


def ln_stress_rows(D):
    """two ordinary rows, `+-1000 + randn`, one 300.0 spike among randn, one constant row of 2.0"""
    g = _gen(D, 77)
    x = mk((LN_ROWS, D), g)
    x[0:2] = x[0:2] * 3.0 + 0.7
    x[2] += 1000.0
    x[3] -= 1000.0
    x[4, D // 3] = 300.0
    x[5] = 2.0
    gamma, beta = 1.0 + 0.1 * mk((D,), g), 0.1 * mk((D,), g)
    return x, gamma, beta


def ln_stress_parts(D, slices):
    """x0, part [slices][6][D] and bias whose sum x0 + sum part + bias is close to the stress rows, and on the constant row
    exactly 2.0 whatever the order (dyadic terms)"""
    target, _, _ = ln_stress_rows(D)
    g = _gen(D, slices, 78)
    part = mk((slices, LN_ROWS, D), g, 0.3)
    bias = _dyadic(mk((D,), g, 0.3), 1024)
    part[:, 5] = _dyadic(part[:, 5], 1024)
    acc = part.double().sum(0) + bias.double()
    x0 = (target.double() - acc).float()
    assert torch.equal(x0[5].double() + acc[5], torch.full((D,), 2.0, dtype=torch.float64))
    return x0, part, bias, x0.double() + acc


def ln_f32(x, gamma, beta, eps=1e-6, one_pass=False):
    """The fp32 statement with 64-lane partial sums: lane l adds its elements l, l + 64, ... in order, the lanes are summed in a
    tree.  one_pass: the variance as E[x^2] - E[x]^2 instead of the mean of the squared deviations."""
    M, D = x.shape

    def wave_sum(v):
        lanes = torch.zeros((M, 64), dtype=torch.float32)
        for i in range(D // 64):
            lanes = lanes + v[:, i * 64:(i + 1) * 64]
        n = 64
        while n > 1:
            n //= 2
            lanes = lanes[:, :n] + lanes[:, n:2 * n]
        return lanes
    x = x.float()
    mean = wave_sum(x) / D
    var = wave_sum(x * x) / D - mean * mean if one_pass else wave_sum((x - mean) * (x - mean)) / D
    return (x - mean) * (1.0 / torch.sqrt(var + eps)) * gamma + beta


def _ulp(v, prec):
    """spacing of the 16-bit type at |v|"""
    mant, emin = (7, -126) if prec == _lib.BF16 else (10, -14)
    _, e = torch.frexp(v.double().abs().clamp_min(2.0 ** emin))
    return torch.pow(2.0, (e - 1 - mant).double())


def cast_excess(got, ref, prec):
    """worst |got - ref cast to the type| over what is allowed for it (see _check_ln_rows); got: values of the 16-bit type"""
    cast = ref.to(DTYPES[prec]).double()
    ulp = torch.maximum(_ulp(cast, prec), _ulp(got, prec))
    e = BAR_LN_OFFSET * ref.abs().amax(dim=-1, keepdim=True)
    allowed = torch.where(ulp >= e, ulp, e + ulp)
    return float(((got.double() - cast).abs() / allowed).max())


def _check_ln_rows(record, prec, tag, out, x_left, gamma, beta):
    """out: the launch's LayerNorm output rows in the precision; x_left: the fp32 rows it normalised"""
    ref = layer_norm64(x_left, gamma, beta)
    got = values(prec, out)
    assert torch.isfinite(got).all(), f"{tag}: non-finite outputs"
    if prec in BAR_LN16:
        _check(record, f"{tag}_all", max(rel_max(got[r], ref[r]) for r in range(LN_ROWS)), BAR_LN16[prec])
        # The value before the final cast: against the reference cast to the type.  Where the type resolves the fp32 bar of these
        # rows (ulp >= e = BAR_LN_OFFSET * max |ref|) an fp32 value within e of the reference rounds to the reference's 16-bit
        # number or a neighbour: one ulp.  On smaller elements both are rounded from within e of each other: e plus one ulp.
        excess = cast_excess(got, ref, prec)
        record(f"{tag}_cast_excess", f"{excess:.3f}")
        assert excess <= 1.0, f"{tag}: {excess:.2f} x the allowed distance from the reference cast to the type"
    else:
        for rows, bar, what in ((ORDINARY + SPIKE, BAR_LN[prec], "ordinary"), (OFFSET, BAR_LN_OFFSET, "offset")):
            _check(record, f"{tag}_{what}", max(rel_max(got[r], ref[r]) for r in rows), bar)
    # the constant row: sum, mean and deviations are exact, so out = beta rounded once
    want = _operand(prec, beta.view(1, -1))
    assert torch.equal(_bits(out[CONSTANT]), _bits(want)), f"{tag}: the constant row is not beta rounded once"


@pytest.mark.parametrize("name,prec", PRECS)
@pytest.mark.parametrize("slices", [1, 4, 8])
@pytest.mark.parametrize("D", WIDTHS)
def test_layernorm_stress_rows(lib, record_property, name, prec, D, slices):
    M = LN_ROWS
    rows, gamma, beta = ln_stress_rows(D)
    gd, bd = gamma.cuda(), beta.cuda()
    # vitvs_op_layernorm on the rows themselves
    xd, out = rows.cuda(), nan_like(prec, M + GUARD, D)
    assert lib.vitvs_op_layernorm(prec, ptr(xd), ptr(gd), ptr(bd), ptr(out), M, D, 1e-6, stream()) == 0
    torch.cuda.synchronize()
    out = out.cpu()
    assert _all_nan(out[M:]), "layernorm: rows beyond M were written"
    _check_ln_rows(record_property, prec, "layernorm", out[:M], rows, gamma, beta)
    # vitvs_op_residual_ln: the rows arrive as x0 + sum of `slices` hand-made partial sums + bias
    x0, part, bias, x_ref = ln_stress_parts(D, slices)
    x = torch.cat([x0, torch.full((GUARD, D), float("nan"))]).cuda()
    pd, biasd, out = part.cuda(), bias.cuda(), nan_like(prec, M + GUARD, D)
    assert lib.vitvs_op_residual_ln(prec, ptr(x), ptr(pd), slices, ptr(biasd), None, ptr(gd), ptr(bd), ptr(out), M, D, 1e-6, stream()) == 0
    torch.cuda.synchronize()
    x, out = x.cpu(), out.cpu()
    assert _all_nan(x[M:]) and _all_nan(out[M:]), "residual_ln: rows beyond M were written"
    _check(record_property, "residual_ln_x", max(rel_max(x[r], x_ref[r]) for r in range(M)), BAR_X[prec])
    assert torch.equal(x[CONSTANT], torch.full((1, D), 2.0)), "residual_ln: the constant row's sum is not exact"
    _check_ln_rows(record_property, prec, "residual_ln", out[:M], x[:M], gamma, beta)
