"""Exact inputs for the linear layers' GELU epilogue and for the hi / lo cross terms of f16x2: cases, operands, fp64 references,
the per-element bars and the fault models (no GPU; used by tests/test_epilogue_exact_host.py and
tests/test_gpu_epilogue_exact.py).

tests/gemm_exact_ref.py leaves two things to the randn tests, whose bars are fractions of max |ref| over a whole matrix:

GELU.  The store epilogue has two codes: gelu_erf (libm erff; fp32 and f16x2 outputs) and gelu_erf_fast (Abramowitz & Stegun
7.1.26 on rcpf / __expf; bf16 and fp16 outputs), the latter copied into BigStore::apply of csrc/gemm_big.hip.  A bf16 bar of
1.5e-2 of max |ref| hides a tanh-form GELU (4.7e-4 away at most), a coefficient wrong in its fourth digit, and an activation
dropped where |z| is small.  Here the PRE-ACTIVATION is exact: A = make_a, W = make_w / 4, bias[n] = c_n + j_n 2^-12 with c_n in
{-4, 0, 4} and j_n in [-2048, 2048), so z = A W^T + bias is a multiple of 2^-12 below 16 in magnitude, the same fp32 number in
every precision and summation order, and the fp64 reference is 0.5 z (1 + erf(z / sqrt 2)) of THAT z.  What is left is the
activation's own error and one rounding to the output type, and the comparison is per element (allowed() below).

f16x2 cross terms.  A contraction is lo.hi + hi.lo + hi.hi on three f16 MFMAs per k-step; integer operands have no low halves,
so two of the three multiply zeros in every case of gemm_exact_ref.  Here A = s (1 + l) at make_a's positions and W = w (1 + l)
with l hashed from {2^-12, 3 2^-13}: every hi / lo split is exact, both halves are non-zero, and every term of the mode's own
statement hi_A hi_W^T + hi_A lo_W^T + lo_A hi_W^T (no lo.lo) is a multiple of 2^-13, so fp32 accumulation is exact in any order
up to K = 1024 and the output's hi + lo holds the sum exactly: the comparison is ==.

Cases come from gemm_exact_ref (shapes, declared plans, packing): nothing here invents a shape.
  GELU_CASES   one store launch per (tile, k-groups, ring, precision, planned or forced): the row-edge sweeps' entry one full row
               tile plus 7 rows (behind 64 full tiles for the shallower ring), under the sweep's in-flight hint
  Both lists keep what the forward can launch (a key of tests/golden/plan_cover.json) or what vitvs_op_linear_variant forces.
  X2_CASES     the f16x2 store and partial cases of CASES with K <= 1024 and at most 2^21 outputs (one k-tile .. K = 1024;
               2, 3, 4, 6, 8 K slices; one and two k-groups; every tile of gemm_big.hip), and the same sweep entries for f16x2
f16x2 runs every case with weight exponent 0 and with the handle's rule (weight_exp): gemm_big.hip packs the exponent and the
GELU flag into one word.
"""
import json
import math
import os

import torch

import gemm_exact_ref as ge
from gemm_exact_ref import BF16, F16, F16X2, F32, STORE
from op_support import weight_exp  # noqa: F401  (the rule a handle applies to its f16x2 weights)

GUARD = 3                         # rows in front of and behind every output that no launch may write
X2_MAX_K, X2_MAX_OUT = 1024, 1 << 21
Z_RANGE = (-6, 6)                 # every unit interval in it holds at least Z_PER_UNIT distinct z per case
Z_PER_UNIT = 64
ULP_WINDOW = (-3.0, 8.0)          # z on which a 16-bit output must be the reference rounded to the type or its neighbour
NEIGHBOUR_CAP = 0.02              # ... and the share of neighbours allowed there (a cap, not a measurement)
MARGIN = 8                        # the ends cover's: rcpf / __expf / erff against the exact division, exp and erf of a restatement

SQRT1_2 = 0.70710678118654752440
AS_P = 0.3275911                  # Abramowitz & Stegun 7.1.26
AS_A = (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)
LIBM, FAST = "libm", "fast"
FORM = {F32: LIBM, F16X2: LIBM, BF16: FAST, F16: FAST}      # the code each output type runs (csrc/gemm.hip, csrc/gemm_big.hip)

# Worst implied erf error |g32(z) - g64(z)| / max(|z| / 2, 2^-11) of the torch fp32 restatement of each form (gelu_f32 below) over
# the z of all GELU cases, measured on the CPU; and the share of neighbours (see ULP_WINDOW) the fast restatement alone gives.
# tests/test_epilogue_exact_host.py re-measures all of them and fails when one is understated or more than twice the figure.
MEASURED_E = {LIBM: 2.0e-7, FAST: 5.7e-7}
MEASURED_SHARE = {BF16: 3.0e-4, F16: 1.9e-3}


# ------------------------------------------------------------------------------------------------ cases
def _edge(s):
    """the sweep's launch at one full row tile plus 7 rows"""
    want = s.rows[1] if s.rows else s.BM + 7
    return next(c for c in ge.sweep_cases(s) if c.M == want)


with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_cover.json")) as _fh:
    FORWARD_KEYS = {tuple(r["key"]) for r in json.load(_fh)["rows"] if r["kind"] == "linear"}


def _reached(c):
    """a launch the forward can make (a key of tests/golden/plan_cover.json), or a tile forced through vitvs_op_linear_variant"""
    return c.variant != 0 or tuple([c.prec, c.epi] + c.key) in FORWARD_KEYS


GELU_CASES = [c for c in (_edge(s) for s in ge.SWEEPS if s.epi == STORE) if _reached(c)]
X2_CASES = [c for c in ge.CASES if c.prec == F16X2 and c.dens == 8 and c.K <= X2_MAX_K and c.M * c.N <= X2_MAX_OUT] + \
           [_edge(s) for s in ge.SWEEPS if s.prec == F16X2]
X2_CASES = [c for c in X2_CASES if _reached(c)]


def case_id(c):
    return f"rows-{c.name}" if c.family == "rows" else ge.case_id(c)


def family(c):
    """the kernel instantiation a case runs, without its precision"""
    big, rows, cols, kg, stages = c.key[:5]
    name = f"big{rows}x{cols}" if big else f"gemm{rows}x{cols}-kg{kg}" + (f"-st{stages}" if stages else "")
    return name + ("-forced" if c.variant else "")


def exponents(c, W):
    """the weight exponents a case runs with: 0, and for f16x2 the handle's rule on these weights"""
    return [0, weight_exp(W)] if c.prec == F16X2 else [0]


# ------------------------------------------------------------------------------------------------ GELU: operands, reference, bars
def gelu_bias(N):
    """fp32 [N]: c_n + j_n 2^-12, c_n in {-4, 0, 4}, j_n in [-2048, 2048)"""
    n = torch.arange(N, dtype=torch.int64)
    z = torch.zeros_like(n)
    c = torch.tensor([-4.0, 0.0, 4.0], dtype=torch.float64)[ge._mix(n, z, 21) % 3]
    j = (ge._mix(n, z, 22) % 4096 - 2048).double()
    return (c + j * 2.0 ** -12).float()


def gelu_operands(c):
    """(A, W, bias, z): fp32 operands as the reference multiplies them, and the exact pre-activation in fp64"""
    A, W, bias = ge.make_a(c.M, c.K, c.dens), ge.make_w(c.N, c.K) * 0.25, gelu_bias(c.N)
    return A, W, bias, A.double() @ W.double().t() + bias.double()


def pack_w(prec, W, e=0):
    """what the kernel is given for the weights W, carrying 2^e (f16x2 only)"""
    return ge.pack(prec, W * 2.0 ** e)


def gelu64(z):
    z = z.double()
    return 0.5 * z * (1.0 + torch.erf(z * math.sqrt(0.5)))


def gelu_f32(form, z, a=AS_A):
    """the torch fp32 restatement of a form, in the kernel's expression order; a: the polynomial's coefficients"""
    v = z.float()
    if form == LIBM:
        return 0.5 * v * (1.0 + torch.erf(v * SQRT1_2))
    x = v.abs() * SQRT1_2
    t = 1.0 / (1.0 + AS_P * x)
    poly = t * (a[0] + t * (a[1] + t * (a[2] + t * (a[3] + t * a[4]))))
    e = 1.0 - poly * torch.exp(-x * x)
    return 0.5 * v * (1.0 + torch.copysign(e, v))


def half_z(z):
    """h = max(|z| / 2, 2^-11): what an erf error is multiplied by in 0.5 z (1 + erf)"""
    return (z.double().abs() / 2).clamp_min(2.0 ** -11)


def implied_erf_error(g, z):
    """worst |g - gelu64(z)| / h"""
    return float(((g.double() - gelu64(z)).abs() / half_z(z)).max())


def ulp32(v):
    _, e = torch.frexp(v.double().abs().clamp_min(2.0 ** -126))
    return torch.pow(2.0, (e - 24).double())


def ulp16(v, prec):
    """spacing of the 16-bit type at |v|"""
    mant, emin = (7, -126) if prec == BF16 else (10, -14)
    _, e = torch.frexp(v.double().abs().clamp_min(2.0 ** emin))
    return torch.pow(2.0, (e - 1 - mant).double())


def allowed(prec, z, ref, E=None):
    """The per-element bar on |got - ref|: one rounding to the output type plus MARGIN x the form's implied erf error.  fp32: a
    whole ulp, the fp32 expression rounds more than once; f16x2: and half a spacing of fp16's subnormals, where a low half ends."""
    e = MARGIN * (MEASURED_E if E is None else E)[FORM[prec]] * half_z(z)
    if prec == F32:
        return ulp32(ref) + e
    if prec == F16X2:
        return ulp32(ref) + e + 2.0 ** -25
    return ulp16(ref, prec) / 2 + e


def _ordered(t):
    """the 16-bit floats of t as integers in value order (-0 and +0 both 0)"""
    b = t.contiguous().view(torch.int16).int()
    return torch.where(b >= 0, b, -(b & 0x7FFF))


def output_values(prec, out):
    """fp64 values of a launch's output rows (f16x2: hi + lo)"""
    if prec == F16X2:
        hi, lo = ge.from_x2(out)
        return hi + lo
    return out.double()


def to_output(prec, v):
    """a model's fp64 / fp32 values as the output type would hold them (one rounding; f16x2: hi and lo of the fp32 value)"""
    return ge.to_x2(v.float()) if prec == F16X2 else v.to(ge.DTYPES[prec])


def gelu_verdict(prec, z, out, E=None):
    """(worst |got - ref| / allowed, share of one-ulp neighbours on ULP_WINDOW, outputs further than one ulp there).

    The second and third are for the 16-bit types only (0 otherwise).  Below z = -3 the factor 1 + erf cancels in fp32, for
    either form and for torch's own GELU: the output is then many ulps of ITS OWN size from the reference while still within
    the absolute bar, so there only the absolute bar applies.  Do not tighten that to ulps."""
    ref = gelu64(z)
    got = output_values(prec, out)
    ratio = float(((got - ref).abs() / allowed(prec, z, ref, E)).max())
    if prec not in (BF16, F16):
        return ratio, 0.0, 0
    window = (z >= ULP_WINDOW[0]) & (z <= ULP_WINDOW[1])
    steps = (_ordered(out) - _ordered(ref.to(ge.DTYPES[prec]))).abs()[window]
    return ratio, float((steps == 1).double().mean()), int((steps > 1).sum())


def erf_margin_used(prec, z, out):
    """worst (|got - ref| - the bar's rounding term) / (MARGIN x the form's implied erf error): the part of the margin a launch
    uses; at most 1 exactly when gelu_verdict's ratio is, negative where rounding alone explains every element"""
    ref = gelu64(z)
    e = MARGIN * MEASURED_E[FORM[prec]] * half_z(z)
    return float((((output_values(prec, out) - ref).abs() - (allowed(prec, z, ref) - e)) / e).max())


def describe_gelu_misses(c, z, out):
    """count and the first few elements beyond the per-element bar, with tile, wave and 16-row block"""
    ref = gelu64(z)
    got = output_values(c.prec, out)
    bad = ((got - ref).abs() > allowed(c.prec, z, ref)).nonzero()
    first = "; ".join(f"{ge.locate(c, int(m), int(n))} z {float(z[m, n]):g} got {float(got[m, n]):.9g} want {float(ref[m, n]):.9g} "
                      f"allowed {float(allowed(c.prec, z, ref)[m, n]):.3g}" for m, n in bad[:6].tolist())
    return f"{len(bad)} of {ref.numel()} elements are beyond the bar: {first}"


def z_coverage(z):
    """distinct z per unit interval of Z_RANGE"""
    u = torch.unique(z)
    return [int(((u >= a) & (u < a + 1)).sum()) for a in range(Z_RANGE[0], Z_RANGE[1])]


# ---- what a wrong epilogue would store (host test only): fp64 / fp32 values before the rounding to the output type
def fault_tanh(c, A, W, bias, z):
    return 0.5 * z * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (z + 0.044715 * z ** 3)))


def fault_bias_after(c, A, W, bias, z):
    return gelu64(z - bias.double()) + bias.double()


def fault_no_activation_block(c, A, W, bias, z):
    """the last 16-row block (in the ragged row tile) leaves without the activation"""
    g = gelu64(z)
    b0 = (c.M - 1) // 16 * 16
    g[b0:] = z[b0:]
    return g


def fault_coefficient(c, A, W, bias, z):
    """the fast form with its third coefficient rounded to four digits (1.421)"""
    return gelu_f32(FAST, z, AS_A[:2] + (1.421,) + AS_A[3:])


GELU_FAULTS = {           # name -> (model, the forms it applies to)
    "tanh-form": (fault_tanh, (LIBM, FAST)),
    "bias-after-activation": (fault_bias_after, (LIBM, FAST)),
    "no-activation-on-a-16-row-block": (fault_no_activation_block, (LIBM, FAST)),
    "coefficient-to-four-digits": (fault_coefficient, (FAST,)),
}


# ------------------------------------------------------------------------------------------------ f16x2 cross terms
def _low(a, b, seed):
    """l in {2^-12, 3 2^-13}, hashed"""
    return torch.where((ge._mix(a, b, seed) >> 9) & 1 == 1, 2.0 ** -12, 3 * 2.0 ** -13).double()


def x2_operands(c):
    """(A, W, bias, ls): A = s (1 + l) at make_a's positions, W = w (1 + l); bias and ls as gemm_exact_ref (integers)"""
    r = torch.arange(c.M, dtype=torch.int64)[:, None]
    ch = torch.arange(c.K // 8, dtype=torch.int64)[None, :]
    A = ge.make_a(c.M, c.K, 8).double() * (1.0 + _low(r, ch, 11).repeat_interleave(8, dim=1))
    n = torch.arange(c.N, dtype=torch.int64)[:, None]
    k = torch.arange(c.K, dtype=torch.int64)[None, :]
    W = ge.make_w(c.N, c.K).double() * (1.0 + _low(n, k, 12))
    bias, ls = ge.make_cols(c.N)
    return A.float(), W.float(), bias, ls


def split(t):
    """(hi, lo) fp64 of an fp32 matrix, as the f16x2 layout holds it"""
    hi = t.half().double()
    return hi, t.double() - hi


def _slices(c):
    s = max(c.slices, 1)
    ks = c.K // s
    return [slice(z * ks, (z + 1) * ks) for z in range(s)]


def x2_reference(c, A, W):
    """fp64 [slices, M, N]: the mode's statement hi.hi + hi.lo + lo.hi of every K slice (lo.lo is not part of it)"""
    (ah, al), (wh, wl) = split(A), split(W)
    return torch.stack([ah[:, k] @ wh[:, k].t() + ah[:, k] @ wl[:, k].t() + al[:, k] @ wh[:, k].t() for k in _slices(c)])


def x2_full_product(c, A, W):
    return torch.stack([A[:, k].double() @ W[:, k].double().t() for k in _slices(c)])


def x2_fp32_sums(c, A, W):
    """The same statement accumulated in fp32 in two orders: per 32-k tile lo.hi, hi.lo, hi.hi as the kernels issue them; and
    whole-K products over k reversed, hi.hi first."""
    (ah, al), (wh, wl) = (tuple(x.float() for x in split(t)) for t in (A, W))
    first, second = [], []
    for k in _slices(c):
        acc = torch.zeros(c.M, c.N, dtype=torch.float32)
        for k0 in range(k.start, k.stop, 32):
            t = slice(k0, k0 + 32)
            acc = acc + al[:, t] @ wh[:, t].t()
            acc = acc + ah[:, t] @ wl[:, t].t()
            acc = acc + ah[:, t] @ wh[:, t].t()
        first.append(acc)
        f = [x[:, k].flip(1) for x in (ah, al, wh, wl)]
        second.append((f[0] @ f[2].t() + f[0] @ f[3].t()) + f[1] @ f[2].t())
    return torch.stack(first), torch.stack(second)


def x2_fault_tile(c):
    """(slice, k-tile of it) the cross-term faults hit: the last slice's second k-tile (its only one where it has one)"""
    nk = c.K // max(c.slices, 1) // 32
    return max(c.slices, 1) - 1, min(1, nk - 1)


def x2_faults(c, A, W, ref):
    """name -> the reference with one cross-term fault in one 32-k tile of one slice (every output tile is touched)"""
    (ah, al), (wh, wl) = split(A), split(W)
    z, j = x2_fault_tile(c)
    ks = c.K // max(c.slices, 1)
    nk = ks // 32
    t = slice(z * ks + j * 32, z * ks + j * 32 + 32)
    hilo, lohi = ah[:, t] @ wl[:, t].t(), al[:, t] @ wh[:, t].t()

    def at(delta):
        out = ref.clone()
        out[z] += delta
        return out
    faults = {"hi.lo dropped": at(-hilo), "lo.hi dropped": at(-lohi), "lo.lo for lo.hi": at(al[:, t] @ wl[:, t].t() - lohi)}
    if nk > 1:      # low halves of the neighbouring 32-column group of the same slice
        o = (j + 1) % nk
        u = slice(z * ks + o * 32, z * ks + o * 32 + 32)
        faults["low halves of the neighbouring group"] = at(ah[:, t] @ wl[:, u].t() + al[:, u] @ wh[:, t].t() - hilo - lohi)
    return faults


def changed_share_per_tile(c, a, b):
    """the smallest share, over the case's output tiles, of elements on which a and b [M, N] differ"""
    bm, bn = ge.tile_geometry(c)[:2]
    worst = 1.0
    for m0 in range(0, c.M, bm):
        d = (a[m0:m0 + bm] != b[m0:m0 + bm]).double()
        worst = min(worst, float(d.reshape(d.shape[0], c.N // bn, bn).mean(dim=(0, 2)).min()))
    return worst
