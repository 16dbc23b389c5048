"""Test infrastructure: attention inputs on which every key counts, their fp64 reference, and the faults they must expose.
Shared by tests/test_attention_keys_host.py (no GPU) and tests/test_gpu_attention_keys.py.  A reference, never shipped.

On random operands a softmax row is close to uniform: each of N keys carries ~1/N of it, and a key that is counted twice, masked,
or replicated into the padding moves the row by less than the 16-bit bars.  Here softmax is a two-key gather instead.  Per
(image, head), with N tokens:

  k[j], v[j]   every entry +-1, drawn per (image, head) from a seeded generator (another head's or image's K / V is wrong by O(1))
  q[i]         4 (k[a(i)] + k[N - 1]),  a(i) != N - 1

so q is 0 or +-8: every operand is exact in fp32, bf16, fp16 and the f16x2 hi / lo layout (lo = 0), and every q . k is an exact
integer in fp32.  The logits of the two partners a(i) and N - 1 are 32 + k[a(i)] . k[N - 1] / 2 both; every other key's is
N(0, 5.7).  A row's weight is therefore one half on key a(i) and one half on the LAST key, the one the kernels' clamped loads
(row min(j, N - 1)) replicate into the padding: a counted replica moves a row from 1/2 : 1/2 to 1/3 : 2/3, a masked last key to
1 : 0.  Both partners' V rows are +-1, so max |ref| of a row is ~1.

Families (the partner map a):

  every_key   a(i) = (i + c) mod (N - 1), c = shift + 7 (image H + head): over a launch every key 0 .. N - 2 is some query's partner
  tail        R keys in the last 64-key tile: launches c = 0 .. R - 2 with a(i) = N - 2 - ((i + c) mod (R - 1)): over the sweep every
              (query, real key of the last tile) pair is probed once.  R = 1: no launch (every_key covers the tile)
  tilted      every_key, and q[i] += k[a(i)] on head dimensions 0 .. 7 (q stays a small integer): key a(i) gains 1 nat, the last
              key 0.125 k[a(i)] . k[N - 1] over those dimensions, in [-1, 1]: the partners' logits differ by 0 .. 2 nats, so where
              they lie in different key groups or ranges the merge has unequal maxima to rescale

N = 1 is its own case: q = 8 k[0], and the output must equal v[0].

The fault models at the bottom act on the fp64 reference alone: tests/test_attention_keys_host.py asserts that each moves the
rows it touches by at least ten times the loosest attention bar, which is what makes the GPU comparison meaningful."""
from __future__ import annotations

import collections

import torch

from op_support import from_x2, to_x2, values  # noqa: F401

F32, BF16, F16, F16X2 = 0, 1, 2, 3               # vitvs_amd._lib's precision codes
K_F32, K_SHORT, K_Q64, K_Q64KS2, K_LONG = 1, 2, 3, 4, 5   # vitvs_op_attention_plan's kernel codes
PREC_NAMES = {F32: "fp32", BF16: "bf16", F16: "fp16", F16X2: "f16x2"}
DTYPES = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16, F16X2: torch.float16}
LOG2E = 1.4426950408889634
Q_FACTOR = 4.0                                    # q = Q_FACTOR (k[a] + k[N - 1]); the host test blunts it once, on purpose
SHIFTS = (0, 87)                                  # every_key / tilted: the diagonal, and one tile and 23 lanes further
# the project's bars for attention (tests/test_gpu_ops.py test_attention, tests/test_gpu_plan_cover.py BAR_ATTN)
BARS = {F32: 1e-5, BF16: 2e-2, F16: 3e-3, F16X2: 1e-5}
BAR_F16_RAW_LONG = 4e-3                           # fp16, raw q, N >= 512: the kernel rounds q * scale to 16 bits once more
SENSITIVITY = 0.2                                 # ten times the loosest bar

Case = collections.namedtuple("Case", "prec path n_img N H hint kernel divided ranges short")


def _cases():
    out = []
    for p in (BF16, F16):
        out += [Case(p, "short", n, N, H, 1, K_SHORT, 0, 1, 0) for n, N, H in ((1, 1, 1), (3, 37, 1), (2, 256, 2))]
        out += [Case(p, "q64", n, N, H, 1, K_Q64, 0, 1, 0) for n, N, H in ((81, 64, 2), (43, 100, 3))]
        out += [Case(p, "q64ks2", n, N, H, 1, K_Q64KS2, 0, 1, 0) for n, N, H in ((64, 81, 2), (36, 129, 2), (1, 257, 1), (1, 449, 1))]
        out += [Case(p, "long-whole", 43, 130, 2, 1, K_LONG, 0, 1, 0), Case(p, "long-whole", 1, 513, 1, 2, K_LONG, 0, 1, 0)]
        out += [Case(p, "long-divided", 1, 512, 1, 1, K_LONG, 1, 2, 0), Case(p, "long-divided", 1, 513, 1, 1, K_LONG, 1, 2, 1),
                Case(p, "long-divided", 1, 1000, 1, 1, K_LONG, 1, 4, 0), Case(p, "long-divided", 1, 1025, 1, 1, K_LONG, 1, 4, 1)]
    out += [Case(F16X2, "short", 3, 37, 1, 1, K_SHORT, 0, 1, 0)]
    out += [Case(F16X2, "q64", n, N, H, 1, K_Q64, 0, 1, 0) for n, N, H in ((43, 130, 2), (81, 64, 2))]
    out += [Case(F16X2, "q64ks2", n, N, H, 1, K_Q64KS2, 0, 1, 0) for n, N, H in ((36, 129, 2), (1, 513, 1))]
    out += [Case(F16X2, "long-whole", 1, 2049, 1, 1, K_LONG, 0, 1, 0)]
    out += [Case(F32, "f32", n, N, H, 1, K_F32, 0, 1, 0) for n, N, H in ((3, 37, 1), (43, 130, 2), (1, 513, 1))]
    return out


CASES = _cases()


def case_id(c: Case) -> str:
    return f"{PREC_NAMES[c.prec]}-{c.path}-{c.n_img}x{c.N}x{c.H}-hint{c.hint}"


def case_key(c: Case) -> list:
    """(precision, kernel, divided, key ranges, last range short): the key of tests/golden/plan_cover.json's attention rows."""
    return [c.prec, c.kernel, c.divided, c.ranges, c.short]


def plan_key(prec: int, N: int, plan) -> list:
    """The same key from vitvs_op_attention_plan's six outputs (tools/plan_cover.py attention_key)."""
    kernel, per, divided = plan[0], plan[4], plan[5]
    nt = (N + 63) // 64
    ranges = -(-nt // per) if per else 1
    return [prec, kernel, divided, ranges, int(ranges > 1 and nt % per != 0)]


# ---------------------------------------------------------------------------------------------------------------- the fixtures
Fixture = collections.namedtuple("Fixture", "family launch n_img N H a qkv")   # a [n_img, H, N] partner map, qkv [n_img N, 3 H 64] fp32


def last_tile_keys(N: int) -> int:
    return N - 64 * ((N - 1) // 64)


def launches(N: int) -> list:
    """(family, launch parameter) of every launch a case makes."""
    if N == 1:
        return [("every_key", 0)]
    return ([("every_key", s) for s in SHIFTS] + [("tail", c) for c in range(last_tile_keys(N) - 1)]
            + [("tilted", s) for s in SHIFTS])


_KV = {}


def _kv(n_img, N, H):
    """K and V of a shape, +-1, [n_img, H, N, 64] fp32: one draw per shape, shared by its families and launches."""
    key = (n_img, N, H)
    if key not in _KV:
        g = torch.Generator().manual_seed(1_000_003 * N + 1_009 * n_img + H)
        k = torch.randint(0, 2, (n_img, H, N, 64), generator=g).float() * 2 - 1
        v = torch.randint(0, 2, (n_img, H, N, 64), generator=g).float() * 2 - 1
        _KV[key] = (k, v)
    return _KV[key]


def partner_map(n_img, N, H, family, launch):
    i = torch.arange(N).expand(n_img, H, N)
    if N == 1:
        return torch.zeros_like(i)
    if family == "tail":
        R = last_tile_keys(N)
        assert 0 <= launch < R - 1
        return N - 2 - ((i + launch) % (R - 1))
    assert family in ("every_key", "tilted")
    pair = (torch.arange(n_img)[:, None] * H + torch.arange(H)[None, :])[:, :, None]
    return (i + launch + 7 * pair) % (N - 1)


def fixture(n_img, N, H, family, launch, q_factor=Q_FACTOR) -> Fixture:
    k, v = _kv(n_img, N, H)
    a = partner_map(n_img, N, H, family, launch)
    ka = torch.gather(k, 2, a[..., None].expand(-1, -1, -1, 64))
    q = q_factor * (ka + k[:, :, N - 1:N, :])
    if family == "tilted":
        q[..., :8] += ka[..., :8]
    qkv = torch.stack([q, k, v], dim=0).permute(1, 3, 0, 2, 4).reshape(n_img * N, 3 * H * 64).contiguous()
    return Fixture(family, launch, n_img, N, H, a, qkv)


# the f16x2 layout (csrc/common.h; the same helpers as tests/test_gpu_ops_x2.py and tests/test_gpu_plan_cover.py)


def operand(prec, qkv32, prescaled=False):
    """(what the kernel is given, the fp64 values the reference takes).  prescaled: the forward's 16-bit form, q carries
    0.125 log2(e), applied in fp32 before the one rounding to 16 bits; the reference divides it back in fp64."""
    D = qkv32.shape[1] // 3
    if prec == F16X2:
        assert not prescaled
        x = to_x2(qkv32)
        return x, from_x2(x)
    if prescaled:
        assert prec in (BF16, F16)
        qkv32 = qkv32.clone()
        qkv32[:, :D] *= 0.125 * LOG2E
    x = qkv32.to(DTYPES[prec]).contiguous()
    t = x.double()
    if prescaled:
        t[:, :D] /= 0.125 * LOG2E
    return x, t


# ---------------------------------------------------------------------------------------------------------------- the reference
def reference(qkv, n_img, N, H):
    """fp64 softmax attention of the values the kernel is given (tests/test_gpu_plan_cover.py _attention_ref)."""
    D = H * 64
    q, k, v = qkv.double().reshape(n_img, N, 3, H, 64).unbind(2)
    q, k, v = (t.transpose(1, 2) for t in (q, k, v))
    att = ((q @ k.transpose(-2, -1)) * 0.125).softmax(-1)
    return (att @ v).transpose(1, 2).reshape(n_img * N, D)


def row_errors(got, ref, H):
    """max_d |got - ref| / max_d |ref| per (token, head): [rows, H].  A tensor-wide maximum cannot excuse a row."""
    g, r = got.double().reshape(got.shape[0], H, 64), ref.double().reshape(ref.shape[0], H, 64)
    return (g - r).abs().amax(-1) / r.abs().amax(-1).clamp_min(1e-30)


# ---------------------------------------------------------------------------------------------------------------- fault models
class Softmax:
    """The reference taken apart, [image, head, query, ...] in fp64: p = exp(s - max_j s) per key, and per 64-key tile the partial
    numerators O_t = sum p v, denominators l_t = sum p and maxima of p.  A fault that reweighs keys is a cheap edit of these."""

    def __init__(self, fx: Fixture):
        self.fx = fx
        n_img, N, H = fx.n_img, fx.N, fx.H
        self.nt = nt = (N + 63) // 64
        q, k, v = fx.qkv.double().reshape(n_img, N, 3, H, 64).unbind(2)
        self.q, self.k, self.v = (t.transpose(1, 2).contiguous() for t in (q, k, v))
        self.s = (self.q @ self.k.transpose(-2, -1)) * 0.125
        self.p = torch.exp(self.s - self.s.amax(-1, keepdim=True))
        pad = nt * 64 - N
        pp = torch.nn.functional.pad(self.p, (0, pad)).reshape(n_img, H, N, nt, 64)
        vp = torch.nn.functional.pad(self.v, (0, 0, 0, pad)).reshape(n_img, H, nt, 64, 64)
        self.O_t = torch.einsum("bhqtj,bhtjd->bhqtd", pp, vp)
        self.l_t = pp.sum(-1)
        self.pmax_t = pp.amax(-1)
        self.O, self.L = self.O_t.sum(3), self.l_t.sum(3)
        self.ref = self.O / self.L[..., None]
        self.last = torch.full_like(fx.a, N - 1)

    def errors(self, out):
        """row errors [image, head, query] of a faulty output against the reference"""
        return (out - self.ref).abs().amax(-1) / self.ref.abs().amax(-1).clamp_min(1e-30)

    def _at(self, idx):
        return torch.gather(self.p, 3, idx[..., None])[..., 0], torch.gather(self.v, 2, idx[..., None].expand(-1, -1, -1, 64))

    def gap(self):
        """logit of key a(i) minus logit of the last key, in nats"""
        return torch.gather(self.s, 3, self.fx.a[..., None])[..., 0] - self.s[..., self.fx.N - 1]

    def reweigh_key(self, idx, factor):
        """key idx[i] counts `factor` times in row i (0: masked, 2: counted once more)"""
        p, v = self._at(idx)
        return (self.O + ((factor - 1) * p)[..., None] * v) / (self.L + (factor - 1) * p)[..., None]

    def reweigh_tile(self, t, factor):
        """the 64-key tile t counts `factor` times in every row (0: dropped, 2: counted twice)"""
        return (self.O + (factor - 1) * self.O_t[:, :, :, t]) / (self.L + (factor - 1) * self.l_t[:, :, :, t])[..., None]

    def owners(self, t, exactly_one=False):
        """rows with a partner in tile t (exactly_one: with one partner in it and one outside)"""
        ia, il = self.fx.a // 64 == t, self.last // 64 == t
        return (ia ^ il) if exactly_one else (ia | il)

    def unscaled_part(self, parts):
        """parts [image, head, query, tile]: the id of the key group / range that holds each tile, per query row.  The part that
        holds the LOWER partner is merged without rescaling to the common maximum, i.e. it counts exp(max - its own max) times.
        Returns (output, rows whose partners lie in different parts)."""
        gap = self.gap()
        low = torch.where(gap < 0, self.fx.a, self.last)
        part_a = torch.gather(parts, 3, (self.fx.a // 64)[..., None])[..., 0]
        part_l = torch.gather(parts, 3, (self.last // 64)[..., None])[..., 0]
        target = torch.gather(parts, 3, (low // 64)[..., None])
        mask = (parts == target).double()
        factor = 1.0 / (self.pmax_t * mask).amax(-1)               # p is relative to the row's maximum: exp(max - part's max)
        O_p, l_p = (self.O_t * mask[..., None]).sum(3), (self.l_t * mask).sum(3)
        out = (self.O + (factor - 1)[..., None] * O_p) / (self.L + (factor - 1) * l_p)[..., None]
        return out, part_a != part_l

    def other_operands(self, dim, which="kv"):
        """K and / or V taken from the neighbouring image (dim 0) or head (dim 1)"""
        k = self.k.roll(1, dim) if "k" in which else self.k
        v = self.v.roll(1, dim) if "v" in which else self.v
        return ((self.q @ k.transpose(-2, -1)) * 0.125).softmax(-1) @ v

    def swapped_values(self, idx, other):
        """the V rows of keys idx[i] and other[i] swapped, in row i"""
        p1, v1 = self._at(idx)
        p2, v2 = self._at(other)
        return (self.O + (p1 - p2)[..., None] * (v2 - v1)) / self.L[..., None]


def key_parts(case: Case, plan_per: int):
    """[image, head, query, tile] ids of the key sets whose online-softmax states the case's kernel merges: the key ranges of the
    divided long kernel (range g = tiles [g per, (g + 1) per) of the item-major list of (128-query block, tile) units, so a
    range may start inside one query block's keys and end inside the next one's), the two key groups of the two-group
    64-query kernel (tiles [0, ceil(nt / 2)) and the rest), and otherwise the 64-key tiles themselves (the short kernel gives
    each wave one tile and merges the waves; every other kernel rescales its running state tile by tile)."""
    n_img, N, H = case.n_img, case.N, case.H
    nt = (N + 63) // 64
    t = torch.arange(nt)
    if case.kernel == K_LONG and case.divided:
        nqb = (N + 127) // 128
        item = ((torch.arange(n_img)[:, None, None] * H + torch.arange(H)[None, :, None]) * nqb + (torch.arange(N) // 128)[None, None, :])
        return (item[..., None] * nt + t) // plan_per
    if case.kernel == K_Q64KS2:
        return (t // ((nt + 1) // 2)).expand(n_img, H, N, nt)
    return t.expand(n_img, H, N, nt)
