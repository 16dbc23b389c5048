"""Attention's key set, exactly: tails, ranges, images and heads (GPU).

Random operands make a softmax row close to uniform, and a key that is counted twice, masked or replicated into the padding then
stays under the 16-bit bars.  The inputs of tests/attention_keys_ref.py make softmax a two-key gather - one half of every row on
a chosen key, one half on the LAST key, the one clamped loads replicate - so that any such fault moves a row by >= 0.2
(tests/test_attention_keys_host.py proves that on the fp64 reference alone).  Every case of attention_keys_ref.CASES - the
smallest shapes that reach each kernel, each key-group and key-range arrangement, full and one-key last tiles - runs its
launches (two `every_key` shifts, the `tail` sweep over the last tile, two `tilted` shifts) through vitvs_op_attention, and in
bf16 / fp16 also through vitvs_op_attention_q in the forward's form, after the plan hook has confirmed under the case's in-flight
hint that the hook launches the kernel the case names.  Outputs start as NaN with guard rows behind them; the error is taken per
(token, head) row, max_d |got - ref| / max_d |ref|, and the worst ROW is held to the project's bars for attention (fp32 and f16x2
1e-5, bf16 2e-2, fp16 3e-3, fp16 with raw q from 512 tokens on 4e-3).  Divided cases launch twice back to back on one stream
and must repeat bit for bit (the workspace's tickets are left zero).  The VITVS_ATTN_ONES=1 variant of the long kernel is read
once per process, so a fresh child process runs the long-kernel cases under it.

Each case records its worst row error as a junit property (`--junitxml=FILE -o junit_family=legacy`).  Worst per kernel,
measured on an MI355X (raw q | forward's form):

    kernel                      bf16               fp16               f16x2     fp32
    short                       2.41e-3 | 2.11e-3  3.19e-4 | 2.86e-4  3.02e-7
    64-query, one key group     2.41e-3 | 2.50e-3  3.35e-4 | 2.92e-4  5.05e-7
    64-query, two key groups    2.41e-3 | 2.27e-3  3.34e-4 | 2.86e-4  1.39e-6
    long, whole items           3.19e-3 | 2.48e-3  3.69e-4 | 2.91e-4  1.48e-6
    long, divided               2.77e-3 | 2.49e-3  3.68e-4 | 3.31e-4
    fp32 kernel                                                                 1.55e-6

(an fp64 emulation of the 16-bit roundings the kernels document - q times the scale, P and the output rounded to the type - gives
3.2e-3 in bf16 and 3.7e-4 in fp16 on these inputs: the kernels sit at their formats' rounding.)  The module's 70 tests take 9 s.
"""
import ctypes as C
import os
import subprocess
import sys
import time

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:                     # the child process of the ONES test starts without pytest's conftest
    sys.path.insert(0, ROOT)

import vitvs_amd  # noqa: E402,F401
from vitvs_amd import _lib  # noqa: E402
from op_support import gpu_lib as lib  # noqa: F401
from op_support import ptr, stream

import attention_keys_ref as ak  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 3                 # rows behind every output that no launch may write
RUNS = [(c, form) for c in ak.CASES for form in (("raw", "forward") if c.prec in (ak.BF16, ak.F16) else ("raw",))]


def run_id(c, form):
    return f"{ak.case_id(c)}-{form}"


def bar(c, form):
    return ak.BAR_F16_RAW_LONG if (c.prec == ak.F16 and form == "raw" and c.N >= 512) else ak.BARS[c.prec]


def _launch(lib, c, form, x):
    """one launch into a fresh NaN output with guard rows; returns the output"""
    rows, D = c.n_img * c.N, c.H * 64
    out = torch.full((rows + GUARD, 2 * D if c.prec == ak.F16X2 else D), float("nan"), dtype=ak.DTYPES[c.prec], device="cuda")
    if form == "forward":
        rc = lib.vitvs_op_attention_q(c.prec, ptr(x), ptr(out), c.n_img, c.N, c.H, 1, stream())
    else:
        rc = lib.vitvs_op_attention(c.prec, ptr(x), ptr(out), c.n_img, c.N, c.H, stream())
    assert rc == 0, f"{run_id(c, form)}: launch returned {rc}"
    return out


def run_case(lib, c, form, record=None):
    """Every launch of a case, under its hint (restored whatever happens).  Returns the worst row error per family."""
    what = run_id(c, form)
    rows = c.n_img * c.N
    prev = lib.vitvs_op_plan_in_flight(c.hint)
    try:
        plan = (C.c_int32 * 6)()
        assert lib.vitvs_op_attention_plan(c.prec, c.n_img, c.N, c.H, plan) == 0
        assert ak.plan_key(c.prec, c.N, list(plan)) == ak.case_key(c), f"{what}: the hook plans {list(plan)} here, not the case's key"
        worst = {}
        for family, launch in ak.launches(c.N):
            fx = ak.fixture(c.n_img, c.N, c.H, family, launch)
            x, t = ak.operand(c.prec, fx.qkv, prescaled=form == "forward")
            xd = x.cuda()
            outs = [_launch(lib, c, form, xd) for _ in range(2 if c.divided else 1)]
            ref = ak.reference(t, c.n_img, c.N, c.H)              # on the CPU, while the launch runs
            torch.cuda.synchronize()
            where = f"{what} {family} {launch}"
            for out in outs:
                assert torch.isnan(out[rows:].float()).all(), f"{where}: rows beyond the last token were written"
                assert torch.isfinite(out[:rows].float()).all(), f"{where}: non-finite outputs"
            if c.divided:
                assert torch.equal(outs[0][:rows], outs[1][:rows]), f"{where}: two launches on one stream differ"
            got = ak.values(c.prec, outs[0][:rows].cpu())
            if c.N == 1:
                assert torch.equal(got, t[:, 2 * c.H * 64:]), f"{where}: one token must return its own v"
            err = ak.row_errors(got, ref, c.H)
            e = float(err.max())
            worst[family] = max(worst.get(family, 0.0), e)
            if e > bar(c, form):
                r, h = divmod(int(err.argmax()), c.H)
                raise AssertionError(f"{where}: row error {e:.3e} > {bar(c, form):g} at image {r // c.N} token {r % c.N} head {h} "
                                     f"(partner key {int(fx.a[r // c.N, h, r % c.N])}; {int((err > bar(c, form)).sum())} of "
                                     f"{err.numel()} rows over the bar)")
        if record:
            for family, e in worst.items():
                record(f"{family}_worst_row", f"{e:.3e}")
        return worst
    finally:
        lib.vitvs_op_plan_in_flight(prev)


@pytest.mark.parametrize("case,form", [pytest.param(c, f, id=run_id(c, f)) for c, f in RUNS])
def test_attention_keys_against_fp64(lib, record_property, case, form):
    run_case(lib, case, form, record_property)


def test_ones_variant_of_the_long_kernel_in_a_fresh_process(lib):
    """VITVS_ATTN_ONES=1 (row sums on the matrix pipe) is read once per process: a child runs the long-kernel cases under it."""
    env = dict(os.environ, VITVS_ATTN_ONES="1")
    res = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    print(res.stdout)
    print(res.stderr, file=sys.stderr)
    assert res.returncode == 0, f"the child exited with {res.returncode}:\n{res.stdout[-4000:]}\n{res.stderr[-4000:]}"
    assert "long-kernel runs ok" in res.stdout


def main():
    """The 16-bit long-kernel cases in this process (the ONES test's child); exit status 1 on a miss."""
    assert torch.cuda.is_available(), "needs a HIP device"
    lib = _lib.load()
    runs = [(c, f) for c, f in RUNS if c.kernel == ak.K_LONG and c.prec in (ak.BF16, ak.F16)]
    print(f"VITVS_ATTN_ONES={os.environ.get('VITVS_ATTN_ONES', '')}")
    bad = 0
    for c, form in runs:
        t0 = time.time()
        try:
            worst = run_case(lib, c, form)
            print(f"ok   {run_id(c, form)}: " + " ".join(f"{k} {v:.3e}" for k, v in worst.items()) + f"  ({time.time() - t0:.2f} s)")
        except AssertionError as exc:
            bad += 1
            print(f"MISS {exc}")
    print(f"{len(runs) - bad} of {len(runs)} long-kernel runs ok")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
