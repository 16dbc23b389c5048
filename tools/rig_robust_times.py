"""Device time of the robust rig law's kernel (rig.hip rig_robust_kernel) at its seam, vitvs_op_rig_robust_law, beside the plain
rig law's (vitvs_op_rig_law, rig_kernel<0>) on the same systems: 8 cameras x 24 feature pairs (the stack's copy LDS-resident)
and 2 cameras x 1024 pairs (the global work copy, the rank counting over 2048 values), one pair in eight a gross outlier;
N = 0 (the plain law), 1, 4 and 16 re-weightings, i.e. N + 1 solves.

Times are HIP event pairs on the stream around ONE call, median / p10 / p90 over --reps calls after a warm-up; --rounds repeats
everything, so the run-to-run spread of a line shows in one output.

    python tools/rig_robust_times.py [--reps 200] [--rounds 3]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import vitvs_amd  # noqa: E402,F401
from vitvs_amd import _lib  # noqa: E402
from rig_times import point_rows, rotation  # noqa: E402
from vitvs_amd import servo  # noqa: E402

SMIN = 0.002


def systems(rng, n, pairs):
    """(rows [n], L [n][7][ld], W [n][36]): n cameras of `pairs` random points following one rig twist up to +-0.005, one pair in
    eight with a gross error."""
    ld = 2 * pairs
    L, W = np.zeros((n, 7, ld)), np.zeros((n, 36))
    v = rng.standard_normal(6) * 0.1
    for i in range(n):
        Wi = servo.twist_matrix(rotation(rng.uniform(-0.6, 0.6, 3)), rng.uniform(-0.3, 0.3, 3))
        Li = np.concatenate([point_rows(rng.uniform(-0.4, 0.4), rng.uniform(-0.4, 0.4), rng.uniform(0.5, 1.5)) for _ in range(pairs)])
        e = Li @ Wi @ v + rng.uniform(-0.005, 0.005, ld)
        for k in rng.choice(pairs, pairs // 8, replace=False):
            a, m = rng.uniform(0, 2 * np.pi), rng.uniform(0.3, 0.8)
            e[2 * k] += m * np.cos(a)
            e[2 * k + 1] += m * np.sin(a)
        L[i, :6], L[i, 6], W[i] = Li.T, e, Wi.reshape(36)
    return np.full(n, ld, np.int32), L, W


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    print(f"library: {_lib.LIB_PATH}")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    for rnd in range(args.rounds):
        for n, pairs, name in ((8, 24, "8 x 24 pairs"), (2, 1024, "2 x 1024 pairs")):
            rows, L, W = (torch.as_tensor(a).to(dev) for a in systems(np.random.default_rng(7), n, pairs))
            ld = 2 * pairs
            plan = (C.c_int32 * 4)()
            assert lib.vitvs_op_rig_robust_plan(n, ld, plan) == 0
            scratch = torch.zeros(lib.vitvs_op_rig_robust_scratch_bytes(n, ld), dtype=torch.uint8, device=dev)
            v = torch.zeros(6, dtype=torch.float64, device=dev)
            st = torch.zeros(9, dtype=torch.int32, device=dev)
            normal = torch.zeros(28, dtype=torch.float64, device=dev)
            weights = torch.zeros((n, pairs), dtype=torch.float64, device=dev)
            sigma = torch.zeros(1, dtype=torch.float64, device=dev)
            s = C.c_void_p(stream.cuda_stream)
            for N in (0, 1, 4, 16):
                if N == 0:
                    call = lambda: lib.vitvs_op_rig_law(n, p(rows), p(L), ld, p(W), 0.35, p(scratch), p(v), p(st), p(st[1:]),  # noqa: E731
                                                        p(normal), s)
                else:
                    call = lambda: lib.vitvs_op_rig_robust_law(n, p(rows), None, p(L), ld, p(W), 0.35, N, SMIN, p(scratch), p(v),  # noqa: E731
                                                               p(st), p(st[1:]), p(normal), p(weights), p(sigma), s)
                with torch.cuda.stream(stream):
                    for _ in range(20):
                        assert call() == 0
                    stream.synchronize()
                    us = []
                    for _ in range(args.reps):
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record(stream)
                        call()
                        b.record(stream)
                        b.synchronize()
                        us.append(1000 * a.elapsed_time(b))
                info = st.cpu().numpy()
                print(f"round {rnd} {name:16s} N = {N:2d} ({'rig_kernel<0>    ' if N == 0 else 'rig_robust_kernel'}): median "
                      f"{np.median(us):8.2f} us, p10 {np.percentile(us, 10):8.2f}, p90 {np.percentile(us, 90):8.2f} over {len(us)} calls; "
                      f"LDS {plan[0] if N else 0} B, stack {'in LDS' if plan[1] else 'in the work block'}; rows {int(info[2])}, "
                      f"sweeps {int(info[3])}, re-weightings {int(info[6])}, zero weights {int(info[7])}", flush=True)


if __name__ == "__main__":
    main()
