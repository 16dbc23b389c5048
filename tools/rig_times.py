"""Device time of the rig law's kernel (rig.hip) at its seam, vitvs_op_rig_law, on random systems: 2 and 8 cameras x 24 feature
pairs (48 rows each), 8 cameras x a 1 700-pair dense selection (3 400 rows each), and 8 x 24 pairs of a rank-deficient stack (eight
equal cameras of two live pairs: the Jacobi fallback over the stacked rows); each as the one launch with its in-launch fan-in and
as two plain launches (vitvs_op_rig_two_launches: the cameras' sums, then the solve).

Times are HIP event pairs on the stream around ONE call (what a control loop waits for behind its velocity call), median / mean /
p10 / p90 over --reps calls after a warm-up, and around --burst calls back to back divided by their number (the event pair's own
cost amortised).  --rounds repeats everything, so the run-to-run spread of a line shows in one output.

    python tools/rig_times.py [--reps 200] [--rounds 3] [--burst 50]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import vitvs_amd  # noqa: E402,F401
from vitvs_amd import _lib, servo  # noqa: E402


def point_rows(x, y, Z):
    return np.array([[-1.0 / Z, 0.0, x / Z, x * y, -(1.0 + x * x), y], [0.0, -1.0 / Z, y / Z, 1.0 + y * y, -(x * y), -x]])


def rotation(w):
    th = np.linalg.norm(w)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    return np.eye(3) + (np.sin(th) / th) * K + ((1.0 - np.cos(th)) / (th * th)) * (K @ K)


def systems(rng, n, pairs, equal):
    """(rows [n], L [n][7][ld], W [n][36]) of n cameras with `pairs` random points each; equal: every camera the same two live pairs."""
    ld = 2 * pairs
    L = np.zeros((n, 7, ld))
    W = np.zeros((n, 36))
    v_star = rng.standard_normal(6)
    for i in range(n):
        if i == 0 or not equal:
            Wi = servo.twist_matrix(rotation(rng.uniform(-0.6, 0.6, 3)), rng.uniform(-0.3, 0.3, 3))
            live = 2 if equal else pairs
            Li = np.zeros((ld, 6))
            Li[:2 * live] = np.concatenate([point_rows(rng.uniform(-0.4, 0.4), rng.uniform(-0.4, 0.4), rng.uniform(0.5, 1.5))
                                            for _ in range(live)])
            e = Li @ Wi @ v_star + 1e-3 * rng.standard_normal(ld) * (np.abs(Li).sum(1) > 0)
        L[i, :6], L[i, 6], W[i] = Li.T, e, Wi.reshape(36)
    return np.full(n, ld, np.int32), L, W


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--burst", type=int, default=50)
    args = ap.parse_args()
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    print(f"library: {_lib.LIB_PATH}")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    for rnd in range(args.rounds):
        for n, pairs, equal, name in ((2, 24, False, "2 x 24 pairs"), (8, 24, False, "8 x 24 pairs"), (8, 1700, False, "8 x 1700 pairs"),
                                      (8, 24, True, "8 x 24 pairs, rank 4")):
            rows, L, W = (torch.as_tensor(a).to(dev) for a in systems(np.random.default_rng(7), n, pairs, equal))
            ld = 2 * pairs
            scratch = torch.zeros(lib.vitvs_op_rig_scratch_bytes(n, ld), dtype=torch.uint8, device=dev)
            v = torch.zeros(6, dtype=torch.float64, device=dev)
            st = torch.zeros(9, dtype=torch.int32, device=dev)
            normal = torch.zeros(28, dtype=torch.float64, device=dev)
            call = lambda: lib.vitvs_op_rig_law(n, p(rows), p(L), ld, p(W), 0.03, p(scratch), p(v), p(st), p(st[1:]), p(normal),  # noqa: E731
                                                C.c_void_p(stream.cuda_stream))
            results = {}
            for two in (0, 1):
                lib.vitvs_op_rig_two_launches(two)
                try:
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
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record(stream)
                        for _ in range(args.burst):
                            call()
                        b.record(stream)
                        b.synchronize()
                        burst = 1000 * a.elapsed_time(b) / args.burst
                finally:
                    lib.vitvs_op_rig_two_launches(0)
                results[two] = (v.cpu().numpy().copy(), st.cpu().numpy().copy())
                print(f"round {rnd} {name:22s} {'two launches' if two else 'fan-in      '}: median {np.median(us):7.2f} us, mean "
                      f"{np.mean(us):7.2f}, p10 {np.percentile(us, 10):7.2f}, p90 {np.percentile(us, 90):7.2f} over {len(us)} calls; "
                      f"{burst:7.2f} us per call in a burst of {args.burst}; sweeps {int(st[3])}, rows {int(st[2])}", flush=True)
            assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1])


if __name__ == "__main__":
    main()
