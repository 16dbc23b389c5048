"""Device time of the pose rig law's kernel (pose_rig.hip pose_rig_kernel) at its seam, vitvs_op_pose_rig_law: 2 cameras x 24
rows, 8 x 24 and 2 x 1024 rows (the rank counting over 2048 values), one row in eight a gross outlier; N = 0 (the plain alignment)
and N = 4 re-weightings, i.e. N + 1 solves.

Times are HIP event pairs on the stream around ONE call, median / p10 / p90 over --reps calls after a warm-up; --rounds repeats
everything, so the run-to-run spread of a line shows in one output.  --out also writes the lines into a file.

    python tools/pose_rig_times.py [--reps 200] [--rounds 3] [--out profiles/pose_rig_law.txt]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vitvs_amd  # noqa: E402,F401
from vitvs_amd import _lib  # noqa: E402
import pose_rig_ref as rr  # noqa: E402

SMIN = 0.002


def systems(rng, n, rows):
    """(P, Q [n][rows][3], usable [n][rows], rTc [n][12]): a seeded rig and displacement, points 0.5 .. 1 m in front of it with
    2 mm of noise, one row in eight moved by 0.1 .. 0.4 m."""
    rig = rr.seeded_rig(rng, n)
    R, t = rr.seeded_displacement(rng)
    X = np.concatenate([rng.uniform(-0.4, 0.4, (n, rows, 2)), rng.uniform(0.5, 1.0, (n, rows, 1))], 2)
    P, Q = rr.camera_points(X, rig, R, t)
    P = P + 0.002 * rng.standard_normal(P.shape)
    for i in range(n):
        for k in rng.choice(rows, rows // 8, replace=False):
            P[i, k] += rr.unit(rng.standard_normal(3)) * rng.uniform(0.1, 0.4)
    return P, Q, np.ones((n, rows), np.int32), rr.rtc_rows(rig)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    lines = [f"library: {_lib.LIB_PATH}", f"device: {torch.cuda.get_device_name(dev)}"]
    print("\n".join(lines), flush=True)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    for rnd in range(args.rounds):
        for n, rows in ((2, 24), (8, 24), (2, 1024)):
            P, Q, usable, rtc = (torch.as_tensor(a).to(dev) for a in systems(np.random.default_rng(7), n, rows))
            scratch = torch.zeros(lib.vitvs_op_pose_rig_scratch_bytes(n, rows), dtype=torch.uint8, device=dev)
            v, pose, moments = (torch.zeros(k, dtype=torch.float64, device=dev) for k in (6, 12, 18))
            st = torch.zeros(9, dtype=torch.int32, device=dev)
            weights = torch.zeros((n, rows), dtype=torch.float64, device=dev)
            sigma = torch.zeros(1, dtype=torch.float64, device=dev)
            s = C.c_void_p(stream.cuda_stream)
            for N in (0, 4):
                plan = (C.c_int32 * 3)()
                assert lib.vitvs_op_pose_rig_plan(n, rows, N, plan) == 0
                call = lambda: lib.vitvs_op_pose_rig_law(n, rows, p(P), p(Q), p(usable), p(rtc), None, 0.35, N, SMIN, p(scratch),  # noqa: E731
                                                         p(v), p(st), p(pose), p(st[1:]), p(moments), p(weights), p(sigma), s)
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
                line = (f"round {rnd} {n} x {rows:4d} rows N = {N} (pose_rig_kernel<{int(N > 0)}>): median {np.median(us):8.2f} us, p10 "
                        f"{np.percentile(us, 10):8.2f}, p90 {np.percentile(us, 90):8.2f} over {len(us)} calls; LDS {plan[0]} B; status "
                        f"{int(info[0])}, usable {int(info[2])}, sweeps {int(info[3])}, re-weightings {int(info[4])}, zero weights "
                        f"{int(info[5])}")
                print(line, flush=True)
                lines.append(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
