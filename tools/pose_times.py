"""Device time of the pose law's kernel (pose.hip) at its seam, vitvs_op_pose_law, on random points: 1 x 24 and 8 x 24 pairs
(pairs of frames x feature rows) and one 1 x 3136 dense case, each with N = 0 and N = 4 Tukey re-weightings.  A sixth of the rows of
the 24-row cases and 300 of the dense case are gross outliers, so the re-weightings have something to reject.

Times are HIP event pairs on the stream around ONE call (what a control loop waits for behind its velocity call), median / mean /
p10 / p90 over --reps calls after a warm-up, and around --burst calls back to back divided by their number (the event pair's own
cost amortised).  --rounds repeats everything, so the run-to-run spread of a line shows in one output.

--consensus M adds, behind every leg, the same leg with the consensus start of M three-point hypotheses
(vitvs_op_pose_consensus_law, seed 0): the legs without it are the yardstick of the same run.

    python tools/pose_times.py [--reps 200] [--rounds 3] [--burst 50] [--consensus 0] [--out profiles/pose_law.txt]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import vitvs_amd  # noqa: E402,F401
from vitvs_amd import _lib  # noqa: E402


def rotation(w):
    th = np.linalg.norm(w)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    return np.eye(3) + (np.sin(th) / th) * K + ((1.0 - np.cos(th)) / (th * th)) * (K @ K)


def clouds(rng, n, rows, outliers):
    """(P, Q [n][rows][3], usable [n][rows]): per pair a random pose, Q at 0.5 - 0.8 m, P = Q in the camera + 2 mm noise."""
    P, Q = np.zeros((n, rows, 3)), np.zeros((n, rows, 3))
    for b in range(n):
        R, t = rotation(rng.uniform(-0.5, 0.5, 3)), rng.uniform(-0.08, 0.08, 3)
        Z = rng.uniform(0.5, 0.8, rows)
        Q[b] = np.stack([rng.uniform(-0.4, 0.4, rows) * Z, rng.uniform(-0.3, 0.3, rows) * Z, Z], 1)
        P[b] = (Q[b] - t) @ R + 0.002 * rng.standard_normal((rows, 3))
        bad = rng.choice(rows, outliers, replace=False)
        P[b, bad] += rng.uniform(-0.3, 0.3, (outliers, 3))
    return P, Q, np.ones((n, rows), np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--burst", type=int, default=50)
    ap.add_argument("--consensus", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_law.txt"))
    args = ap.parse_args()
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    lines = [f"pose law (vitvs_op_pose_consensus_law; consensus 0 is vitvs_op_pose_law), {torch.cuda.get_device_name(dev)}; HIP event pairs, microseconds"]
    print(lines[0])
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    for rnd in range(args.rounds):
        for n, rows, outliers in ((1, 24, 4), (8, 24, 4), (1, 3136, 300)):
            P, Q, usable = (torch.as_tensor(a).to(dev) for a in clouds(np.random.default_rng(7), n, rows, outliers))
            scratch = torch.zeros(lib.vitvs_op_pose_scratch_bytes(n, rows), dtype=torch.uint8, device=dev)
            v = torch.zeros((n, 6), dtype=torch.float64, device=dev)
            st = torch.zeros(n, dtype=torch.int32, device=dev)
            info = torch.zeros((n, 8), dtype=torch.int32, device=dev)
            pose = torch.zeros((n, 12), dtype=torch.float64, device=dev)
            w = torch.zeros((n, rows), dtype=torch.float64, device=dev)
            sigma = torch.zeros(n, dtype=torch.float64, device=dev)
            for n_iter, n_hyp in [(N, M) for N in (0, 4) for M in sorted({0, args.consensus})]:
                call = lambda: lib.vitvs_op_pose_consensus_law(n, rows, p(P), p(Q), p(usable), 0.03, n_iter, 0.004, p(scratch), p(v),  # noqa: E731
                                                               p(st), p(pose), p(info), p(w), p(sigma), C.c_void_p(stream.cuda_stream),
                                                               n_hyp, 0)
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
                i0 = info.cpu().numpy()[0]
                assert not st.cpu().numpy().any()
                line = (f"round {rnd} {n} x {rows:4d} rows, N = {n_iter}, consensus {n_hyp:3d}: median {np.median(us):7.2f} us, mean {np.mean(us):7.2f}, p10 "
                        f"{np.percentile(us, 10):7.2f}, p90 {np.percentile(us, 90):7.2f} over {len(us)} calls; {burst:7.2f} us per call in a "
                        f"burst of {args.burst}; pair 0: sweeps {int(i0[1])}, re-weightings {int(i0[2])}, zero weights {int(i0[3])}, winner {int(i0[6])}, "
                        f"start weights {int(i0[7])}")
                print(line, flush=True)
                lines.append(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
