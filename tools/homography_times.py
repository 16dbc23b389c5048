"""Device time of the homography law's kernel (homography.hip) at its seam, vitvs_op_homography_law, on random points of a plane:
1 x 24 and 8 x 24 pairs (pairs of frames x feature rows) and one 1 x 3136 dense case, each with N = 0 and N = 4 Tukey re-weightings.
An eighth of the rows of the 24-row cases and 300 of the dense case are gross outliers, so the re-weightings have something to reject.

Times are HIP event pairs on the stream around ONE call (what a control loop waits for behind its velocity call), median / mean /
p10 / p90 over --reps calls after a warm-up, and around --burst calls back to back divided by their number (the event pair's own
cost amortised).  --rounds repeats everything, so the run-to-run spread of a line shows in one output.

--consensus M adds a second leg behind every line: the same call with the consensus start of M four-point hypotheses in front of its
solve loop (vitvs_op_homography_consensus_law), in the same run, so the legs without it are the yardstick; its output goes to
profiles/homography_consensus.txt.

    python tools/homography_times.py [--reps 200] [--rounds 3] [--burst 50] [--consensus M] [--out profiles/homography_law.txt]
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


def points(rng, n, rows, outliers):
    """(m, ms [n][rows][2], usable [n][rows]): per pair a random pose over the plane z = 0.61, m* the goal's normalised points, m the
    camera's + 0.002 noise."""
    m, ms = np.zeros((n, rows, 2)), np.zeros((n, rows, 2))
    for b in range(n):
        R, t = rotation(rng.normal(0.0, 0.2, 3)), rng.normal(0.0, 0.04, 3)
        X = np.stack([rng.uniform(-0.3, 0.3, rows), rng.uniform(-0.3, 0.3, rows), np.full(rows, 0.61)], 1)
        Xc = (X - t) @ R
        ms[b] = X[:, :2] / 0.61
        m[b] = Xc[:, :2] / Xc[:, 2:3] + 0.002 * rng.standard_normal((rows, 2))
        bad = rng.choice(rows, outliers, replace=False)
        m[b, bad] += rng.uniform(0.1, 0.4, (outliers, 2)) * rng.choice([-1.0, 1.0], (outliers, 2))
    return m, ms, np.ones((n, rows), np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--burst", type=int, default=50)
    ap.add_argument("--consensus", type=int, default=0, help="hypotheses of the consensus leg (0: no such leg)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "homography_consensus.txt" if args.consensus else "homography_law.txt")
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    lines = [f"homography law (vitvs_op_homography_law), {torch.cuda.get_device_name(dev)}; HIP event pairs, microseconds"]
    if args.consensus:
        lines[0] += f"; 'consensus {args.consensus}' lines: vitvs_op_homography_consensus_law with that many hypotheses, seed 0"
    print(lines[0])
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    for rnd in range(args.rounds):
        for n, rows, outliers in ((1, 24, 3), (8, 24, 3), (1, 3136, 300)):
            m, ms, usable = (torch.as_tensor(a).to(dev) for a in points(np.random.default_rng(7), n, rows, outliers))
            scratch = torch.zeros(lib.vitvs_op_homography_scratch_bytes(n, rows), dtype=torch.uint8, device=dev)
            v = torch.zeros((n, 6), dtype=torch.float64, device=dev)
            st = torch.zeros(n, dtype=torch.int32, device=dev)
            info = torch.zeros((n, 8), dtype=torch.int32, device=dev)
            H = torch.zeros((n, 9), dtype=torch.float64, device=dev)
            w = torch.zeros((n, rows), dtype=torch.float64, device=dev)
            sigma = torch.zeros(n, dtype=torch.float64, device=dev)
            for n_iter, n_hyp in [(N, M) for N in (0, 4) for M in ((0, args.consensus) if args.consensus else (0,))]:
                if n_hyp:
                    call = lambda: lib.vitvs_op_homography_consensus_law(n, rows, p(m), p(ms), p(usable), 0.03, 0.61, n_iter, 0.004,  # noqa: E731
                                                                         p(scratch), p(v), p(st), p(H), p(info), p(w), p(sigma),
                                                                         C.c_void_p(stream.cuda_stream), n_hyp, 0)
                else:
                    call = lambda: lib.vitvs_op_homography_law(n, rows, p(m), p(ms), p(usable), 0.03, 0.61, n_iter, 0.004,  # noqa: E731
                                                               p(scratch), p(v), p(st), p(H), p(info), p(w), p(sigma),
                                                               C.c_void_p(stream.cuda_stream))
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
                leg = f", consensus {n_hyp}" if n_hyp else ""
                line = (f"round {rnd} {n} x {rows:4d} rows, N = {n_iter}{leg}: median {np.median(us):7.2f} us, mean {np.mean(us):7.2f}, p10 "
                        f"{np.percentile(us, 10):7.2f}, p90 {np.percentile(us, 90):7.2f} over {len(us)} calls; {burst:7.2f} us per call in a "
                        f"burst of {args.burst}; pair 0: sweeps {int(i0[1])}, re-weightings {int(i0[2])}, zero weights {int(i0[3])}")
                if n_hyp:
                    line += f", winner {int(i0[6])}, start weights at 1: {int(i0[7])} of {int(i0[0])}"
                print(line, flush=True)
                lines.append(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
