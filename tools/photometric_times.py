"""The photometric law (photometric.hip, vitvs_photometric_velocity_dev) measured on the GPU:

  * device time of one call (its two launches) at 224 x 224 and 640 x 480, levels 0 .. 3, 1 and 8 pairs, with a depth image: HIP
    event pairs on the stream around ONE call, median / mean / p10 / p90 over --reps calls after a warm-up, and around --burst calls
    back to back divided by their number (the event pair's own cost amortised); --rounds repeats everything, so the run-to-run
    spread of a line shows in one output.  Beside each line: the bytes the call has to read (two frames and the depth image per pair)
    and what they come to per second of the burst time;
  * the rate of ``servo.Controller.ibvs()`` before the hand-over (the ViT update: two forwards, the correspondence, the law) and after
    it (the photometric law alone), host clock around calls that end in a read of the twist, on the closed-loop tests' scene
    (tests/closed_loop.py: ViT-S/16 224, fp32, subpatch, 640 x 480 camera);
  * with --loop: the two closed loops of tests/test_gpu_photometric_loop.py (their end points and the update of the hand-over) and
    the twist gap of tests/test_gpu_photometric_op.py (the device against the fp64 reference, and the reference against itself
    summed in reversed row order), computed by those tests' own code.

    python tools/photometric_times.py [--reps 200] [--rounds 2] [--burst 50] [--loop] [--out profiles/photometric.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))          # the closed-loop scaffold and the reference live with the tests
import vitvs_amd  # noqa: E402,F401
from vitvs_amd import _lib, config, synth  # noqa: E402
from vitvs_amd.engine import Engine  # noqa: E402


def op_times(args, lines):
    dev = torch.device("cuda", 0)
    cfg = config.baseline_config("vits16_224")
    eng = Engine(cfg, config.ServoParams(dino_input_size=cfg.img_size), precision="fp32", max_pairs=8)    # no weights: no forward runs
    stream = torch.cuda.Stream(dev)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    tex = synth.texture(640, 5)
    warped = synth.warp_similarity(tex, shift=(1.0, -0.7), rot_deg=0.8, scale=1.01, noise_sigma=1.0, seed=5)
    for rnd in range(args.rounds):
        for H, W in ((224, 224), (480, 640)):
            for n in (1, 8):
                cur = torch.from_numpy(np.ascontiguousarray(np.stack([warped[:H, :W]] * n))).to(dev)
                des = torch.from_numpy(np.ascontiguousarray(np.stack([tex[:H, :W]] * n))).to(dev)
                Z = torch.from_numpy(np.stack([synth.depth_pattern(H, W)] * n)).to(dev)
                K = torch.tensor([[500.0, 500.0, W / 2.0, H / 2.0]] * n, dtype=torch.float64, device=dev)
                v = torch.zeros((n, 6), dtype=torch.float64, device=dev)
                st = torch.zeros(n, dtype=torch.int32, device=dev)
                normal = torch.zeros((n, 28), dtype=torch.float64, device=dev)
                info = torch.zeros((n, 8), dtype=torch.int32, device=dev)
                for level in range(4):
                    call = lambda: lib_call(eng, n, p(cur), p(des), H, W, p(Z), p(K), level, p(v), p(st), p(normal), p(info), stream)  # noqa: E731
                    with torch.cuda.stream(stream):
                        for _ in range(20):
                            assert call() == 0, _lib.last_error(eng.handle)
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
                    assert not st.cpu().numpy().any()
                    i0 = info.cpu().numpy()[0]
                    mb = n * H * W * 8 / 1e6
                    line = (f"round {rnd} {n} x {H} x {W}, level {level}: median {np.median(us):7.2f} us, mean {np.mean(us):7.2f}, p10 "
                            f"{np.percentile(us, 10):7.2f}, p90 {np.percentile(us, 90):7.2f} over {len(us)} calls; {burst:7.2f} us per call in "
                            f"a burst of {args.burst}; {int(i0[3])} bands x {n}, {int(i0[0])} rows per pair; {mb:.2f} MB to read = "
                            f"{mb / burst * 1e3:.0f} GB/s of the burst time")
                    print(line, flush=True)
                    lines.append(line)
    eng.close()


def lib_call(eng, n, cur, des, H, W, Z, K, level, v, st, normal, info, stream):
    return eng.lib.vitvs_photometric_velocity_dev(eng.handle, n, cur, des, H, W, Z, 0.0, K, level, 1, 0.01, 0.5, v, st, normal, info,
                                                  C.c_void_p(stream.cuda_stream))


def ibvs_rates(args, lines):
    import closed_loop as cl
    for name, extra in (("before the hand-over (the ViT update)", {}),
                        ("after the hand-over (the photometric law alone)", dict(photometric_handover=1e9, photometric_lambda=0.5))):
        eng, _, ctl, sim = cl.set_up(dict(subpatch=True, **extra), "fp32", give_goal_depth=True)
        torch.manual_seed(121)
        sim.sense()
        for _ in range(10):
            ctl.ibvs()
        assert ctl.photometric_active == bool(extra)
        rates = []
        for _ in range(args.rounds + 1):
            t0 = time.perf_counter()
            for _ in range(args.reps):
                ctl.ibvs()
            rates.append(args.reps / (time.perf_counter() - t0))
        assert ctl.photometric_active == bool(extra) and ctl.v_c is not None
        line = (f"Controller.ibvs() {name}: " + ", ".join(f"{r:.1f}" for r in rates) + f" updates/s over {args.reps} calls each "
                f"(host clock; every call ends in a read of the twist)")
        print(line, flush=True)
        lines.append(line)
        eng.close()


def loops_and_gap(lines):
    import test_gpu_photometric_loop as tl
    import test_gpu_photometric_op as to
    import law_support as ls
    from vitvs_amd import weights
    plain, _, _, _ = tl.run_loop(0.0)
    fine, _, handed, statuses = tl.run_loop(tl.THRESHOLD)
    for name, tr in (("hand-over off", plain), ("hand-over on ", fine)):
        lines.append(f"closed loop fp32, subpatch, {name}: pose error (cm / deg) at updates 0, 10, .., {tl.UPDATES}: "
                     + "  ".join(f"{p:.4f}/{r:.4f}" for p, r in tr[::10]))
    lines.append(f"photometric_handover {tl.THRESHOLD}: hand-over behind update {handed} at {fine[handed + 1, 0]:.4f} cm / "
                 f"{fine[handed + 1, 1]:.4f} deg, {sum(s != 0 for s in statuses)} photometric updates not OK; after {tl.UPDATES} updates "
                 f"{plain[-1, 0]:.4f} cm / {plain[-1, 1]:.4f} deg without the hand-over, {fine[-1, 0]:.5f} cm / {fine[-1, 1]:.5f} deg with it")
    cfg = ls.tiny_cfg(64)
    eng = Engine(cfg, config.ServoParams(dino_input_size=64, use_feature_binning=False), precision="fp32", max_pairs=4, max_rows=48)
    eng.load_state_dict(weights.synthetic_state_dict(cfg, 0))
    gap_dev, gap_self, cases = 0.0, 0.0, to.SMALL + to.TAIL + to.FULL + to.WIDE
    for case in cases:
        ref, rev = to._reference(case), to._reference(case, True)
        v, _ = to._device(eng, case)
        norm = np.linalg.norm(ref["v"])
        gap_dev = max(gap_dev, float(np.linalg.norm(v - ref["v"]) / norm))
        gap_self = max(gap_self, float(np.linalg.norm(rev["v"] - ref["v"]) / norm))
    eng.close()
    lines.append(f"twist gap over the {len(cases)} cases of tests/test_gpu_photometric_op.py (relative L2, the largest): the device "
                 f"against the fp64 reference {gap_dev:.3e}; the reference against itself summed in reversed row order {gap_self:.3e}")
    for line in lines[-4:]:
        print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--burst", type=int, default=50)
    ap.add_argument("--loop", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "photometric.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    lines = [f"photometric law (vitvs_photometric_velocity_dev: photometric_rows_kernel + photometric_solve_kernel), "
             f"{torch.cuda.get_device_name(0)}; HIP event pairs, microseconds"]
    print(lines[0])
    op_times(args, lines)
    ibvs_rates(args, lines)
    if args.loop:
        loops_and_gap(lines)
    # what a call has to do, from the shapes (counted, not timed): per row 28 products and five fp64 divisions
    for H, W in ((224, 224), (480, 640)):
        for level in range(4):
            h, w = H >> level, W >> level
            rows = (h - 2) * (w - 2)
            per_band = max(1, min((2048 >> level) // w, h // 256))
            lines.append(f"counted, 1 x {H} x {W}, level {level}: up to {rows} rows = {28 * rows} fp64 products and {5 * rows} fp64 divisions; "
                         f"{H * W * 8 / 1e6:.2f} MB of frames and depth, the gradient image read {1 + 2.0 / per_band:.2f} times (halo rows), "
                         f"the other image and the depth once")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
