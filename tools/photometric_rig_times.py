"""The photometric rig law (photometric.hip, vitvs_photometric_rig_velocity_dev) measured on the GPU against the
robust photometric law with one pair per camera, on the same box in the same run:

  * device time of one call at 224 x 224 and 640 x 480, levels 0 and 2, 1, 3 and 8 cameras, with a depth image, every current frame
    under "gain+bias and block": the batched robust call with n_pairs = n_cams (3 N + 2 launches), then the rig call (4 N + 2
    launches), both with ``illumination`` and N = 0 .. 4 re-weightings.  HIP event pairs on the stream around ONE call, median over
    --reps calls after a warm-up;
  * with --loop: the closed loop of tests/test_gpu_photometric_rig_loop.py and the gaps of tests/test_gpu_photometric_rig_op.py (the
    device against the fp64 reference, and the reference against itself summed in reversed order), by those tests' own code;
  * the compiler's resource report of the law's two kernels (VGPRs, scratch, LDS), from a compilation of photometric.hip with
    -Rpass-analysis=kernel-resource-usage into a temporary directory (--no-resources skips it; --resources-only needs no GPU).

    python tools/photometric_rig_times.py [--reps 200] [--loop] [--out profiles/photometric_rig.txt]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vitvs_amd  # noqa: E402,F401
from vitvs_amd import _lib, config, servo, synth  # noqa: E402
from vitvs_amd.engine import Engine  # noqa: E402
from photometric_robust_times import disturbed, median_us, resources  # noqa: E402


def ring(n):
    """n cameras on a ring of 15 cm about the rig's z axis, each turned about it."""
    out = []
    for i in range(n):
        a = 2 * np.pi * i / max(n, 1)
        c, s = np.cos(0.3 * i), np.sin(0.3 * i)
        out.append(servo.twist_matrix(np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]), np.array([0.15 * np.cos(a), 0.15 * np.sin(a), 0.0])))
    return np.stack(out)


def op_times(args, lines):
    dev = torch.device("cuda", 0)
    cfg = config.baseline_config("vits16_224")
    eng = Engine(cfg, config.ServoParams(dino_input_size=cfg.img_size), precision="fp32", max_pairs=8)    # no weights: no forward runs
    stream = torch.cuda.Stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    tex = synth.texture(640, 5)
    warped = synth.warp_similarity(tex, shift=(1.0, -0.7), rot_deg=0.8, scale=1.01, noise_sigma=1.0, seed=5)
    lib, h = eng.lib, eng.handle
    for H, W in ((224, 224), (480, 640)):
        for n in (1, 3, 8):
            cur = torch.from_numpy(np.ascontiguousarray(np.stack([disturbed(warped[:H, :W])] * n))).to(dev)
            des = torch.from_numpy(np.ascontiguousarray(np.stack([tex[:H, :W]] * n))).to(dev)
            Z = torch.from_numpy(np.stack([synth.depth_pattern(H, W)] * n)).to(dev)
            K = torch.tensor([[500.0, 500.0, W / 2.0, H / 2.0]] * n, dtype=torch.float64, device=dev)
            cVr = torch.from_numpy(ring(n)).to(dev)
            v = torch.zeros((n, 6), dtype=torch.float64, device=dev)
            st = torch.zeros(n, dtype=torch.int32, device=dev)
            normal = torch.zeros((n, 45), dtype=torch.float64, device=dev)
            robust = torch.zeros((n, 4), dtype=torch.float64, device=dev)
            info = torch.zeros((n, 8), dtype=torch.int32, device=dev)
            rig_normal = torch.zeros(28, dtype=torch.float64, device=dev)
            for level in (0, 2):
                batched, rig = [], []
                for N in range(5):
                    batched.append(median_us(lambda: lib.vitvs_photometric_robust_velocity_dev(
                        h, n, p(cur), p(des), H, W, p(Z), 0.0, p(K), level, 1, 0.01, 0.5, 1, N, 1.0, p(v), p(st), p(robust), p(normal), p(info),
                        sp), stream, args.reps))
                    assert not st.cpu().numpy().any(), _lib.last_error(h)
                    rig.append(median_us(lambda: lib.vitvs_photometric_rig_velocity_dev(
                        h, n, p(cur), p(des), H, W, p(Z), 0.0, p(K), p(cVr), None, level, 1, 0.01, 0.5, 1, N, 1.0, p(v), p(st), p(robust),
                        p(normal), p(rig_normal), p(info), sp), stream, args.reps))
                    assert int(st.cpu().numpy()[0]) == 0, _lib.last_error(h)
                i0 = info.cpu().numpy()[0]
                line = (f"{n} x {H} x {W}, level {level}, illumination, N = 0 .. 4: batched robust " + " ".join(f"{t:7.2f}" for t in batched)
                        + " us; rig " + " ".join(f"{t:7.2f}" for t in rig) + " us; rig - batched " + " ".join(f"{r - b:6.2f}" for r, b in zip(rig, batched))
                        + f" us; N = 4: {int(i0[2])} of {int(i0[1])} rows of the stack at weight 0")
                print(line, flush=True)
                lines.append(line)
    eng.close()


def loop_and_gaps(lines):
    import test_gpu_photometric_rig_loop as tl
    import test_gpu_photometric_rig_op as to
    import photometric_rig_cases as pc
    import photometric_rig_scene as rs
    import law_support as ls
    from vitvs_amd import weights
    for name, (illum, N) in (("illumination, N = 4", (True, 4)), ("no illumination, N = 0", (False, 0))):
        track, handed, seen = tl.run_loop(illum, N)
        last = seen[-1]
        lines.append(f"closed loop fp32, three cameras under three lightings, 60 % of camera 0 covered, rig hand-over ({name}): pose error "
                     f"(cm / deg) at updates 0, 5, .., {rs.UPDATES}: " + "  ".join(f"{p:.4f}/{r:.4f}" for p, r in track[::5]))
        lines.append(f"    hand-over behind update {handed}, {sum(s['status'] != 0 for s in seen)} photometric updates not OK; the last update: "
                     f"gains {np.round(last['gain'], 4).tolist()}, biases {np.round(last['bias'], 3).tolist()}, sigma {last['sigma']:.3f}, rejected "
                     f"{np.round(last['rejected'], 4).tolist()}")
    cfg = ls.tiny_cfg(64)
    eng = Engine(cfg, config.ServoParams(dino_input_size=64, use_feature_binning=False), precision="fp32", max_pairs=5, max_rows=48)
    eng.load_state_dict(weights.synthetic_state_dict(cfg, 0))
    gap_dev, gap_self = np.zeros(4), np.zeros(4)
    for name, illum, N in pc.RUNS:
        ref, rev = pc.reference(name, illum, N), pc.reference(name, illum, N, True)
        v, info = to._call(eng, name, illum, N)
        gap_dev = np.maximum(gap_dev, to._gaps(v, info["gamma"], info["bias"], info["weight"], ref))
        gap_self = np.maximum(gap_self, to._gaps(rev["v"], rev["robust"][:, 0], rev["robust"][:, 1], rev["robust"][:, 3], ref))
    eng.close()
    lines.append(f"gaps over the {len(pc.RUNS)} runs of tests/test_gpu_photometric_rig_op.py (v_rig relative L2, gamma, beta, sum w relative; the "
                 f"largest): the device against the fp64 reference " + " ".join(f"{g:.3e}" for g in gap_dev)
                 + "; the reference against itself summed in reversed order " + " ".join(f"{g:.3e}" for g in gap_self))
    for line in lines[-5:]:
        print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--loop", action="store_true")
    ap.add_argument("--no-resources", action="store_true")
    ap.add_argument("--resources-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "photometric_rig.txt"))
    args = ap.parse_args()
    lines = []
    if not args.resources_only:
        assert torch.cuda.is_available(), "a measurement needs the GPU"
        lines.append(f"photometric rig law (vitvs_photometric_rig_velocity_dev: 4 N + 2 launches) against the robust photometric law with one "
                     f"pair per camera (vitvs_photometric_robust_velocity_dev: 3 N + 2 launches), {torch.cuda.get_device_name(0)}; HIP event "
                     f"pairs around one call, median of {args.reps}, microseconds; every current frame under gain+bias and a block, sigma_min 1")
        print(lines[0])
        op_times(args, lines)
        if args.loop:
            loop_and_gaps(lines)
    if not args.no_resources:
        every = []
        resources(every)
        lines += [ln for ln in every if "photometric_rig" in ln]
    if args.out:
        with open(args.out, "a" if args.resources_only else "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
