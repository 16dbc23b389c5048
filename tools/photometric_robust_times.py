"""The robust photometric law (photometric.hip, vitvs_photometric_robust_velocity_dev) measured on the GPU against the
plain law on the same box in the same run:

  * device time of one call at 224 x 224 and 640 x 480, levels 0 and 2, 1 and 8 pairs, with a depth image, the current frame under
    "gain+bias and block": the plain call (2 launches), then the robust call with N = 0 .. 4 re-weightings (3 N + 2 launches), without
    and with ``illumination``.  HIP event pairs on the stream around ONE call, median over --reps calls after a warm-up;
  * with --loop: the closed loop of tests/test_gpu_photometric_robust_loop.py and the gaps of tests/test_gpu_photometric_robust_op.py
    (the device against the fp64 reference, and the reference against itself summed in reversed row order), by those tests' own code;
  * the compiler's resource report of the law's kernels (VGPRs, scratch, LDS), from a compilation of photometric.hip with
    -Rpass-analysis=kernel-resource-usage into a temporary directory (--no-resources skips it).

    python tools/photometric_robust_times.py [--reps 200] [--loop] [--out profiles/photometric_robust.txt]
"""
import argparse
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vitvs_amd  # noqa: E402,F401
from vitvs_amd import _lib, config, synth  # noqa: E402
from vitvs_amd.engine import Engine  # noqa: E402


def disturbed(rgb):
    out = np.clip(np.round(1.15 * rgb.astype(np.float64) + 8.0), 0, 255).astype(np.uint8)
    h, w = out.shape[:2]
    blk = np.kron(np.random.default_rng(5).integers(0, 256, (6, 8, 3)), np.ones((h // 24, w // 32, 1))).astype(np.uint8)
    out[h // 4:h // 4 + blk.shape[0], w // 4:w // 4 + blk.shape[1]] = blk          # a sixteenth of the frame
    return out


def median_us(call, stream, reps):
    with torch.cuda.stream(stream):
        for _ in range(20):
            assert call() == 0
        stream.synchronize()
        us = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            call()
            b.record(stream)
            b.synchronize()
            us.append(1000 * a.elapsed_time(b))
    return float(np.median(us))


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
        for n in (1, 8):
            cur = torch.from_numpy(np.ascontiguousarray(np.stack([disturbed(warped[:H, :W])] * n))).to(dev)
            des = torch.from_numpy(np.ascontiguousarray(np.stack([tex[:H, :W]] * n))).to(dev)
            Z = torch.from_numpy(np.stack([synth.depth_pattern(H, W)] * n)).to(dev)
            K = torch.tensor([[500.0, 500.0, W / 2.0, H / 2.0]] * n, dtype=torch.float64, device=dev)
            v = torch.zeros((n, 6), dtype=torch.float64, device=dev)
            st = torch.zeros(n, dtype=torch.int32, device=dev)
            normal = torch.zeros((n, 45), dtype=torch.float64, device=dev)
            robust = torch.zeros((n, 4), dtype=torch.float64, device=dev)
            info = torch.zeros((n, 8), dtype=torch.int32, device=dev)
            for level in (0, 2):
                plain = median_us(lambda: lib.vitvs_photometric_velocity_dev(h, n, p(cur), p(des), H, W, p(Z), 0.0, p(K), level, 1, 0.01,
                                                                             0.5, p(v), p(st), p(normal), p(info), sp), stream, args.reps)
                assert not st.cpu().numpy().any()
                for illum in (0, 1):
                    times = []
                    for N in range(5):
                        times.append(median_us(lambda: lib.vitvs_photometric_robust_velocity_dev(
                            h, n, p(cur), p(des), H, W, p(Z), 0.0, p(K), level, 1, 0.01, 0.5, illum, N, 1.0, p(v), p(st), p(robust), p(normal),
                            p(info), sp), stream, args.reps))
                        assert not st.cpu().numpy().any(), _lib.last_error(h)
                    i0, r0 = info.cpu().numpy()[0], robust.cpu().numpy()[0]
                    line = (f"{n} x {H} x {W}, level {level}: plain {plain:7.2f} us; robust, illumination {illum}, N = 0 .. 4: "
                            + " ".join(f"{t:7.2f}" for t in times) + f" us (x " + " ".join(f"{t / plain:.2f}" for t in times)
                            + f"); N = 4: {int(i0[6])} of {int(i0[0])} rows at weight 0, gamma {r0[0]:.4f} beta {r0[1]:.3f} sigma {r0[2]:.3f}")
                    print(line, flush=True)
                    lines.append(line)
    eng.close()


def loop_and_gaps(lines):
    import test_gpu_photometric_robust_loop as tl
    import test_gpu_photometric_robust_op as to
    import law_support as ls
    from vitvs_amd import weights
    track, handed, seen = tl.run_loop()
    last = seen[-1]
    lines.append(f"closed loop fp32 under gain+bias and block, robust hand-over (illumination, N = 4): pose error (cm / deg) at updates 0, "
                 f"10, .., {tl.UPDATES}: " + "  ".join(f"{p:.4f}/{r:.4f}" for p, r in track[::10]))
    lines.append(f"hand-over behind update {handed}, {sum(s['status'] != 0 for s in seen)} photometric updates not OK; the last update: gain "
                 f"{last['gain']:.4f}, bias {last['bias']:.3f}, sigma {last['sigma']:.3f}, rejected {last['rejected']:.4f}")
    cfg = ls.tiny_cfg(64)
    eng = Engine(cfg, config.ServoParams(dino_input_size=64, use_feature_binning=False), precision="fp32", max_pairs=4, max_rows=48)
    eng.load_state_dict(weights.synthetic_state_dict(cfg, 0))
    gap_dev, gap_self = np.zeros(4), np.zeros(4)
    runs = [(name, N, to.SMIN) for name in to.CASES for N in (1, 2, 3, 4)] + [(name, 4, 1.0) for name in to.FLOORED]
    for name, N, smin in runs:
        ref, rev = to._reference(name, 1, N, smin=smin), to._reference(name, 1, N, True, smin)
        v, info = to._device(eng, name, 1, N, smin)
        gap_dev = np.maximum(gap_dev, to._gaps(v, info, ref))
        rev_info = dict(gamma=[rev["robust"][0]], bias=[rev["robust"][1]], sigma=[rev["robust"][2]], weight=[rev["robust"][3]])
        gap_self = np.maximum(gap_self, to._gaps(rev["v"], rev_info, ref))
    eng.close()
    lines.append(f"gaps over the {len(runs)} runs of tests/test_gpu_photometric_robust_op.py (v relative L2, gamma, beta, sum w relative; the "
                 f"largest): the device against the fp64 reference " + " ".join(f"{g:.3e}" for g in gap_dev)
                 + "; the reference against itself summed in reversed row order " + " ".join(f"{g:.3e}" for g in gap_self))
    for line in lines[-3:]:
        print(line, flush=True)


def resources(lines):
    csrc = os.path.join(ROOT, "vit-vs_amd", "csrc")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-mllvm", "-amdgpu-kernarg-preload-count=16",
             "-mllvm", "-amdgpu-mfma-vgpr-form", "-Rpass-analysis=kernel-resource-usage"]
    with tempfile.TemporaryDirectory() as tmp:
        res = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *flags, "-c", os.path.join(csrc, "photometric.hip"), "-o",
                              os.path.join(tmp, "photometric.o")], capture_output=True, text=True)
    if res.returncode != 0:
        lines.append("compiler resource report: the compilation failed")
        return
    name, got = None, {}
    for ln in res.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
            got[name] = {}
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|VGPRs Spill|LDS Size \[bytes/block\]): (\d+)", ln)
        if m and name:
            got[name][m.group(1)] = int(m.group(2))
    for name, r in got.items():
        short = re.sub(r"^_ZN5vitvs\d+", "", name)
        short = re.split(r"(ENS_|ILb)", short)[0] + ("<true>" if "ILb1" in name else "<false>" if "ILb0" in name else "")
        line = (f"compiler resource report, {short}: {r.get('VGPRs')} VGPRs, {r.get('AGPRs')} AGPRs, scratch "
                f"{r.get('ScratchSize [bytes/lane]')} bytes/lane, {r.get('VGPRs Spill')} VGPRs spilled, occupancy "
                f"{r.get('Occupancy [waves/SIMD]')} waves/SIMD, static LDS {r.get('LDS Size [bytes/block]')} bytes")
        print(line, flush=True)
        lines.append(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--loop", action="store_true")
    ap.add_argument("--no-resources", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "photometric_robust.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    lines = [f"robust photometric law (vitvs_photometric_robust_velocity_dev: 3 N + 2 launches) against the plain law "
             f"(vitvs_photometric_velocity_dev: 2 launches), {torch.cuda.get_device_name(0)}; HIP event pairs around one call, median of "
             f"{args.reps}, microseconds; the current frame under gain+bias and a block, sigma_min 1"]
    print(lines[0])
    op_times(args, lines)
    if args.loop:
        loop_and_gaps(lines)
    if not args.no_resources:
        resources(lines)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
