"""The surface photometric law (photometric.hip, vitvs_photometric_surface_velocity_dev) measured on the GPU against the
tile law and the robust law on the same box in the same run:

  * device time of one call at 224 x 224 and 640 x 480, levels 0 and 2, 1 and 8 pairs, with a depth image, the current frame under a
    gain ramp (0.9 .. 1.1 across the width): the robust call with illumination, the tile call and the surface call with 2 x 2, 4 x 4
    and 8 x 8 cells (3 N + 2 launches each), each with N = 0 and N = 4 re-weightings.  HIP event pairs on the stream around ONE call,
    median over --reps calls after a warm-up;
  * with --loop: the closed loops of tests/test_gpu_photometric_surface_loop.py and the per-case gaps of
    tests/test_gpu_photometric_surface_op.py by those tests' own code;
  * the compiler's resource report of the law's kernels (VGPRs, scratch, LDS), from a compilation of photometric.hip with
    -Rpass-analysis=kernel-resource-usage into a temporary directory (--no-resources skips it; --resources-only makes nothing else and
    needs no GPU; --append adds to the file, so that the measurement and the report can come from two machines).

    python tools/photometric_surface_times.py [--reps 200] [--loop] [--out profiles/photometric_surface.txt]
    python tools/photometric_surface_times.py --loop --no-resources, then --resources-only --append, is how the committed file was made
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
from vitvs_amd import _lib, config, synth  # noqa: E402
from vitvs_amd.engine import Engine  # noqa: E402
from photometric_robust_times import median_us, resources  # noqa: E402

GRIDS = ((2, 2), (4, 4), (8, 8))


def ramped(rgb):
    W = rgb.shape[1]
    g = 0.9 + 0.2 * np.arange(W, dtype=np.float64) / (W - 1)
    return np.clip(np.round(g[None, :, None] * rgb.astype(np.float64)), 0, 255).astype(np.uint8)


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
            cur = torch.from_numpy(np.ascontiguousarray(np.stack([ramped(warped[:H, :W])] * n))).to(dev)
            des = torch.from_numpy(np.ascontiguousarray(np.stack([tex[:H, :W]] * n))).to(dev)
            Z = torch.from_numpy(np.stack([synth.depth_pattern(H, W)] * n)).to(dev)
            K = torch.tensor([[500.0, 500.0, W / 2.0, H / 2.0]] * n, dtype=torch.float64, device=dev)
            v = torch.zeros((n, 6), dtype=torch.float64, device=dev)
            st = torch.zeros(n, dtype=torch.int32, device=dev)
            normal = torch.zeros((n, 64, 45), dtype=torch.float64, device=dev)
            sums = torch.zeros((n, 64, 120), dtype=torch.float64, device=dev)
            robust = torch.zeros((n, 4), dtype=torch.float64, device=dev)
            tiles = torch.zeros((n, 64, 4), dtype=torch.float64, device=dev)
            nodes = torch.zeros((n, 81, 4), dtype=torch.float64, device=dev)
            info = torch.zeros((n, 8), dtype=torch.int32, device=dev)
            for level in (0, 2):
                base = {}
                for N in (0, 4):
                    base[N] = median_us(lambda: lib.vitvs_photometric_robust_velocity_dev(
                        h, n, p(cur), p(des), H, W, p(Z), 0.0, p(K), level, 1, 0.01, 0.5, 1, N, 1.0, p(v), p(st), p(robust), p(normal),
                        p(info), sp), stream, args.reps)
                    assert not st.cpu().numpy().any(), _lib.last_error(h)
                for gy, gx in GRIDS:
                    t, s = {}, {}
                    for N in (0, 4):
                        t[N] = median_us(lambda: lib.vitvs_photometric_tile_velocity_dev(
                            h, n, p(cur), p(des), H, W, p(Z), 0.0, p(K), level, 1, 0.01, 0.5, gy, gx, N, 1.0, p(v), p(st), p(robust),
                            p(tiles), p(normal), p(info), sp), stream, args.reps)
                        assert not st.cpu().numpy().any(), _lib.last_error(h)
                    for N in (0, 4):
                        s[N] = median_us(lambda: lib.vitvs_photometric_surface_velocity_dev(
                            h, n, p(cur), p(des), H, W, p(Z), 0.0, p(K), level, 1, 0.01, 0.5, gy, gx, N, 1.0, p(v), p(st), p(robust),
                            p(nodes), p(sums), p(info), sp), stream, args.reps)
                        assert not st.cpu().numpy().any(), _lib.last_error(h)
                    i0, r0 = info.cpu().numpy()[0], robust.cpu().numpy()[0]
                    line = (f"{n} x {H} x {W}, level {level}: robust N = 0 / 4 {base[0]:7.2f} / {base[4]:7.2f} us; tiles {gy} x {gx} "
                            f"{t[0]:7.2f} / {t[4]:7.2f} us; surface {gy} x {gx} {s[0]:7.2f} / {s[4]:7.2f} us (x {s[0] / t[0]:.2f} / "
                            f"{s[4] / t[4]:.2f} of the tile call, x {s[0] / base[0]:.2f} / {s[4] / base[4]:.2f} of the robust call; per "
                            f"re-weighting {(s[4] - s[0]) / 4:6.2f} against {(t[4] - t[0]) / 4:6.2f} and {(base[4] - base[0]) / 4:6.2f} us); "
                            f"N = 4: live {int(r0[0])} dead {int(r0[1])}, {int(i0[6])} of {int(i0[0])} rows at weight 0, sigma {r0[2]:.3f}")
                    print(line, flush=True)
                    lines.append(line)
    eng.close()


def loop(lines):
    """The closed loops and the per-case gaps, by the GPU tests' own code."""
    import test_gpu_photometric_surface_loop as tl
    import test_gpu_photometric_surface_op as to
    import law_support as ls
    from vitvs_amd import weights
    start = len(lines)
    for name in ("ramp", "spot"):
        track, handed, seen, nodes, _ = tl.run_loop(getattr(tl.sc, name))
        last = seen[-1]
        lines.append(f"closed loop fp32 under \"{name}\", surface hand-over (4 x 4, N = 4): pose error (cm / deg) at updates 0, 10, .., "
                     f"{tl.UPDATES}: " + "  ".join(f"{p:.4f}/{r:.4f}" for p, r in track[::10]))
        lines.append(f"hand-over behind update {handed}, {sum(s['status'] != 0 for s in seen)} photometric updates not OK; the CPU reference's "
                     f"loop ends at {tl.REFERENCE_END[name][0]:.4f}/{tl.REFERENCE_END[name][1]:.4f}; the last update: sigma {last['sigma']:.3f}, "
                     f"rejected {last['rejected']:.4f}, dead unknowns {last['dead']}, gains of the live nodes {last['gain_min']:.4f} .. "
                     f"{last['gain_max']:.4f}; node_gain " + " ".join(f"{g:.4f}" for g in nodes[-1][0].reshape(-1)))
    cfg = ls.tiny_cfg(64)
    eng = Engine(cfg, config.ServoParams(dino_input_size=64, use_feature_binning=False), precision="fp32", max_pairs=4, max_rows=48)
    eng.load_state_dict(weights.synthetic_state_dict(cfg, 0))
    for name in to.CASES:
        gap_dev, gap_self = to.case_gaps(eng, name)
        lines.append(f"gaps of tests/test_gpu_photometric_surface_op.py, {name}, N = 1, 4 (v relative L2, gamma_a, beta_a, sum w relative): "
                     "the device against the fp64 reference " + " ".join(f"{g:.3e}" for g in gap_dev)
                     + "; the reference against itself in reversed order " + " ".join(f"{g:.3e}" for g in gap_self))
    eng.close()
    for line in lines[start:]:
        print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--loop", action="store_true")
    ap.add_argument("--no-resources", action="store_true")
    ap.add_argument("--resources-only", action="store_true")
    ap.add_argument("--append", action="store_true", help="add to --out instead of writing it anew")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "photometric_surface.txt"))
    args = ap.parse_args()
    lines = []
    if not args.resources_only:
        assert torch.cuda.is_available(), "a measurement needs the GPU"
        lines.append(f"surface photometric law (vitvs_photometric_surface_velocity_dev: 3 N + 2 launches) against the tile law "
                     f"(vitvs_photometric_tile_velocity_dev) and the robust law with illumination (vitvs_photometric_robust_velocity_dev), "
                     f"{torch.cuda.get_device_name(0)}; HIP event pairs around one call, median of {args.reps}, microseconds; the current "
                     f"frame under a gain ramp, sigma_min 1")
        print(lines[0])
        op_times(args, lines)
        if args.loop:
            loop(lines)
    if not args.no_resources:
        report = []
        resources(report)
        lines += [ln for ln in report if "photometric_surface" in ln or "photometric_tile" in ln or "failed" in ln]
    if args.out:
        with open(args.out, "a" if args.append else "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
