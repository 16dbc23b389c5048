"""What selection mode BEST costs and what it does to a closed loop (select.hip best_order_kernel).

  kernel    best_order_kernel alone at T = 196, 484, 3136 x select_cells 1 and 4, from the library's own per-launch event pairs
            (vitvs_timing_*): a vitvs_servo_from_nn_dev call in BEST mode is two launches of the "servo" class, the same call in ORDER
            mode is the law alone; the kernel is the difference of the medians.  Tiny handles, 24 rows.
  update    the one-pair update of ViT-S/16 224, one in flight, captured and replayed on a side stream: BEST against ORDER.
  loop      Controller.ibvs() updates/s on camera-resolution host frames (bench.py's controller_loop) for "reference", "order", "best".
  --loops   the closed loops of tests/test_gpu_select_loop.py: "best" against "order" (torch seeds 121 .. 125) on the smooth
            texture, and on the fine texture of tests/test_gpu_robust_loop.py with and without robust_iterations=4.

On a tree without the mode (the parent commit) the BEST lines are left out, so ORDER and "reference" can be measured there too.

    python tools/select_times.py [--reps 200] [--rounds 3] [--loops] [--out profiles/best_selection.txt]
"""
import argparse
import dataclasses
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vitvs_amd  # noqa: E402,F401
from vitvs_amd import _lib, config, servo, synth, weights  # noqa: E402
from vitvs_amd.engine import Engine  # noqa: E402
from oracle import servo_ref as sr  # noqa: E402

BEST = getattr(_lib, "SELECT_BEST", None)


def say(lines, text):
    print(text, flush=True)
    lines.append(text)


def tiny_cfg(img):
    base = config.vit_config("dino_vits16", img)
    return dataclasses.replace(base, dim=128, depth=2, heads=2, layer=1, native_grid=base.grid)


def tables(rng, t):
    S = rng.uniform(0.2, 0.8, size=(t, t)).astype(np.float32)
    n = t // 3
    S[rng.permutation(t)[:n], rng.permutation(t)[:n]] = rng.uniform(0.85, 0.95, size=n).astype(np.float32)
    sim1, nn1, _, nn2 = sr.nearest_neighbours(torch.from_numpy(S))
    return nn1.numpy(), nn2.numpy(), sim1.numpy()


def kernel_times(lines, reps, rounds):
    for g in (14, 22, 56):
        t = g * g
        params = config.ServoParams(dino_input_size=16 * g)
        eng = Engine(tiny_cfg(16 * g), params, precision="fp32", max_pairs=1, max_rows=48)
        nn1, nn2, sim1 = tables(np.random.default_rng(g), t)
        order = np.random.default_rng(1).permutation(t).astype(np.int32)
        depth, K = synth.depth_pattern(), params.intrinsics()

        def servo_us(mode, sel):
            us = []
            for i in range(reps + 20):
                eng.servo_from_nn(nn1, nn2, sim1, depth, K, mode=mode, selection=sel, num_pairs=24)
                ms, launches = eng.timing_collect()["servo"]
                if i >= 20:
                    us.append(1000 * ms)
            return np.array(us), launches
        eng.timing_enable(True)
        for rnd in range(rounds):
            law, n_law = servo_us(_lib.SELECT_ORDER, order)
            say(lines, f"round {rnd} T = {t:4d}: the law alone (ORDER, 24 rows, {n_law} launch): median {np.median(law):7.2f} us, p10 "
                       f"{np.percentile(law, 10):7.2f}, p90 {np.percentile(law, 90):7.2f} over {len(law)} calls")
            if BEST is None:
                continue
            for cells in (1, 4):
                eng.set_option("select_cells", cells)
                both, n_both = servo_us(BEST, None)
                say(lines, f"round {rnd} T = {t:4d} select_cells = {cells}: best_order_kernel + the law (BEST, {n_both} launches): median "
                           f"{np.median(both):7.2f} us, p10 {np.percentile(both, 10):7.2f}, p90 {np.percentile(both, 90):7.2f}; "
                           f"best_order_kernel alone (difference of the medians): {np.median(both) - np.median(law):7.2f} us")
        eng.timing_enable(False)
        eng.close()


def update_rates(lines, reps, rounds, precision):
    cfg = config.baseline_config("vits16_224")
    params = config.ServoParams(dino_input_size=cfg.img_size, use_feature_binning=False)
    eng = Engine(cfg, params, precision=precision, max_pairs=1).load_state_dict(weights.synthetic_state_dict(cfg, 0))
    des, cur = synth.frame_pair(cfg.img_size, synth.ACCEPTED_FRAME_SEEDS["vits16_224"])
    dev = eng.device
    cur_d, des_d = eng._frames(cur), eng._frames(des)
    z_d = torch.as_tensor(synth.depth_pattern()[None]).to(dev).contiguous()
    k_d = torch.as_tensor(params.intrinsics(), dtype=torch.float64).reshape(1, 4).to(dev)
    sel_d = torch.from_numpy(np.random.default_rng(1).permutation(cfg.tokens).astype(np.int32)[None]).to(dev)
    out_v = torch.zeros((1, 6), dtype=torch.float64, device=dev)
    out_s = torch.zeros(1, dtype=torch.int32, device=dev)
    side = torch.cuda.Stream(dev)
    eng.set_option("graph_replay", 1)
    torch.cuda.synchronize()
    modes = [("ORDER", _lib.SELECT_ORDER, sel_d)] + ([("BEST", BEST, None)] if BEST is not None else [])
    for rnd in range(rounds):
        for name, mode, sel in modes:
            with torch.cuda.stream(side):
                for _ in range(30):
                    eng.compute_velocity_dev(cur_d, des_d, z_d, k_d, mode, sel, None, out_v=out_v, out_status=out_s, num_pairs=24)
                    side.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    eng.compute_velocity_dev(cur_d, des_d, z_d, k_d, mode, sel, None, out_v=out_v, out_status=out_s, num_pairs=24)
                    side.synchronize()
                dt = time.perf_counter() - t0
            say(lines, f"round {rnd} one-pair update, {precision}, one in flight, replayed, {name:5s}: {reps / dt:8.1f} updates/s "
                       f"({1e6 * dt / reps:7.1f} us per update), status {int(out_s[0])}")
    eng.close()


def controller_rates(lines, rounds, precision):
    from PIL import Image
    cfg = config.baseline_config("vits16_224")
    params = config.ServoParams(dino_input_size=cfg.img_size, use_feature_binning=False)
    eng = Engine(cfg, params, precision=precision, max_pairs=1).load_state_dict(weights.synthetic_state_dict(cfg, 0))
    des, cur = synth.frame_pair(cfg.img_size, synth.ACCEPTED_FRAME_SEEDS["vits16_224"])
    cam = lambda a: np.asarray(Image.fromarray(a).resize((params.u_max, params.v_max)), dtype=np.uint8)   # noqa: E731
    goal_cam, cur_cam, depth = cam(des), cam(cur), synth.depth_pattern()
    names = ["reference", "order"] + (["best"] if BEST is not None else [])
    for rnd in range(rounds):
        for name in names:
            ctl = servo.Controller(eng, goal_image=goal_cam, selection=name)
            ctl.generator = torch.Generator().manual_seed(121)
            lat = []
            for _ in range(230):
                ctl.image_callback_rgb(cur_cam)
                ctl.image_callback_depth(depth)
                t0 = time.perf_counter()
                ctl.ibvs()
                lat.append(time.perf_counter() - t0)
            lat = np.array(lat[30:]) * 1e3
            say(lines, f"round {rnd} Controller.ibvs(), {precision}, selection {name:9s}: {1e3 / lat.mean():8.1f} updates/s, median "
                       f"{np.median(lat):.4f} ms, p90 {np.percentile(lat, 90):.4f} ms over {len(lat)} updates; status {ctl.last_status}")
    eng.close()


def loops(lines):
    import test_gpu_select_loop as tl

    def line(what, track, statuses):
        say(lines, f"{what}: final {track[-1, 0]:6.3f} cm / {track[-1, 1]:6.3f} deg, mean of the last 60 {track[-60:, 0].mean():6.3f} cm / "
                   f"{track[-60:, 1].mean():6.3f} deg, highest {track[:, 0].max():6.2f} cm, statuses {sorted(set(statuses))}")
    for precision in ("fp32", "bf16"):
        line(f"smooth texture, 360 updates, {precision}, best            ", *tl.run_loop(precision, "best"))
        line(f"smooth texture, 360 updates, {precision}, best, 1 cell    ", *tl.run_loop(precision, "best", select_cells=1))
        for seed in (121, 122, 123, 124, 125):
            line(f"smooth texture, 360 updates, {precision}, order seed {seed}  ", *tl.run_loop(precision, "order", seed=seed))
    for robust in (0, 4):
        line(f"fine texture, 120 updates, fp32, robust_iterations={robust}, best          ",
             *tl.run_loop("fp32", "best", texture=512, robust_iterations=robust, updates=120))
        for seed in (121, 122, 123):
            line(f"fine texture, 120 updates, fp32, robust_iterations={robust}, order seed {seed}",
                 *tl.run_loop("fp32", "order", seed=seed, texture=512, robust_iterations=robust, updates=120))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--loops", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    say(lines, f"library: {os.path.relpath(_lib.LIB_PATH, ROOT)} ({'with' if BEST is not None else 'without'} selection mode BEST)")
    say(lines, f"device: {torch.cuda.get_device_name(0)}")
    kernel_times(lines, args.reps, args.rounds)
    update_rates(lines, args.reps * 2, args.rounds, args.precision)
    controller_rates(lines, args.rounds, args.precision)
    if args.loops and BEST is not None:
        loops(lines)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
