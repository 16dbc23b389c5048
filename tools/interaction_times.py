"""Device time of the control law's kernel (servo_kernel) with each interaction matrix (option "interaction": 0 current, 1 desired,
2 mean).

The law alone on tiny weight-less handles through vitvs_servo_from_nn_dev, like tools/robust_law_times.py: 24 pairs of a 14 x 14
grid in ORDER mode (L in LDS) and a DENSE selection over 56 x 56 = 3136 tokens (L in the global workspace).  Times are the
library's own event pairs around the law's launch (vitvs_timing_*), one collect per call: median (and mean, and the 10th / 90th
percentile) over --reps calls after a warm-up; one line per configuration.  --rounds repeats everything, so the run-to-run spread
of one line shows in one output.  VITVS_LIB=<another build> times that build (a parent commit's library knows mode 0 only:
--modes 0).

    python tools/interaction_times.py [--reps 200] [--rounds 3] [--modes 0,1,2]
"""
import argparse
import dataclasses
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import vitvs_amd  # noqa: E402,F401
from vitvs_amd import _lib, config, synth  # noqa: E402
from vitvs_amd.engine import Engine  # noqa: E402


def tables(rng, t, n_mutual):
    """nn_1 a random permutation, nn_2 its inverse on n_mutual tokens and wrong elsewhere."""
    nn1 = rng.permutation(t).astype(np.int32)
    nn2 = np.empty(t, np.int32)
    nn2[nn1] = np.arange(t, dtype=np.int32)
    bad = rng.permutation(t)[: t - n_mutual]
    nn2[nn1[bad]] = (bad + 1) % t
    return nn1, nn2, rng.uniform(0.3, 0.9, size=t).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--modes", default="0,1,2")
    args = ap.parse_args()
    modes = [int(m) for m in args.modes.split(",")]
    print(f"library: {_lib.LIB_PATH}")
    for rnd in range(args.rounds):
        for g, select, name, n_mutual in ((14, _lib.SELECT_ORDER, "24 pairs", 120), (56, _lib.SELECT_DENSE, "DENSE", 1700)):
            t, img = g * g, 16 * g
            base = config.vit_config("dino_vits16", img)
            cfg = dataclasses.replace(base, dim=128, depth=2, heads=2, layer=1, native_grid=base.grid)
            params = config.ServoParams(dino_input_size=img)
            eng = Engine(cfg, params, precision="fp32", max_pairs=1, max_rows=max(t, 48))
            rng = np.random.default_rng(3)
            nn1, nn2, sim1 = tables(rng, t, n_mutual)
            depth = synth.depth_pattern()
            order = rng.permutation(t).astype(np.int32)
            if any(modes):
                eng.set_goal_depth(np.ascontiguousarray(depth[::-1, ::-1]))
            for mode in modes:
                if mode or any(modes):
                    eng.set_option("interaction", mode)
                call = lambda: eng.servo_from_nn(nn1, nn2, sim1, depth, params.intrinsics(), mode=select,  # noqa: E731
                                                 selection=order if select == _lib.SELECT_ORDER else None, num_pairs=24)
                for _ in range(10):
                    call()
                torch.cuda.synchronize()
                eng.timing_enable(True)
                us = []
                for _ in range(args.reps):
                    call()
                    ms, launches = eng.timing_collect()["servo"]
                    assert launches == 1
                    us.append(1000 * ms)
                eng.timing_enable(False)
                info = eng.last_details(1)["info"][0]
                print(f"round {rnd} T = {t:4d} {name:8s} interaction = {mode}: servo_kernel median {np.median(us):8.2f} us, mean "
                      f"{np.mean(us):8.2f} us, p10 {np.percentile(us, 10):8.2f}, p90 {np.percentile(us, 90):8.2f} over {len(us)} calls, "
                      f"{int(info[1])} feature pairs", flush=True)
            eng.close()


if __name__ == "__main__":
    main()
