"""Device time of the control law's kernel (servo_kernel) with the robust law off and with 1, 4 and 16 re-weightings.

Tiny handles (the law alone, through vitvs_servo_from_nn_dev): 24 pairs in ORDER mode at T = 196 (L and the weights in LDS) and a
DENSE selection at T = 3136 (about a thousand pairs: L, the weights and the Jacobi copy in the global workspace, the residuals
in LDS).  Times are the library's own event pairs around the launch (vitvs_timing_*), mean over --reps launches after a
warm-up; one line per configuration and round.  --rounds repeats everything on the same handle, so the run-to-run spread of a line
shows in one output.

    python tools/robust_law_times.py [--reps 200] [--rounds 1]
"""
import argparse
import dataclasses
import itertools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import vitvs_amd  # noqa: E402,F401
from vitvs_amd import _lib, config, synth  # noqa: E402
from vitvs_amd.engine import Engine  # noqa: E402


def tables(rng, t, n_boost):
    """Arg-max tables of a random similarity matrix with n_boost planted mutual nearest neighbours."""
    S = rng.uniform(0.2, 0.8, size=(t, t)).astype(np.float32)
    S[rng.permutation(t)[:n_boost], rng.permutation(t)[:n_boost]] = rng.uniform(0.85, 0.95, size=n_boost).astype(np.float32)
    sim1, nn1 = torch.max(torch.from_numpy(S), dim=-1)
    nn2 = torch.max(torch.from_numpy(S), dim=-2).indices
    return nn1.numpy(), nn2.numpy(), sim1.numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=1)
    args = ap.parse_args()
    for g, mode, name in ((14, _lib.SELECT_ORDER, "24 pairs, T = 196"), (56, _lib.SELECT_DENSE, "DENSE, T = 3136")):
        t, img = g * g, 16 * g
        base = config.vit_config("dino_vits16", img)
        cfg = dataclasses.replace(base, dim=128, depth=2, heads=2, layer=1, native_grid=base.grid)
        params = config.ServoParams(dino_input_size=img)
        eng = Engine(cfg, params, precision="fp32", max_pairs=1, max_rows=t)
        rng = np.random.default_rng(g)
        nn1, nn2, sim1 = tables(rng, t, t // 3)
        order = rng.permutation(t).astype(np.int32) if mode == _lib.SELECT_ORDER else None
        depth, K = synth.depth_pattern(), params.intrinsics()
        for rnd, n in itertools.product(range(args.rounds), (0, 1, 4, 16)):
            eng.set_option("robust_law", n)
            call = lambda: eng.servo_from_nn(nn1, nn2, sim1, depth, K, mode=mode, selection=order, num_pairs=24)  # noqa: E731
            for _ in range(10):
                call()
            torch.cuda.synchronize()
            eng.timing_enable(True)
            for _ in range(args.reps):
                call()
            ms, launches = eng.timing_collect()["servo"]
            eng.timing_enable(False)
            info = eng.last_details(1)["info"][0]
            print(f"round {rnd} {name}: robust_law = {n:2d}: servo_kernel {1000 * ms / launches:8.2f} us (mean of {launches} "
                  f"launches), {int(info[1])} feature pairs, {int(info[7])} with weight 0, final solve {'LDL^T' if info[4] < 0 else 'Jacobi'}")
        eng.close()


if __name__ == "__main__":
    main()
