"""Device time of the control law's kernel (servo_kernel) with the sub-patch refinement of matches off and on.

The refinement reads what the forward left in the handle, so the law is timed inside whole updates (compute_velocity) on real
handles with synthetic weights: ViT-S/16 224² (196 tokens) and ViT-B/8 448² (3136 tokens), plain and binned descriptors, 24 pairs
in ORDER mode and a DENSE selection, bf16.  Times are the library's own event pairs around the law's launch (vitvs_timing_*),
one collect per update: median (and mean) over --reps updates after a warm-up; one line per configuration.

    python tools/subpatch_times.py [--reps 100] [--configs vits16_224,vitb8_448]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import vitvs_amd  # noqa: E402,F401
from vitvs_amd import _lib, config, synth, weights  # noqa: E402
from vitvs_amd.engine import Engine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--configs", default="vits16_224,vitb8_448")
    ap.add_argument("--precision", default="bf16")
    args = ap.parse_args()
    for key in args.configs.split(","):
        cfg = config.baseline_config(key)
        sd = weights.synthetic_state_dict(cfg, 0)
        des, cur = synth.frame_pair(cfg.img_size, 20250705)
        depth = synth.depth_pattern()
        for binned in (False, True):
            params = config.ServoParams(dino_input_size=cfg.img_size, use_feature_binning=binned)
            eng = Engine(cfg, params, precision=args.precision, max_pairs=1, max_rows=cfg.tokens).load_state_dict(sd)
            order = np.random.default_rng(3).permutation(cfg.tokens).astype(np.int32)
            for mode, name in ((_lib.SELECT_ORDER, "24 pairs"), (_lib.SELECT_DENSE, "DENSE")):
                for on in (0, 1):
                    eng.set_option("subpatch", on)
                    call = lambda: eng.compute_velocity(cur, des, depth, params.intrinsics(), mode=mode,  # noqa: E731
                                                        selection=order if mode == _lib.SELECT_ORDER else None, num_pairs=24)
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
                    print(f"{key} {args.precision} {'binned' if binned else 'plain '} {name:8s} subpatch = {on}: servo_kernel median "
                          f"{np.median(us):8.2f} us, mean {np.mean(us):8.2f} us over {len(us)} updates, {int(info[1])} feature pairs",
                          flush=True)
            eng.close()


if __name__ == "__main__":
    main()
