"""Device time of the roll search (roll.hip, vitvs_roll_velocity_dev): its two launches at T = 196, 484 and 3136 tokens, and
the one-pair update with and without the search.

  quarter turns   vitvs_op_quarter_turns on one random frame at S = 224, 308 and 448 (the frame sizes of those token counts): HIP
                  event pairs on the stream around ONE call, median / p10 / p90 over --reps calls after a warm-up, and around
                  --burst calls back to back divided by their number (the event pair's own cost amortised)
  roll pick       the kernel's own begin / end stamps through the handle's timing classes (class "servo"): a roll call in DENSE
                  mode stamps the pick and the law, a servo_from_nn call on the carried-back tables stamps the same law alone;
                  the pick is the difference of the two class totals, per call, over --reps calls
  update          ViT-B/16 224² bf16, one update in flight: host clock around call + stream synchronise, median / p10 / p90 over
                  --reps updates after a warm-up, for compute_velocity_dev (one pair) and vitvs_roll_velocity_dev, each with the
                  goal forwarded by the call and with the goal cached (set_goal)

--rounds repeats everything, so the run-to-run spread of a line shows in one output.

    python tools/roll_times.py [--reps 200] [--rounds 3] [--burst 50] [--out profiles/roll_search.txt]
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
import vitvs_amd  # noqa: E402,F401
from vitvs_amd import _lib, config, synth, weights  # noqa: E402
from vitvs_amd.engine import Engine  # noqa: E402

KEYS = {196: "vitb16_224", 484: "vits14_308", 3136: "vitb8_448"}


def stats(us):
    return f"median {np.median(us):8.2f} us, p10 {np.percentile(us, 10):8.2f}, p90 {np.percentile(us, 90):8.2f} over {len(us)}"


def quarter_turn_times(lib, dev, stream, S, reps, burst):
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    f = torch.randint(0, 256, (1, S, S, 3), dtype=torch.uint8, device=dev)
    out = torch.empty((1, 4, S, S, 3), dtype=torch.uint8, device=dev)
    call = lambda: lib.vitvs_op_quarter_turns(p(f), 1, S, p(out), C.c_void_p(stream.cuda_stream))  # noqa: E731
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
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(burst):
            call()
        b.record(stream)
        b.synchronize()
    assert np.array_equal(out[0, 1].cpu().numpy(), np.rot90(f[0].cpu().numpy(), 1))
    return us, 1000 * a.elapsed_time(b) / burst


def make_engine(key, precision, max_pairs):
    cfg = config.baseline_config(key)
    params = config.ServoParams(dino_input_size=cfg.img_size, use_feature_binning=False)
    eng = Engine(cfg, params, precision=precision, max_pairs=max_pairs, max_rows=cfg.tokens)
    return cfg, params, eng.load_state_dict(weights.synthetic_state_dict(cfg, 0))


def pick_times(T, reps):
    """(pick us per call, law us per call, k*) from the handle's "servo" timing class."""
    cfg, params, eng = make_engine(KEYS[T], "bf16", 4)
    des, cur = synth.frame_pair(cfg.img_size, synth.ACCEPTED_FRAME_SEEDS[KEYS[T]])
    cur = np.ascontiguousarray(np.rot90(cur, 1))
    z, K = synth.depth_pattern(), params.intrinsics()
    for _ in range(3):
        _, _, info = eng.roll_velocity(cur, des, z, K, mode=_lib.SELECT_DENSE)
    tab = eng.last_tables(1)
    eng.timing_enable(True)
    both_ms = law_ms = 0.0
    both_n = law_n = 0
    for _ in range(reps):                                        # (collected per call: the handle's event pool stays one call's)
        eng.roll_velocity(cur, des, z, K, mode=_lib.SELECT_DENSE)
        ms, n = eng.timing_collect()["servo"]
        both_ms, both_n = both_ms + ms, both_n + n
        eng.servo_from_nn(tab["nn_1"][0], tab["nn_2"][0], tab["sim_1"][0], z, K, mode=_lib.SELECT_DENSE)
        ms, n = eng.timing_collect()["servo"]
        law_ms, law_n = law_ms + ms, law_n + n
    eng.timing_enable(False)
    eng.close()
    assert both_n == 2 * reps and law_n == reps, (both_n, law_n)
    return 1000 * (both_ms - law_ms) / reps, 1000 * law_ms / reps, info["roll"]


def update_times(reps):
    """{(search, cached): per-update microseconds} for ViT-B/16 224² bf16, one in flight."""
    cfg, params, eng = make_engine("vitb16_224", "bf16", 4)
    _, _, plain = make_engine("vitb16_224", "bf16", 1)
    dev = eng.device
    des, cur = synth.frame_pair(cfg.img_size, synth.ACCEPTED_FRAME_SEEDS["vitb16_224"])
    cur = np.ascontiguousarray(np.rot90(cur, 1))
    Ic, Id = torch.from_numpy(cur[None]).to(dev), torch.from_numpy(des[None]).to(dev)
    Z = torch.from_numpy(synth.depth_pattern()[None]).to(dev)
    K = torch.tensor([params.intrinsics()], dtype=torch.float64, device=dev)
    v = torch.zeros((1, 6), dtype=torch.float64, device=dev)
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    rinfo = torch.zeros(8, dtype=torch.int32, device=dev)
    scores = torch.zeros(4, dtype=torch.float64, device=dev)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    stream = torch.cuda.current_stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    lib = eng.lib
    out = {}
    for search in (False, True):
        for cached in (False, True):
            e = eng if search else plain
            if cached:
                e.set_goal(Id)
            d = None if cached else Id
            if search:
                call = lambda: lib.vitvs_roll_velocity_dev(e.handle, p(Ic), p(d), p(Z), p(K), _lib.SELECT_BEST, None, None, 24, p(v),  # noqa: E731
                                                           p(st), p(rinfo), p(scores), sp)
            else:
                call = lambda: lib.vitvs_compute_velocity_dev(e.handle, 1, p(Ic), p(d), 0, p(Z), p(K), _lib.SELECT_BEST, None, None,  # noqa: E731
                                                              24, p(v), p(st), sp)
            for _ in range(20):
                assert call() == 0
            stream.synchronize()
            us = []
            for _ in range(reps):
                t0 = time.perf_counter()
                call()
                stream.synchronize()
                us.append(1e6 * (time.perf_counter() - t0))
            assert int(st.cpu()[0]) in (0, 2)
            out[(search, cached)] = us
    eng.close()
    plain.close()
    return out, int(rinfo.cpu()[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--burst", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roll_search.txt"))
    args = ap.parse_args()
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    lines = [f"roll search (roll.hip, vitvs_roll_velocity_dev), {torch.cuda.get_device_name(dev)}; microseconds"]
    print(lines[0])

    def say(line):
        print(line, flush=True)
        lines.append(line)
    for rnd in range(args.rounds):
        for T, S in ((196, 224), (484, 308), (3136, 448)):
            us, burst = quarter_turn_times(lib, dev, stream, S, args.reps, args.burst)
            say(f"round {rnd} quarter turns, one frame {S} x {S} (T = {T}): {stats(us)} calls; {burst:7.2f} us per call in a burst of {args.burst}")
        for T in (196, 484, 3136):
            pick, law, k = pick_times(T, args.reps)
            say(f"round {rnd} roll pick, T = {T:4d} (kernel stamps, bf16, DENSE): pick {pick:7.2f} us per call, the one-pair law behind it "
                f"{law:7.2f} us; k* = {k}")
        upd, k = update_times(args.reps)
        for (search, cached), us in upd.items():
            say(f"round {rnd} update ViT-B/16 224 bf16, one in flight, selection BEST, roll search {'on ' if search else 'off'}, goal "
                f"{'cached   ' if cached else 'forwarded'}: {stats(us)} updates = {1e6 / np.median(us):7.1f} updates/s" +
                (f"; k* = {k}" if search else ""))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
