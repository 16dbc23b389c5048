"""One representative shape per launch plan the forward can make: the table tests/test_gpu_plan_cover.py checks against fp64.

The forward (api.hip forward_chain) makes five linear launches and one attention launch per block, each decided by
plan_linear / plan_attention from its shape, the precision and the calling handle's in-flight hint.  This script walks the
product's shape domain (the constants below), reads every plan through the library's plan hooks (vitvs_op_linear_plan,
vitvs_op_attention_plan: host arithmetic, no device work), classifies each case by the instantiation it launches, and keeps
one representative per key:

  linear     (precision, epilogue, big family, rows, columns, k-groups, ring stages, K slices > 1, XCD map)
  attention  (precision, kernel, divided, key ranges, last range short)

The representative is the smallest problem (M.N.K; attention n.H.N^2) among the shapes whose last row tile is ragged
(M % rows != 0; all shapes when none is), then the one whose last tile holds the fewest rows, then the first in the walk
(hints ascending).  Store keys also record the GELU flags the forward reaches them with (qkv: off, fc1: on).

  python tools/plan_cover.py           print the table and its difference from tests/golden/plan_cover.json (exit 1 if any)
  python tools/plan_cover.py --write   write tests/golden/plan_cover.json
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vitvs_amd  # noqa: E402,F401
from vitvs_amd import _lib, config  # noqa: E402

TABLE = os.path.join(ROOT, "tests", "golden", "plan_cover.json")

# ---- the product's shape domain ----
MODELS = tuple(config._FAMILY)                # every model config knows
SIZES = (224, 308, 448, 518)                  # input sides; (size, stride) pairs that leave a remainder are not products
STRIDE_DIVISORS = (1, 2)                      # stride = patch, patch / 2
FRAMES = tuple(range(1, 17))                  # images per forward call
HINTS = (1, 2, 3, 4)                          # updates in flight (vitvs_set_option "in_flight")
PRECISIONS = (_lib.F32, _lib.BF16, _lib.F16, _lib.F16X2)
PREC_NAMES = {_lib.F32: "fp32", _lib.BF16: "bf16", _lib.F16: "fp16", _lib.F16X2: "f16x2"}
STORE, PARTIAL = 0, 1
# forward_chain's five linear layers: (name, epilogue, GELU)
LAYERS = (("embed", PARTIAL, 0), ("qkv", STORE, 0), ("proj", PARTIAL, 0), ("fc1", STORE, 1), ("fc2", PARTIAL, 0))
# vitvs_op_attention_plan kernel codes and the queries one workgroup covers
ATTN_KERNELS = {1: ("f32", 64), 2: ("short", 16), 3: ("q64", 64), 4: ("q64ks2", 64), 5: ("long", 128)}


def geometries():
    """(model, size, stride, cfg) for every valid combination of the domain."""
    for model in MODELS:
        patch = config._FAMILY[model][0]
        for size in SIZES:
            for d in STRIDE_DIVISORS:
                try:
                    cfg = config.vit_config(model, size, stride=patch // d)
                except ValueError:
                    continue
                yield model, size, patch // d, cfg


def layer_shapes(cfg, frames):
    """forward_chain's linear shapes (M, N, K) per layer for `frames` images."""
    D, T, N = cfg.dim, cfg.tokens, cfg.seq
    Kp = (cfg.patch_k + 63) // 64 * 64
    return {"embed": (frames * T, D, Kp), "qkv": (frames * N, 3 * D, D), "proj": (frames * N, D, D),
            "fc1": (frames * N, cfg.hidden, D), "fc2": (frames * N, D, cfg.hidden)}


def linear_plan(lib, prec, epi, M, N, K, slices=0):
    """(rc, [big, rows, cols, k-groups, stages, slices, xcd_map]) under the calling thread's hint."""
    out = (C.c_int32 * 7)()
    rc = lib.vitvs_op_linear_plan(prec, epi, M, N, K, slices, out)
    return rc, list(out)


def linear_key(prec, epi, plan):
    big, rows, cols, kg, stages, slices, xcd = plan
    return [prec, epi, big, rows, cols, kg, stages, int(slices > 1), xcd]


def attention_plan(lib, prec, n_img, N, H):
    out = (C.c_int32 * 6)()
    rc = lib.vitvs_op_attention_plan(prec, n_img, N, H, out)
    return rc, list(out)


def attention_key(prec, N, plan):
    kernel, per, divided = plan[0], plan[4], plan[5]
    nt = (N + 63) // 64
    ranges = -(-nt // per) if per else 1
    return [prec, kernel, divided, ranges, int(ranges > 1 and nt % per != 0)]


def key_id(key):
    """A readable test id for a key."""
    prec = PREC_NAMES[key[0]]
    if len(key) == 5:
        _, kernel, divided, ranges, short = key
        return f"{prec}-attn-{ATTN_KERNELS[kernel][0]}-{'divided' if divided else 'whole'}-r{ranges}" + ("-short" if short else "")
    _, epi, big, rows, cols, kg, stages, multi, xcd = key
    return (f"{prec}-{'partial' if epi == PARTIAL else 'store'}-{'big' if big else 'gemm'}{rows}x{cols}-kg{kg}-st{stages}"
            f"-{'slices' if multi else 'one'}" + ("-xcd" if xcd else ""))


def enumerate_table(lib):
    """The table: a list of rows sorted by key, one per reachable plan key."""
    best = {}      # key tuple -> (rank, row)
    gelus = {}     # store key tuple -> GELU flags seen
    cache = {}
    prev = lib.vitvs_op_plan_in_flight(1)
    try:
        order = 0
        for hint in HINTS:
            lib.vitvs_op_plan_in_flight(hint)
            for prec in PRECISIONS:
                for model, size, stride, cfg in geometries():
                    for frames in FRAMES:
                        shapes = layer_shapes(cfg, frames)
                        for layer, epi, gelu in LAYERS:
                            M, N, K = shapes[layer]
                            ck = (hint, prec, epi, M, N, K)
                            if ck not in cache:
                                cache[ck] = linear_plan(lib, prec, epi, M, N, K)
                            rc, plan = cache[ck]
                            if rc != 0:
                                raise RuntimeError(f"unlaunchable product shape {model} {size}/{stride} x{frames} {layer}: "
                                                   f"{PREC_NAMES[prec]} {M} x {N} x {K} (rc {rc})")
                            key = tuple(linear_key(prec, epi, plan))
                            if epi == STORE:
                                gelus.setdefault(key, set()).add(gelu)
                            rows = plan[1]
                            rank = (M % rows == 0, M * N * K, M % rows, order)
                            order += 1
                            if key not in best or rank < best[key][0]:
                                best[key] = (rank, {"kind": "linear", "hint": hint, "model": model, "size": size,
                                                    "stride": stride, "frames": frames, "layer": layer,
                                                    "M": M, "N": N, "K": K, "slices": plan[5]})
                        n_img, Ns, H = frames, cfg.seq, cfg.heads
                        ck = ("attn", hint, prec, n_img, Ns, H)
                        if ck not in cache:
                            cache[ck] = attention_plan(lib, prec, n_img, Ns, H)
                        rc, plan = cache[ck]
                        if rc != 0:
                            raise RuntimeError(f"no attention plan for {model} {size}/{stride} x{frames} (rc {rc})")
                        key = tuple(attention_key(prec, Ns, plan))
                        qrows = ATTN_KERNELS[plan[0]][1]
                        rank = (Ns % qrows == 0, n_img * H * Ns * Ns, Ns % qrows, order)
                        order += 1
                        if key not in best or rank < best[key][0]:
                            best[key] = (rank, {"kind": "attention", "hint": hint, "model": model, "size": size,
                                                "stride": stride, "frames": frames, "layer": "attention",
                                                "n_img": n_img, "N": Ns, "H": H})
    finally:
        lib.vitvs_op_plan_in_flight(prev)
    table = []
    for key in sorted(best, key=lambda k: (len(k) == 5, k)):
        row = {"id": key_id(key), "key": list(key)}
        row.update(best[key][1])
        if row["kind"] == "linear" and key[1] == STORE:
            row["gelu"] = sorted(gelus[key])
        table.append(row)
    return table


def load_table(path=TABLE):
    with open(path) as fh:
        return json.load(fh)["rows"]


def diff(old, new):
    """Lines describing how `new` differs from `old`, by key."""
    o = {r["id"]: r for r in old}
    n = {r["id"]: r for r in new}
    lines = [f"+ {i}  (new reachable plan)" for i in n if i not in o]
    lines += [f"- {i}  (no longer reachable)" for i in o if i not in n]
    lines += [f"~ {i}  representative {o[i]} -> {n[i]}" for i in n if i in o and o[i] != n[i]]
    return lines


def fmt(row):
    if row["kind"] == "linear":
        shape = f"{row['M']} x {row['N']} x {row['K']}" + (f"  slices {row['slices']}" if row["key"][1] == PARTIAL else
                                                           f"  gelu {row['gelu']}")
    else:
        shape = f"n {row['n_img']} N {row['N']} H {row['H']}"
    return (f"{row['id']:<44} hint {row['hint']}  {row['model']} {row['size']}/{row['stride']} x{row['frames']} "
            f"{row['layer']:<9} {shape}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--write", action="store_true", help=f"write {os.path.relpath(TABLE, ROOT)}")
    args = ap.parse_args()
    table = enumerate_table(_lib.load())
    n_lin = sum(r["kind"] == "linear" for r in table)
    if args.write:
        with open(TABLE, "w") as fh:   # one row per line, so that a change of the planner reads as a short diff
            fh.write('{"comment": "one representative shape per reachable launch plan; written by tools/plan_cover.py --write",\n'
                     ' "rows": [\n' + ",\n".join("  " + json.dumps(r) for r in table) + "\n ]}\n")
        print(f"wrote {len(table)} rows ({n_lin} linear, {len(table) - n_lin} attention) to {os.path.relpath(TABLE, ROOT)}")
        return 0
    for row in table:
        print(fmt(row))
    print(f"{len(table)} keys: {n_lin} linear, {len(table) - n_lin} attention")
    old = load_table() if os.path.isfile(TABLE) else []
    d = diff(old, table)
    print("\n".join(d) if d else f"no difference from {os.path.relpath(TABLE, ROOT)}")
    return 1 if d else 0


if __name__ == "__main__":
    sys.exit(main())
