"""CPU-side checks of tests/golden/plan_cover.json, the table of one representative shape per launch plan the forward can make
(tools/plan_cover.py; tests/test_gpu_plan_cover.py runs every row against fp64).  The plans are host arithmetic in the library
(vitvs_op_linear_plan, vitvs_op_attention_plan): no device calls here."""
import ctypes
import os

import pytest

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib, config
from op_support import host_lib as lib  # noqa: F401
from op_support import plan_cover as cover  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REGEN = "run `python tools/plan_cover.py --write`"


@pytest.fixture(scope="module")
def table(cover):
    return cover.load_table()


def test_fresh_enumeration_is_the_committed_table(lib, cover, table):
    """A plan the planner gains or loses, or a representative that moves, fails here by name."""
    fresh = cover.enumerate_table(lib)
    old = {r["id"]: r for r in table}
    new = {r["id"]: r for r in fresh}
    for i in new:
        assert i in old, f"plan {i} {new[i]['key']} is reachable but not in tests/golden/plan_cover.json: {REGEN}"
    for i in old:
        assert i in new, f"plan {i} {old[i]['key']} is no longer reachable: {REGEN}"
    for i in new:
        assert new[i] == old[i], f"representative of plan {i} changed: {old[i]} -> {new[i]}: {REGEN}"
    assert [r["id"] for r in fresh] == [r["id"] for r in table], REGEN


def test_every_row_plans_its_key_under_its_hint(lib, cover, table):
    assert table
    prev = lib.vitvs_op_plan_in_flight(1)
    try:
        for row in table:
            lib.vitvs_op_plan_in_flight(row["hint"])
            prec = row["key"][0]
            if row["kind"] == "linear":
                epi = row["key"][1]
                rc, plan = cover.linear_plan(lib, prec, epi, row["M"], row["N"], row["K"])
                assert rc == 0, (row["id"], rc)
                assert cover.linear_key(prec, epi, plan) == row["key"], (row["id"], plan)
                assert plan[5] == row["slices"], row["id"]
                # the partial-sum hook at the row's explicit slice count launches the same plan
                if epi == cover.PARTIAL:
                    assert cover.linear_plan(lib, prec, epi, row["M"], row["N"], row["K"], row["slices"]) == (rc, plan)
                    assert lib.vitvs_op_splitk_slices(prec, row["M"], row["N"], row["K"]) == row["slices"]
                else:
                    assert row["slices"] == 1 and row["gelu"] and set(row["gelu"]) <= {0, 1}
                    t = (ctypes.c_int32 * 3)()     # the older tile hook agrees
                    assert lib.vitvs_op_linear_tile(prec, row["M"], row["N"], row["K"], 0, t) == 0
                    assert list(t) == [plan[1], plan[2], plan[3]], row["id"]
            else:
                rc, plan = cover.attention_plan(lib, prec, row["n_img"], row["N"], row["H"])
                assert rc == 0, (row["id"], rc)
                assert cover.attention_key(prec, row["N"], plan) == row["key"], (row["id"], plan)
            assert cover.key_id(row["key"]) == row["id"]
    finally:
        lib.vitvs_op_plan_in_flight(prev)


def test_rows_are_product_shapes(table):
    """Every row is the shape forward_chain launches for the model, input, stride and frame count it names."""
    layers = {"embed", "qkv", "proj", "fc1", "fc2", "attention"}
    for row in table:
        cfg = config.vit_config(row["model"], row["size"], stride=row["stride"])
        assert 1 <= row["frames"] <= 16 and row["layer"] in layers and 1 <= row["hint"] <= 4, row["id"]
        if row["kind"] == "attention":
            assert (row["n_img"], row["N"], row["H"]) == (row["frames"], cfg.seq, cfg.heads), row["id"]
            continue
        Kp = (3 * cfg.patch ** 2 + 63) // 64 * 64
        want = {"embed": (row["frames"] * cfg.tokens, cfg.dim, Kp),
                "qkv": (row["frames"] * cfg.seq, 3 * cfg.dim, cfg.dim),
                "proj": (row["frames"] * cfg.seq, cfg.dim, cfg.dim),
                "fc1": (row["frames"] * cfg.seq, cfg.hidden, cfg.dim),
                "fc2": (row["frames"] * cfg.seq, cfg.dim, cfg.hidden)}[row["layer"]]
        assert (row["M"], row["N"], row["K"]) == want, row["id"]
        if row["layer"] == "embed":
            assert row["K"] == Kp and row["K"] % 64 == 0, row["id"]
        assert row["key"][1] == (0 if row["layer"] in ("qkv", "fc1") else 1), row["id"]


def test_linear_plan_hook_refuses_what_it_cannot_plan(lib):
    out = (ctypes.c_int32 * 7)()
    assert lib.vitvs_op_linear_plan(_lib.BF16, 2, 197, 384, 384, 0, out) == -1       # the residual epilogue is not a forward layer
    assert lib.vitvs_op_linear_plan(_lib.BF16, 1, 197, 384, 384, -1, out) == -1
    assert lib.vitvs_op_linear_plan(_lib.BF16, 0, 197, 384, 100, 0, out) == -2       # K not a multiple of the k-tile
    assert out[1] == 0
    assert lib.vitvs_op_linear_plan(_lib.BF16, 1, 394, 768, 3072, 5, out) == -2     # 3072 is not a multiple of 5 k-tiles
    assert lib.vitvs_op_linear_plan(_lib.BF16, 1, 394, 768, 3072, 3, out) == 0 and out[5] == 3
