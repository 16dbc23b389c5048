"""tests/history_cases.py is a fair test (no GPU): unique names, every dirtying call exceeds its probe in the extent its axis
names (for "<axis>-reverse" rows the probe exceeds the dirtier, and the forward row of that axis exists), the two never share
their inputs, and every axis, refusal and pool call the GPU module runs is in the table."""
import history_cases as hc

AXES = ["pairs", "in_flight", "geometry", "entry", "graph", "rows", "solver", "status", "options", "follow", "first_use", "select",
        "consensus", "roll"]


def test_names_are_unique():
    names = [r[0] for r in hc.ROWS]
    assert len(names) == len(set(names))
    pool = [n for n, _ in hc.POOL]
    assert len(pool) == len(set(pool)) and len(pool) >= 12
    assert len(set(hc.REFUSALS)) == len(hc.REFUSALS) == 5
    assert len({n for n, _, _ in hc.ENTRY_ROWS}) == len(hc.ENTRY_ROWS) == 9


def test_every_dirtier_exceeds_its_probe_in_its_axis():
    seen = set()
    for name, d, p, axis in hc.ROWS:
        base, _, reverse = axis.partition("-")
        assert base in AXES and reverse in ("", "reverse"), name
        big, small = (p, d) if reverse else (d, p)
        assert hc.extent(big, base) > hc.extent(small, base), (name, hc.extent(d, base), hc.extent(p, base))
        seen.add(axis)
    for axis in AXES:
        assert axis in seen, axis
    for axis in seen:
        assert axis.partition("-")[0] in seen, axis                  # no reverse row without its forward row


def test_rows_beyond_the_lds_edge_are_the_other_side():
    sides = {name: (hc.extent(d, "rows")[0], hc.extent(p, "rows")[0]) for name, d, p, axis in hc.ROWS if axis.startswith("rows")}
    assert sides and all(a != b for a, b in sides.values()), sides
    assert {a for a, _ in sides.values()} == {True, False}          # L global first and L in LDS first


def test_dirtier_and_probe_never_share_their_inputs():
    for name, d, p, _ in hc.ROWS:
        assert hc.inputs(d) and hc.inputs(p) and not (hc.inputs(d) & hc.inputs(p)), name


def test_the_table_covers_what_the_issue_lists():
    picks = {c["pick"] if c["depth"] else "no_depth" for _, d, p, a in hc.ROWS if a.startswith("status") for c in hc._leaves(d) + hc._leaves(p)}
    assert picks >= {"few", "no_mutual", "all_mutual", "no_depth", "same_image", "mutual"}
    solver = {c["pick"] for _, d, p, a in hc.ROWS if a.startswith("solver") for c in hc._leaves(d) + hc._leaves(p)}
    assert solver == {"mutual", "repeat1", "repeat2"}
    laws = {c["law"] for _, d, p, a in hc.ROWS if a.startswith("follow") for c in hc._leaves(d) if c["kind"] == "follow"}
    assert laws == set(hc.FOLLOW_LAWS)
    for law in hc.FOLLOW_LAWS:
        kinds = ("big_then_small", "small_then_big", "first_use_after_20_updates")
        assert all(any(n == f"follow_{law}_{k}" for n, *_ in hc.ROWS) for k in kinds), law
    singles = {d["options"] for _, d, _, a in hc.ROWS if a == "options"}
    assert singles == {hc.ALL_ON, (4, 0, 0), (0, 1, 0), (0, 0, 2)}
    kinds = {c["kind"] for _, c in hc.POOL}
    assert kinds == {"velocity", "forward", "law", "follow", "roll"}
    noise = [n for n, d, _, _ in hc.ROWS if any(c.get("frames") == "noise" for c in hc._leaves(d))]
    assert noise                                                   # a dirtier far from every probe's values


def _rows(axis):
    return {name: (d, p) for name, d, p, a in hc.ROWS if a.partition("-")[0] == axis}


def test_the_best_rows_are_what_they_say():
    rows = _rows("select")
    assert len(rows) == 7
    d, p = rows["best_four_noise_pairs_then_order"]
    assert hc.extent(d, "select")[:2] == (1, 4 * hc.TOKENS) and d["frames"] == "noise" and d["num_pairs"] == 48
    assert hc.extent(p, "select") == (0, 0, 0, 0) and p["mode"] == "order"
    d, p = rows["order_then_best_four_pairs"]
    assert d["mode"] == "order" and p["mode"] == "best" and len(p["seeds"]) == 4
    cells = {name: (d["select_cells"], p["select_cells"]) for name, (d, p) in rows.items() if "cell" in name}
    assert sorted(cells.values()) == [(1, 4), (4, 1)]
    assert all(d["mode"] == p["mode"] == "best" for name, (d, p) in rows.items() if name in cells)
    d, p = rows["best_long_order_then_short"]
    t = d["grid"] ** 2
    assert hc.extent(d, "select")[2] == (2 * t) // 3 and hc.extent(p, "select")[2] == 12 < p["num_pairs"] == 24
    d, p = rows["best_short_order_then_long"]
    assert hc.extent(d, "select")[2] == 12 and hc.extent(p, "select")[2] == (2 * t) // 3
    d, p = rows["best_no_correspondence_then_normal"]
    assert d["pick"] == "no_mutual" and d["mode"] == p["mode"] == "best" and p["pick"] == "mutual"
    best_graph = [p for name, d, p, a in hc.ROWS if a == "graph" and p["mode"] == "best"]
    assert len(best_graph) == 1
    host_best = [d for name, d, _ in hc.ENTRY_ROWS if d.get("mode") == "best"]
    assert len(host_best) == 1 and host_best[0]["entry"] == "host" and host_best[0]["goal"] == "own"
    assert hc.SELECT["best"] == 3


def test_the_consensus_rows_are_what_they_say():
    rows = _rows("consensus")
    assert len(rows) == 4 * len(hc.CONSENSUS_LAWS)
    for law in hc.CONSENSUS_LAWS:
        d, p = rows[f"consensus_{law}_4096_then_none"]
        assert (d["law"], d["n_iter"], d["consensus"], d["seed"], d["camera"]) == (law, 4, 4096, 7, hc.CAM_BIG)
        assert (p["law"], p["n_iter"], p["consensus"], p["camera"]) == (law, 0, 0, hc.CAM_SMALL)
        d, p = rows[f"consensus_{law}_none_then_4096"]
        assert d["consensus"] == 0 and p["consensus"] == 4096
        d, p = rows[f"consensus_{law}_4096_then_256"]
        assert (d["consensus"], p["consensus"]) == (4096, 256)
        assert hc.extent(d, "consensus")[1:4] == hc.extent(p, "consensus")[1:4]         # a camera call of the same shape
        d, p = rows[f"consensus_{law}_seed_7_then_0"]
        assert (d["consensus"], d["seed"], p["consensus"], p["seed"]) == (256, 7, 256, 0)
        first = [p for name, d, p, a in hc.ROWS if name == f"consensus_{law}_first_use_after_20_updates" and a == "first_use"]
        assert len(first) == 1 and first[0]["consensus"] > 0 and first[0]["law"] == law
    old = [c for name, d, p, a in hc.ROWS if a.startswith("follow") for c in (d, p)]
    assert old and not any(c["consensus"] for c in old)                                  # the rows of axis 10 run as they did


def test_the_roll_rows_are_what_they_say():
    rows = _rows("roll")
    assert len(rows) == 9
    probes = {hc.P1["seeds"], hc.P4["seeds"]}
    assert {p["seeds"] for d, p in rows.values() if p["kind"] == "velocity"} == probes and hc.P4["goal"] == "own"
    for name in ("roll_then_one_pair", "roll_then_four_pairs_four_goals"):
        assert hc.extent(rows[name][0], "roll") == (1, 1)
    for name, dirt, entry in (("four_pairs_then_roll", hc.D4, "dev"), ("four_pairs_one_goal_then_roll_host", hc.D4_SHARED, "host")):
        assert rows[name][0] == dirt and hc.extent(rows[name][1], "roll") == (1, 1) and rows[name][1]["entry"] == entry
    d, p = rows["roll_winner_3_then_winner_0"]
    assert d["turn"] == 1 and d["winner"] == "nonzero" and p["turn"] == 0 and p["winner"] == "zero" and not p["at_goal"]
    d, p = rows["roll_winner_3_then_at_the_goal"]
    assert d["winner"] == "nonzero" and p["turn"] == 0 and p["winner"] == "zero" and p["at_goal"]
    for name in ("roll_then_pose_consensus", "pose_consensus_then_roll"):
        law = [c for side in rows[name] for c in hc._leaves(side) if c["kind"] == "follow"]
        assert law and all((c["law"], c["n_iter"], c["consensus"], len(c["camera"]["seeds"])) == ("pose", 4, 256, 1) for c in law)
    assert rows["four_pairs_then_roll_best"][1]["mode"] == "best"
    eager = [d for name, d, p, a in hc.ROWS if a == "graph" and d["kind"] == "roll"]
    assert len(eager) == 1 and eager[0]["winner"] == "nonzero"
    rolls = [c for _, d, p, _ in hc.ROWS for side in (d, p) for c in hc._leaves(side) if c["kind"] == "roll"]
    assert all(c["turn"] in (0, 1, 2, 3) and (c["winner"] == "zero") == (c["turn"] == 0) or c["winner"] == "any" for c in rolls)
    assert all(c["seed"] in hc.DIRT_SEEDS + hc.PROBE_SEEDS for c in rolls)
    entry = {name: (d, survives) for name, d, survives in hc.ENTRY_ROWS if d["kind"] == "roll"}
    assert {d["goal"]: survives for d, survives in entry.values()} == {"own": False, "cached_keep": True}
    pool = [c for _, c in hc.POOL]
    assert sum(c["kind"] == "roll" and c["winner"] == "nonzero" for c in pool) == 1
    assert sum(c.get("mode") == "best" for c in pool) == 1
    assert sum(c["kind"] == "follow" and c["law"] == "pose" and c["consensus"] > 0 for c in pool) == 1
