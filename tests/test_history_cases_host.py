"""tests/history_cases.py is a fair test (no GPU): unique names, every dirtying call exceeds its probe in the extent its axis
names (for "<axis>-reverse" rows the probe exceeds the dirtier, and the forward row of that axis exists), the two never share
their inputs, and every axis, refusal and pool call the GPU module runs is in the table."""
import history_cases as hc

AXES = ["pairs", "in_flight", "geometry", "entry", "graph", "rows", "solver", "status", "options", "follow", "first_use"]


def test_names_are_unique():
    names = [r[0] for r in hc.ROWS]
    assert len(names) == len(set(names))
    pool = [n for n, _ in hc.POOL]
    assert len(pool) == len(set(pool)) and len(pool) >= 12
    assert len(set(hc.REFUSALS)) == len(hc.REFUSALS) == 5
    assert len({n for n, _, _ in hc.ENTRY_ROWS}) == len(hc.ENTRY_ROWS) == 6


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
    assert kinds == {"velocity", "forward", "law", "follow"}
    noise = [n for n, d, _, _ in hc.ROWS if any(c.get("frames") == "noise" for c in hc._leaves(d))]
    assert noise                                                   # a dirtier far from every probe's values
