"""tests/graph_cache_cases.py is a fair test of the captured-update cache (no GPU): every pair of FIELD_PAIRS differs in exactly
the key field it names, and in what its buffers hold or where it writes; the schedules reach the eviction, the recapture of an
evicted tuple and replays of the tuples that outlived an eviction as often as they claim; and a cache whose key has lost a field
replays the wrong capture on that field's sequence (so the GPU module, which holds every visit to the eager twin, would see it).
The figures are conditions on the case lists, not measurements."""
import pytest

import graph_cache_cases as gc

PAIR_IDS = [p[0] for p in gc.FIELD_PAIRS]


def test_the_key_has_its_fifteen_fields():
    assert len(gc.KEY_FIELDS) == len(set(gc.KEY_FIELDS)) == 15
    assert len(gc.key(gc.BASE)) == 15
    with_pair = {field for _, field, _, _ in gc.FIELD_PAIRS}
    assert with_pair | set(gc.NO_PAIR) == set(gc.KEY_FIELDS) and not with_pair & set(gc.NO_PAIR)
    assert len(PAIR_IDS) == len(set(PAIR_IDS))


@pytest.mark.parametrize("name", PAIR_IDS)
def test_a_pair_differs_in_exactly_one_key_field(name):
    _, field, base, variant = next(p for p in gc.FIELD_PAIRS if p[0] == name)
    differing = [f for f, a, b in zip(gc.KEY_FIELDS, gc.key(base), gc.key(variant)) if a != b]
    assert differing == [field], (name, differing)
    a, b = base[field], variant[field]
    if isinstance(a, str) and isinstance(b, str):                    # two addresses: other contents, or another destination
        assert gc.holds(a) != gc.holds(b) and gc.holds(a)[0] == gc.holds(b)[0], (name, a, b)
        n = base["n_pairs"]
        if field in ("I_cur", "I_des", "Z_mm", "K"):                 # ... in the rows the call reads
            assert gc.holds(a)[1:1 + n] != gc.holds(b)[1:1 + n], (name, a, b)
    assert (variant["goal"] is not None) == (variant["I_des"] is None) and base["goal"] is None
    if variant["goal"]:                                              # the cached goal is another image than the base's I_des
        assert gc.holds(variant["goal"])[1] != gc.holds(base["I_des"])[1]


def test_the_pairs_the_issue_lists_are_there():
    variants = {name: v for name, _, _, v in gc.FIELD_PAIRS}
    assert variants["I_des_null"]["I_des"] is None and variants["Z_mm_null"]["Z_mm"] is None
    d = next(p for p in gc.FIELD_PAIRS if p[0] == "des_shared")
    assert (d[2]["n_pairs"], d[2]["des_shared"], d[3]["n_pairs"], d[3]["des_shared"]) == (2, 0, 2, 1)
    assert gc.holds(d[2]["I_des"])[1] != gc.holds(d[2]["I_des"])[2]          # two different goal frames in the buffer
    n = next(p for p in gc.FIELD_PAIRS if p[0] == "n_pairs")
    assert (n[2]["n_pairs"], n[3]["n_pairs"]) == (1, 2)
    assert {gc.BASE["select_mode"], variants["select_dense"]["select_mode"], variants["select_best"]["select_mode"]} == \
        {gc.ORDER, gc.DENSE, gc.BEST}
    assert (gc.BASE["num_pairs"], variants["num_pairs"]["num_pairs"]) == (8, 12) and 12 <= gc.MAX_ROWS
    assert variants["v_c"]["v_c"] != gc.BASE["v_c"] and variants["status"]["status"] != gc.BASE["status"]
    assert len({gc.holds(f"k{j}")[1] for j in range(4)}) == 4                 # four different intrinsics


def test_the_device_schedule_is_the_one_stated():
    assert len(gc.SCHEDULE_DEV) == 40
    for i, c in enumerate(gc.SCHEDULE_DEV):
        assert (c["I_cur"], c["I_des"], c["K"], c["num_pairs"], c["v_c"], c["status"]) == \
            (f"cur{i % 5}", f"des{i % 5}", f"k{i % 4}", 4 + i % 8, f"v{i}", f"s{i}")
        assert c["select_mode"] == gc.ORDER and c["selection"]                 # a fresh order per visit: not in the key
    assert len({gc.key(c) for c in gc.SCHEDULE_DEV}) == 40
    stated = list(range(32)) + [5] + list(range(32, 40)) + [0, 1, 5, 39, 6] + list(range(40))
    assert gc.VISITS_DEV[:gc.STATED_VISITS_DEV] == stated and gc.STATED_VISITS_DEV == 86
    assert gc.VISITS_DEV[86:] == list(range(39, 7, -1))


def test_the_device_schedule_evicts_recaptures_and_replays_survivors():
    walked = gc.walk([gc.SCHEDULE_DEV[i] for i in gc.VISITS_DEV])
    n = gc.counts(walked)
    assert n["capture_evicting"] >= 8 and n["recapture"] >= 4 and n["replay_of_survivor"] >= 20, n
    assert n == {"capture": 40, "capture_evicting": 8, "recapture": 39, "replay": 39, "replay_of_survivor": 37}, n
    stated = gc.counts(walked[:gc.STATED_VISITS_DEV])                          # the stated visits alone thrash: few replays
    assert (stated["capture"], stated["recapture"], stated["replay"]) == (40, 39, 7)
    assert all(run is gc.SCHEDULE_DEV[i] for i, (_, run, _, _) in zip(gc.VISITS_DEV, walked))   # the full key never replays wrongly
    # tuple 5 is still resident when 6 is evicted: the victim is the least recently USED, not the oldest capture
    model = gc.CacheModel()
    for i in gc.VISITS_DEV:
        victim = model.visit(gc.SCHEDULE_DEV[i])[2]
        if victim is gc.SCHEDULE_DEV[6]:
            assert model.resident(gc.SCHEDULE_DEV[5])
            break
    else:
        raise AssertionError("tuple 6 is never evicted")
    victims = [gc.SCHEDULE_DEV.index(v) for _, _, v, _ in walked[:41] if v is not None]
    assert victims == [0, 1, 2, 3, 4, 6, 7, 8]                                 # 5 was replayed at visit 32: passed over


def test_every_second_round_host_visit_is_a_recapture():
    assert len(gc.SCHEDULE_HOST) == 48 > gc.CAPACITY
    assert len({gc.key(gc.host_call(c)) for c in gc.SCHEDULE_HOST}) == 48
    assert {(c["n_pairs"], c["des_shared"], c["select_mode"], c["depth"]) for c in gc.SCHEDULE_HOST} == \
        {(n, s, m, d) for n in (1, 2, 3, 4) for s in (0, 1) for m in (gc.ORDER, gc.DENSE, gc.BEST) for d in (True, False)}
    assert gc.VISITS_HOST == list(range(48)) * 2
    walked = gc.walk([gc.host_call(gc.SCHEDULE_HOST[i]) for i in gc.VISITS_HOST])
    assert [w[0] for w in walked[:48]] == ["capture"] * 48
    assert [w[0] for w in walked[48:]] == ["recapture"] * 48
    assert gc.counts(walked) == {"capture": 48, "capture_evicting": 16, "recapture": 48, "replay": 0, "replay_of_survivor": 0}


@pytest.mark.parametrize("name", PAIR_IDS)
def test_a_cache_that_lost_the_field_replays_the_wrong_capture(name):
    """The fault model: with the pair's field left out of the key, the pair's sequence replays a capture made for the other call."""
    _, field, base, variant = next(p for p in gc.FIELD_PAIRS if p[0] == name)
    seq = gc.pair_sequence(base, variant)
    assert [c is base for c in seq] == [True, False, True, False]
    whole = gc.walk(seq)
    assert [w[0] for w in whole] == ["capture", "capture", "replay", "replay"] and all(w[1] is c for w, c in zip(whole, seq))
    lost = gc.walk(seq, [f for f in gc.KEY_FIELDS if f != field])
    wrong = [i for i, (w, c) in enumerate(zip(lost, seq)) if w[0] == "replay" and w[1] is not c]
    assert wrong, (name, "the sequence would not notice the field missing from the key")


def test_the_model_evicts_the_least_recently_used():
    calls = [gc.call(v_c=f"v{i}") for i in range(4)]
    model = gc.CacheModel(capacity=2)
    seen = [model.visit(calls[i]) for i in (0, 1, 0, 2, 1, 2)]
    assert [s[0] for s in seen] == ["capture", "capture", "replay", "capture", "recapture", "replay"]
    assert seen[3][2] is calls[1] and seen[4][2] is calls[0]                   # 0 was used after 1: 1 goes first
    assert [s[3] for s in seen] == [0, 0, 0, 0, 0, 1]                          # the last replay's entry outlived one eviction
