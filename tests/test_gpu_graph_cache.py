"""The captured-update cache of a handle with option graph_replay, against an eager twin (GPU).

replay_update (api.hip) captures a velocity call once per argument tuple - a key of 15 fields, addresses among them - and replays
it afterwards; a handle keeps 32 captures and evicts the least recently used.  A key that has lost a field, or compares one
wrongly, replays ANOTHER call's capture: the twist goes to the previous caller's buffer, the law reads the previous intrinsics or
runs for the previous num_pairs.  Nothing faults; the answer is wrong.  Here every call of a replaying handle is held to the same
call on its twin, a handle with graph_replay 0 that shares nothing with it but the weights' values and the buffers: the twin runs
the same launches, so the two are equal BIT FOR BIT (include/vitvs.h promises that of a replay) - twists, statuses, and
last_details' `selected` and `info`.  The eager path itself is held to fp64 by tests/test_gpu_servo_cover.py and
tests/test_gpu_path.py; tests/test_gpu_path.py::test_graph_replay_matches_eager holds one to four tuples per handle, this module
what follows from many: each key field (tests/graph_cache_cases.py FIELD_PAIRS), the eviction, the recapture of an evicted
tuple, replays of the tuples that outlived an eviction (SCHEDULE_DEV, SCHEDULE_HOST), and a full cache dropped by an option.

Handles: the two-block tiny model (tests/law_support.py tiny_cfg(64): 16 tokens, width 128), fp32, max_pairs 4, max_rows 16.
The replaying handle is driven on a side stream (the library never replays on the null stream), the twin on the same one.  All
input and output buffers are made once per module and kept alive: every name of graph_cache_cases is one stable address.  Before
a call the output buffers are filled with sentinels (NaN twists, status -7), so a write to the wrong place shows as a sentinel
where an answer belongs and an answer where a sentinel belongs.  A failed comparison names the visit, the tuple and what the
model of the cache says the visit was: a miss on a "replay" reads "replayed the wrong entry", one on a "recapture" "the capture
after an eviction differs".

No test synchronises less than the header allows, and none destroys a handle with work in flight: the back-to-back test enqueues
calls on ONE stream with no host synchronisation between them, which is the use the header allows for `_dev` calls; the eviction
itself drains the device before it destroys the victim's graph (replay_update).

That the module notices a damaged key was checked once against a library made to zero one key field at a time: each of the ten
fields with a pair failed exactly its own pairs (n_pairs, des_shared, Z_mm and select_mode the host schedule as well), and the
whole key passed.  Module time on an MI355X: 3.0 - 3.6 s for the 17 tests (0.8 s of it the handles and buffers; the longest
test 0.13 s) - 318 captures of the update's graph and about as many eager calls."""
import types

import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib, config, synth, weights
from vitvs_amd.engine import Engine

import graph_cache_cases as gc
import law_support as ls

pytestmark = pytest.mark.gpu

NAN_STATUS = -7
HINT = {"capture": "the first capture of this tuple differs from the eager call",
        "replay": "replayed the wrong entry (or a damaged one)",
        "recapture": "the capture after an eviction differs"}


# ----------------------------------------------------------------------------------------------------- buffers and handles
def _content(name):
    """numpy contents of an input buffer, from what graph_cache_cases.holds says of it."""
    kind, *rows = gc.holds(name)
    if kind in ("cur", "des"):
        return np.stack([synth.frame_pair(64, seed)[0 if kind == "des" else 1] for seed in rows])
    if kind == "z":
        p = synth.depth_pattern()
        flips = (p, p[::-1], p[:, ::-1], p[::-1, ::-1])
        return np.stack([np.ascontiguousarray(flips[f]) for f in rows])
    assert kind == "k"
    return np.array(rows, np.float64)


@pytest.fixture(scope="module")
def rig():
    assert _lib.SELECT_ORDER == gc.ORDER and _lib.SELECT_DENSE == gc.DENSE and _lib.SELECT_BEST == gc.BEST
    cfg = ls.tiny_cfg(64)
    assert cfg.tokens == gc.TOKENS
    params = config.ServoParams(dino_input_size=64, use_feature_binning=False, num_pairs=8)
    sd = weights.synthetic_state_dict(cfg, 5)
    dev = torch.device("cuda", torch.cuda.current_device())
    R = types.SimpleNamespace(cfg=cfg, params=params, dev=dev, side=torch.cuda.Stream(dev), made=[])
    names = [f"{k}{j}" for k in ("cur", "des") for j in range(5)] + ["z0", "z1"] + [f"k{j}" for j in range(4)]
    R.host = {name: _content(name) for name in names}
    R.buf = {name: torch.from_numpy(a).to(dev).contiguous() for name, a in R.host.items()}
    for i in range(gc.N_OUTPUTS):
        R.buf[f"v{i}"] = torch.empty((gc.MAX_PAIRS, 6), dtype=torch.float64, device=dev)
        R.buf[f"s{i}"] = torch.empty(gc.MAX_PAIRS, dtype=torch.int32, device=dev)
    assert len({t.data_ptr() for t in R.buf.values()}) == len(R.buf)
    # one visiting order per visit and pair (seeded by the visit's index): the selection's contents are outside the key
    n_orders = 512
    R.orders_host = np.stack([np.stack([np.random.default_rng(1000 * v + b).permutation(gc.TOKENS) for b in range(gc.MAX_PAIRS)])
                              for v in range(n_orders)]).astype(np.int32)
    R.orders = torch.from_numpy(R.orders_host).to(dev)

    def handle(graph_replay):
        eng = Engine(cfg, params, precision="fp32", max_pairs=gc.MAX_PAIRS, max_rows=gc.MAX_ROWS).load_state_dict(sd)
        eng.set_option("graph_replay", graph_replay)
        R.made.append(eng)
        return eng
    R.handle = handle
    R.twin = handle(0)
    torch.cuda.synchronize()
    yield R
    torch.cuda.synchronize()
    for eng in R.made:
        eng.close()


@pytest.fixture
def replaying(rig):
    """A fresh handle with graph_replay 1: an empty cache, whatever ran before."""
    eng = rig.handle(1)
    yield eng
    torch.cuda.synchronize()
    eng.close()


def _outputs(*calls):
    return sorted({c[f] for c in calls for f in ("v_c", "status")})


def _fill(R, names):
    for name in names:
        R.buf[name].fill_(float("nan") if name.startswith("v") else NAN_STATUS)


def _enqueue(R, eng, c, visit):
    """The call `c` with the visiting order of `visit`, on torch's current stream; nothing synchronises."""
    n, n_des = c["n_pairs"], 1 if c["des_shared"] else c["n_pairs"]
    if c["goal"]:
        eng.set_goal(R.buf[c["goal"]][:n_des])
    des = None if c["I_des"] is None else R.buf[c["I_des"]][:n_des]
    z = None if c["Z_mm"] is None else R.buf[c["Z_mm"]][:n]
    sel = R.orders[visit][:n] if c["selection"] else None
    assert not c["n_selected"]
    eng.compute_velocity_dev(R.buf[c["I_cur"]][:n], des, z, R.buf[c["K"]][:n], c["select_mode"], sel, None,
                             des_shared=bool(c["des_shared"]), out_v=R.buf[c["v_c"]], out_status=R.buf[c["status"]],
                             num_pairs=c["num_pairs"])


def _visit(R, eng, c, visit, outs):
    """One synchronised visit: sentinels into `outs`, the call, then `outs` and the details as host arrays."""
    with torch.cuda.stream(R.side):
        _fill(R, outs)
        _enqueue(R, eng, c, visit)
    R.side.synchronize()
    got = {name: R.buf[name].cpu().numpy().copy() for name in outs}
    det = eng.last_details(c["n_pairs"])
    got["selected"], got["info"] = det["selected"].copy(), det["info"].copy()
    return got


def _differing(a, b):
    return [k for k in a if a[k].shape != b[k].shape or not np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f")]


def _label(visit, what, c, index=None):
    return f"visit {visit}: tuple {'' if index is None else index} ({gc.describe(c)}), by the model a {what}: {HINT[what]}"


def _sentinels_elsewhere(got, c, outs, label):
    for name in outs:
        if name not in (c["v_c"], c["status"]):
            clean = np.isnan(got[name]).all() if name.startswith("v") else (got[name] == NAN_STATUS).all()
            assert clean, (label, f"{name} is not this call's and was written")
    n = c["n_pairs"]
    assert np.isnan(got[c["v_c"]][n:]).all() and (got[c["status"]][n:] == NAN_STATUS).all(), (label, "rows past n_pairs were written")
    assert not np.isnan(got[c["v_c"]][:n]).any() and (got[c["status"]][:n] != NAN_STATUS).all(), (label, "the call's rows were not written")


@pytest.fixture(scope="module")
def twin_dev(rig):
    """The twin's answer to every visit of VISITS_DEV (made once: both capacity tests and the option test read it)."""
    return [_visit(rig, rig.twin, gc.SCHEDULE_DEV[i], v, _outputs(gc.SCHEDULE_DEV[i])) for v, i in enumerate(gc.VISITS_DEV)]


# ----------------------------------------------------------------------------------------------------- one pair per key field
@pytest.mark.parametrize("name", [p[0] for p in gc.FIELD_PAIRS])
def test_each_key_field_selects_its_own_capture(rig, replaying, name):
    """base, variant, base, variant on a fresh handle: two captures, then a replay of each.  Per visit the twin runs BOTH tuples
    with the visit's order: the called one is what the replaying handle must give, the other one is what it would give had it
    replayed the other tuple's capture - and the two must differ (in an answer or in where it goes), or the visit proves nothing."""
    _, field, base, variant = next(p for p in gc.FIELD_PAIRS if p[0] == name)
    seq = gc.pair_sequence(base, variant)
    outs = _outputs(base, variant)
    for visit, (c, walked) in enumerate(zip(seq, gc.walk(seq))):
        other = variant if c is base else base
        label = _label(visit, walked[0], c)
        if_other = _visit(rig, rig.twin, other, visit, outs)
        want = _visit(rig, rig.twin, c, visit, outs)
        assert _differing(want, if_other), (label, f"the twin answers the two tuples alike: the pair cannot tell their captures apart ({field})")
        _sentinels_elsewhere(want, c, outs, label + " [the twin]")
        got = _visit(rig, replaying, c, visit, outs)
        assert not _differing(got, want), (label, _differing(got, want), {k: (got[k], want[k]) for k in _differing(got, want)})
        _sentinels_elsewhere(got, c, outs, label)
        if c["Z_mm"] is None:
            assert (want[c["status"]][:c["n_pairs"]] == _lib.STATUS_NO_DEPTH).all(), label


# ----------------------------------------------------------------------------------------------------- past the capacity
def _dev_visits():
    visits = [gc.SCHEDULE_DEV[i] for i in gc.VISITS_DEV]
    return list(zip(gc.VISITS_DEV, visits, gc.walk(visits)))


def test_past_capacity_synchronised(rig, replaying, twin_dev):
    """SCHEDULE_DEV on one handle, the stream synchronised after every visit: 40 captures (8 evict), 39 recaptures, 39 replays,
    37 of them of tuples that outlived an eviction.  Every visit equals the twin's."""
    for visit, (i, c, walked) in enumerate(_dev_visits()):
        outs = _outputs(c)
        got = _visit(rig, replaying, c, visit, outs)
        label = _label(visit, walked[0], c, i)
        assert not _differing(got, twin_dev[visit]), (label, _differing(got, twin_dev[visit]))
        _sentinels_elsewhere(got, c, outs, label)


def test_past_capacity_back_to_back(rig, replaying, twin_dev):
    """The same schedule enqueued on the side stream with no host synchronisation between the calls (the header allows `_dev` calls
    on one stream back to back): a 33rd tuple then evicts a capture whose launch may still be queued, which is why the eviction
    drains the device first.  One synchronisation at the end; every tuple's buffers hold the twin's answer to its LAST visit."""
    last = {}
    for visit, (i, c, walked) in enumerate(_dev_visits()):
        last[i] = (visit, walked[0])
    everything = _outputs(*gc.SCHEDULE_DEV)
    with torch.cuda.stream(rig.side):
        _fill(rig, everything)
        for visit, (i, c, _) in enumerate(_dev_visits()):
            _enqueue(rig, replaying, c, visit)
    rig.side.synchronize()
    for i, c in enumerate(gc.SCHEDULE_DEV):
        visit, what = last[i]
        for name in _outputs(c):
            got, want = rig.buf[name].cpu().numpy(), twin_dev[visit][name]
            assert np.array_equal(got, want, equal_nan=True), (_label(visit, what, c, i), name, got, want)
    # the details are those of the call made last
    det = replaying.last_details(1)
    assert np.array_equal(det["selected"], twin_dev[-1]["selected"]) and np.array_equal(det["info"], twin_dev[-1]["info"])


def test_a_full_cache_is_dropped_whole(rig, replaying, twin_dev):
    """32 captures, then option robust_law 0 -> 2 (drop_graphs walks 32 entries): tuples 0, 17 and 31 equal the twin under the same
    option - recaptured, not replayed from a capture of the plain law - and again after the option is set back."""
    for visit in range(gc.CAPACITY):
        c = gc.SCHEDULE_DEV[gc.VISITS_DEV[visit]]
        got = _visit(rig, replaying, c, visit, _outputs(c))
        assert not _differing(got, twin_dev[visit]), _label(visit, "capture", c, visit)
    plain = {}
    try:
        for robust, visit in ((2, 200), (0, 300)):
            rig.twin.set_option("robust_law", robust)
            replaying.set_option("robust_law", robust)
            for i in (0, 17, 31):
                c, outs = gc.SCHEDULE_DEV[i], _outputs(gc.SCHEDULE_DEV[i])
                want = _visit(rig, rig.twin, c, visit + i, outs)
                got = _visit(rig, replaying, c, visit + i, outs)
                label = f"robust_law {robust}, tuple {i} ({gc.describe(c)}): a capture made under the previous option was replayed?"
                assert not _differing(got, want), (label, _differing(got, want))
                assert (want[c["status"]][:1] == _lib.STATUS_OK).all(), label
                plain[(robust, i)] = rig.twin.last_weights(1)[0].copy()
        # the option does change the law on these inputs (a Tukey weight strictly between 0 and 1; the plain law's are 1 on live
        # rows and 0 on padded ones), so the captures under the two settings are not alike
        assert any(((plain[(2, i)] > 0.0) & (plain[(2, i)] < 1.0)).any() for i in (0, 17, 31))
        assert all(np.isin(plain[(0, i)], (0.0, 1.0)).all() for i in (0, 17, 31))
    finally:
        rig.twin.set_option("robust_law", 0)


# ----------------------------------------------------------------------------------------------------- the host-pointer form
def test_host_form_thrashes_the_cache(rig, replaying):
    """SCHEDULE_HOST through compute_velocity_host, in order, twice: 48 tuples on 32 places, so every visit of the second round
    recaptures an evicted tuple.  Statuses, twists and the host-served details are equal per visit; then vitvs_reselect."""
    visits = [gc.SCHEDULE_HOST[i] for i in gc.VISITS_HOST]
    walked = gc.walk([gc.host_call(c) for c in visits])
    H = rig.host
    for visit, (i, c, w) in enumerate(zip(gc.VISITS_HOST, visits, walked)):
        n, n_des = c["n_pairs"], 1 if c["des_shared"] else c["n_pairs"]
        order = rig.orders_host[visit][:n] if c["select_mode"] == gc.ORDER else None
        answers = []
        for eng in (rig.twin, replaying):
            v, st = eng.compute_velocity_host(H["cur0"][:n], H["des0"][:n_des], H["z0"][:n] if c["depth"] else None, H["k0"][:n],
                                              mode=c["select_mode"], selection=order, des_shared=bool(c["des_shared"]))
            det = eng.last_details(n)
            answers.append(dict(v_c=v.copy(), status=st.copy(), **{k: det[k].copy() for k in ("nn_1", "nn_2", "sim_1", "info")}))
        want, got = answers
        label = f"visit {visit}: host tuple {i} ({c}), by the model a {w[0]}: {HINT[w[0]]}"
        assert not _differing(got, want), (label, _differing(got, want))
        assert (want["status"] == (_lib.STATUS_OK if c["depth"] else _lib.STATUS_NO_DEPTH)).all(), (label, want["status"])
    order = rig.orders_host[400][:visits[-1]["n_pairs"]]
    want, got = (eng.reselect_host(gc.ORDER, order) for eng in (rig.twin, replaying))
    assert np.array_equal(got[0], want[0], equal_nan=True) and np.array_equal(got[1], want[1]), ("vitvs_reselect after the last visit", got, want)
