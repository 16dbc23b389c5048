"""The cases of tests/test_gpu_graph_cache.py and a model of the captured-update cache, as plain data (no GPU, no torch).

With option graph_replay a velocity call is captured once per argument tuple and replayed afterwards (api.hip, replay_update); a
handle keeps `CAPACITY` = 32 captures and evicts the least recently used.  The key of a capture has the 15 fields of `KEY_FIELDS`.

A call is a dict of what the key is made of, with buffers by NAME (the GPU module allocates each name once and keeps it alive, so a
name is an address): `n_pairs`, `I_cur`, `I_des` (None: the goal cached by set_goal), `des_shared`, `Z_mm` (None: no depth image),
`K`, `select_mode`, `num_pairs`, `selection` / `n_selected` (given or not: their contents are not in the key), `v_c`, `status`;
and `goal`, which is NOT in the key: the goal buffer whose first frames set_goal caches in front of a call with `I_des` None.
`holds(name)` says what a buffer holds:
  cur<j> / des<j>   four frames each: the current / goal frames of synth.frame_pair seeds FRAME_SEED + 4 j .. + 3
  z<j>              four depth images: synth.depth_pattern and its three flips, rotated by j
  k<j>              four intrinsics: INTRINSICS rotated by j
  v<i> / s<i>       a call's outputs: twists [4, 6] and statuses [4]

`FIELD_PAIRS`: (id, field, base, variant) - the variant differs from its base in that key field only, and its answer or its
destination is another one, so a handle that replays the base's capture for the variant (the field dropped from the key, or compared
wrongly) answers wrongly or writes to the wrong place; the GPU test runs base, variant, base, variant.  Key fields WITHOUT a pair:
  selection given, n_selected given   check_selection accepts both forms only where the law reads neither (the selection under
                    DENSE and BEST, n_selected under ORDER, DENSE and BEST: servo.hip reads it in EXPLICIT alone), so two calls that
                    differ in one of them alone give the same answer at the same place: no test can tell their captures apart, and
                    replaying the one for the other would not be wrong
  the two frame-geometry ints         changing them drops the whole cache by design (vitvs_set_frame_size): tests/test_gpu_resize.py
  the detail block                    allocated once at vitvs_create; no call changes it during a handle's life
`SCHEDULE_DEV` / `VISITS_DEV`: 40 device-form tuples on one handle, past the capacity.  The visits are 0 .. 31; 5 again (the least
recently used is then no longer the oldest capture); 32 .. 39; 0, 1, 5, 39, 6; the 40 tuples once more - `STATED_VISITS_DEV` of
them, under the model 40 captures (8 of them evict), 39 recaptures and 7 replays: cyclic access over 40 keys makes nearly every
visit of the last round a recapture.  Replays of tuples that outlived an eviction are what shows that evicting one entry leaves the
others whole, so the 32 tuples then resident are visited once more, newest first (32 replays, no capture).
`SCHEDULE_HOST`: 48 host-form tuples, visited in order, twice: every visit of the second round is a recapture of an evicted
tuple (the worst case of an LRU).
`CacheModel` is the cache in 30 lines; a model whose key omits a field is the fault tests/test_graph_cache_host.py holds every
pair's sequence against."""
from collections import OrderedDict

EXPLICIT, ORDER, DENSE, BEST = 0, 1, 2, 3       # include/vitvs.h VITVS_SELECT_*
CAPACITY = 32
TOKENS = 16                 # of the tiny model at 64 x 64 (a 4 x 4 grid)
MAX_PAIRS, MAX_ROWS = 4, 16
FRAME_SEED = 20250801
INTRINSICS = ((502.3016357421875, 502.3016357421875, 320.0, 240.0), (431.0, 467.0, 309.5, 251.25),
              (611.5, 583.25, 333.0, 229.0), (355.75, 349.0, 301.0, 262.5))
KEY_FIELDS = ("n_pairs", "I_cur", "I_des", "des_shared", "Z_mm", "K", "select_mode", "num_pairs", "selection", "n_selected",
              "v_c", "status", "in_h", "in_w", "details")
HANDLE_FIELDS = {"in_h": 64, "in_w": 64, "details": "the handle's"}      # the same for every call of these tests


def call(**fields):
    base = dict(n_pairs=1, I_cur="cur0", I_des="des0", des_shared=0, Z_mm="z0", K="k0", select_mode=ORDER, num_pairs=8,
                selection=True, n_selected=False, v_c="v0", status="s0", goal=None)
    assert set(fields) <= set(base), fields
    return dict(base, **fields)


def key(c, fields=KEY_FIELDS):
    """The cache key of a call, or its projection on some of the fields."""
    full = dict(HANDLE_FIELDS, **c)
    return tuple(full[f] for f in fields)


def holds(name):
    """What a buffer holds (hashable): two names hold the same data exactly when this is equal."""
    kind, j = name.rstrip("0123456789"), int(name[len(name.rstrip("0123456789")):])
    if kind in ("cur", "des"):
        return (kind,) + tuple(FRAME_SEED + 4 * j + f for f in range(MAX_PAIRS))
    if kind == "z":
        return (kind,) + tuple((j + f) % 4 for f in range(MAX_PAIRS))        # which flip of the depth pattern
    if kind == "k":
        return (kind,) + tuple(INTRINSICS[(j + f) % 4] for f in range(MAX_PAIRS))
    if kind in ("v", "s"):
        return (kind, j)                                                     # outputs: a place, not contents
    raise KeyError(name)


def describe(c):
    return ", ".join(f"{f}={c[f]}" for f in KEY_FIELDS[:12]) + (f", goal={c['goal']}" if c["goal"] else "")


class CacheModel:
    """replay_update's cache: `capacity` keys, least recently used (captured or replayed) evicted.  `fields`: what its key is made
    of - all of KEY_FIELDS, or fewer for a cache that has lost one."""

    def __init__(self, fields=KEY_FIELDS, capacity=CAPACITY):
        self.fields, self.capacity = tuple(fields), capacity
        self.entries = OrderedDict()            # key -> [the call it was captured for, evictions it has outlived]
        self.gone = set()

    def visit(self, c):
        """(what, the call whose capture runs, the evicted call or None, evictions the entry had outlived); what is "capture",
        "replay", or "recapture" for a key seen before and since evicted."""
        k = key(c, self.fields)
        if k in self.entries:
            self.entries.move_to_end(k)
            return ("replay", self.entries[k][0], None, self.entries[k][1])
        what, victim = ("recapture" if k in self.gone else "capture"), None
        if len(self.entries) >= self.capacity:
            gone, (victim, _) = self.entries.popitem(last=False)
            self.gone.add(gone)
            for e in self.entries.values():
                e[1] += 1
        self.entries[k] = [c, 0]
        return (what, c, victim, 0)

    def resident(self, c):
        return key(c, self.fields) in self.entries


def walk(visits, fields=KEY_FIELDS):
    """[(what, captured_for, victim, outlived)] of a list of calls under a model with these key fields."""
    model = CacheModel(fields)
    return [model.visit(c) for c in visits]


# ---------------------------------------------------------------------------------------------- one pair per key field
BASE = call()
BASE_2 = call(n_pairs=2)
FIELD_PAIRS = [
    ("I_cur", "I_cur", BASE, call(I_cur="cur1")),                            # another address holding other frames
    ("I_des", "I_des", BASE, call(I_des="des1")),
    ("I_des_null", "I_des", BASE, call(I_des=None, goal="des1")),            # the cached goal of another image
    ("des_shared", "des_shared", BASE_2, call(n_pairs=2, des_shared=1)),     # des0 holds two different goal frames
    ("n_pairs", "n_pairs", BASE, BASE_2),                                    # the same buffers: one more row written
    ("Z_mm", "Z_mm", BASE, call(Z_mm="z1")),
    ("Z_mm_null", "Z_mm", BASE, call(Z_mm=None)),                            # status VITVS_NO_DEPTH
    ("K", "K", BASE, call(K="k1")),
    ("select_dense", "select_mode", BASE, call(select_mode=DENSE)),          # (the order still given: it is not read)
    ("select_best", "select_mode", BASE, call(select_mode=BEST)),
    ("num_pairs", "num_pairs", BASE, call(num_pairs=12)),
    ("v_c", "v_c", BASE, call(v_c="v1")),
    ("status", "status", BASE, call(status="s1")),
]
NO_PAIR = ("selection", "n_selected", "in_h", "in_w", "details")             # (the module docstring says why)


def pair_sequence(base, variant):
    return [base, variant, base, variant]


# ---------------------------------------------------------------------------------------------- past the capacity
SCHEDULE_DEV = [call(I_cur=f"cur{i % 5}", I_des=f"des{i % 5}", K=f"k{i % 4}", num_pairs=4 + i % 8, v_c=f"v{i}", status=f"s{i}")
                for i in range(40)]
_STATED = list(range(32)) + [5] + list(range(32, 40)) + [0, 1, 5, 39, 6] + list(range(40))
STATED_VISITS_DEV = len(_STATED)                                             # 86
VISITS_DEV = _STATED + list(range(39, 7, -1))                                # + the 32 residents, newest first
N_OUTPUTS = len(SCHEDULE_DEV)                                                # output buffers v0 .. v39, s0 .. s39

SCHEDULE_HOST = [dict(n_pairs=n, des_shared=shared, select_mode=mode, depth=depth)
                 for n in (1, 2, 3, 4) for shared in (0, 1) for mode in (ORDER, DENSE, BEST) for depth in (True, False)]
VISITS_HOST = list(range(len(SCHEDULE_HOST))) * 2


def host_call(c):
    """A host-form tuple as the call replay_update sees: every address is one of the handle's own staging block."""
    return call(n_pairs=c["n_pairs"], I_cur="cur0", I_des="des0", des_shared=c["des_shared"], Z_mm="z0" if c["depth"] else None,
                select_mode=c["select_mode"], n_selected=True)


def counts(walked):
    """What the summary states of a schedule: captures, captures that evict, recaptures, replays, replays of survivors."""
    n = {"capture": 0, "capture_evicting": 0, "recapture": 0, "replay": 0, "replay_of_survivor": 0}
    for what, _, victim, outlived in walked:
        n[what] += 1
        n["capture_evicting"] += what == "capture" and victim is not None
        n["replay_of_survivor"] += what == "replay" and outlived > 0
    return n
