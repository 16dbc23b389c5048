"""A long-lived handle's answers do not depend on its past (GPU).

Every other suite runs its calls on a handle made for that test, and a fresh handle's workspaces are all zero (api.hip dev_alloc):
a kernel that reads workspace the current call did not write reads zeros there, and the oracle usually agrees with zero.  Here a
probe call P runs on a handle that ran a dirtying call D first, and every output must equal, BIT FOR BIT, what P gives on a handle
that has only ever run P (the side the other suites hold to the fp64 oracle).  The rows (name, D, P, axis) are
tests/history_cases.py's; every axis test also asserts that D's outputs differ from P's, so stale values would have shown.

A snapshot of a velocity / law call: v_c, status, every array of last_details (with last_weights, last_offsets, last_goal_depth)
and of last_features; the header's promises past the rows a call defines (selected -1, everything else 0, the options' "off"
values) are asserted on both sides.  A follow-on law's snapshot: its own outputs and the camera's snapshot read after it.  A
forward-only call's: the tensors it returns.  A call in selection mode BEST adds its visiting order (last_order); after any other
mode last_order must be refused with -5.  A roll call's: v_c, status, the winner, the scores, the four n_mutual, the same-image flag
and the one-pair law's snapshot behind it."""
import ctypes as C
import dataclasses
import functools
import json

import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib, config, servo, synth, weights
from vitvs_amd.engine import Engine, VitvsError

import history_cases as hc
import rig_ref as rg
import law_support as ls

pytestmark = pytest.mark.gpu

PRECISIONS = ["fp32", "bf16", "fp16", "f16x2"]
IN_FLIGHT = [1, 3]
MAX_SWEEPS = 40


# ----------------------------------------------------------------------------------------------------- handles
@functools.lru_cache(maxsize=None)
def _model(kind):
    if kind == "real":
        cfg = config.baseline_config("vits16_224")
        return cfg, weights.synthetic_state_dict(cfg, 0)
    if kind == "law17":
        return ls.tiny_cfg(16 * 17), None
    if kind == "tiny_long":
        base = config.vit_config("dino_vits8", 8 * 23)
        cfg = dataclasses.replace(base, dim=128, depth=2, heads=2, layer=1, native_grid=base.grid)
        return cfg, weights.synthetic_state_dict(cfg, 3)
    cfg = ls.tiny_cfg(224)
    return cfg, weights.synthetic_state_dict(cfg, 3)


class Ctx:
    """One handle and what the calls on it share.  kind: "tiny" (the 2-block model, max_pairs 4, max_rows 196), "tiny_binned" (the
    same with binned descriptors: the raw-Gram workspace and the stencil), "tiny_long" (the same width at 23 x 23 tokens of 8 pixels:
    530 rows per image, where the 16-bit attention cuts its keys into ranges), "real" (ViT-S/16 224 at real width, max_pairs 4) or
    "law17" (no weights: the law alone on a 17 x 17 grid, max_rows 289)."""

    def __init__(self, kind, precision="fp32", in_flight=1):
        self.kind, self.precision, self.in_flight = kind, precision, in_flight
        self.cfg, sd = _model(kind)
        self.params = config.ServoParams(dino_input_size=self.cfg.img_size, use_feature_binning=kind == "tiny_binned")
        if kind == "law17":
            self.eng = Engine(self.cfg, self.params, precision="fp32", max_pairs=1, max_rows=289)
        else:
            self.eng = Engine(self.cfg, self.params, precision=precision, max_pairs=4, max_rows=196 if kind.startswith("tiny") else 48)
            self.eng.load_state_dict(sd)
            self.eng.set_option("in_flight", in_flight)
        self.goal_depth = False

    def close(self):
        torch.cuda.synchronize()
        self.eng.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# ----------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def _pair(seed, frames, geometry, size):
    """(des, cur) uint8 [h, w, 3] of one frame-pair seed."""
    if frames == "synth":
        assert geometry is None
        return synth.frame_pair(size, seed)
    h, w = geometry or (size, size)
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, size=(2, h, w, 3), dtype=np.uint8)        # saturated noise: far from every probe's values
    f[:, ::3, ::5] = 255
    f[:, 1::3, ::4] = 0
    return f[0], f[1]


def _frames(c, size, update=0):
    pairs = [_pair(s + 1000 * update, c.get("frames", "synth"), c.get("geometry"), size) for s in c["seeds"]]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def _depths(n):
    return np.stack([np.roll(synth.depth_pattern(), 7 * b, axis=1) for b in range(n)])


def _goal_depth():
    return (np.ascontiguousarray(synth.depth_pattern()[::-1, ::-1]).astype(np.int64) + 137).clip(1, 65535).astype(np.uint16)


def _orders(seed, n, tokens):
    return np.stack([np.random.default_rng(seed + 97 * b).permutation(tokens) for b in range(n)]).astype(np.int32)


def _rig(n):
    rng = np.random.default_rng(3)
    ext = [rg.random_extrinsic(rng, 0.3, 0.2) for _ in range(4)][:n]
    return ext, np.stack([servo.twist_matrix(R, t) for R, t in ext])


# ----------------------------------------------------------------------------------------------------- snapshots
def _np(x):
    return x.detach().cpu().numpy().copy() if torch.is_tensor(x) else np.asarray(x).copy()


def _law_snapshot(eng, v, st, n):
    snap = dict(v_c=_np(v).reshape(n, 6), status=_np(st).reshape(n))
    snap.update(eng.last_details(n))
    snap.update({"features." + k: a for k, a in eng.last_features(n).items()})
    return snap


def _with_order(eng, snap, n, best):
    """BEST: the visiting order the law ran on joins the snapshot.  Any other mode: vitvs_last_order is refused, whatever ran before."""
    if best:
        snap["order"] = eng.last_order(n)
    else:
        with pytest.raises(VitvsError, match=r"\(-5\)"):
            eng.last_order(n)
    return snap


def _check_promises(snap, options=hc.OFF):
    """include/vitvs.h: past a call's feature rows the getters return -1 / 0 whatever an earlier call left; the options' "off"
    values; a status that skips the law leaves v_c = 0."""
    n = snap["status"].shape[0]
    if "order" in snap:                                                 # a permutation of 0 .. T - 1 per pair
        tokens = snap["order"].shape[1]
        assert snap["order"].shape[0] == n and np.array_equal(np.sort(snap["order"], axis=1), np.tile(np.arange(tokens, dtype=np.int32), (n, 1)))
    for b in range(n):
        rows = int(snap["info"][b, 1])
        assert np.all(snap["selected"][b, rows:] == -1) and not snap["s_uv"][b, rows:].any() and not snap["feat"][b, rows:].any()
        assert not snap["L"][b, :, 2 * rows:].any()
        assert not snap["weights"][b, rows:].any() and not snap["offsets"][b, rows:].any() and not snap["Z_goal"][b, rows:].any()
        if snap["status"][b] != _lib.STATUS_OK:
            assert not snap["v_c"][b].any()
        elif not options[0]:
            live = int(snap["info"][b, 3])
            assert np.all(snap["weights"][b, :min(live, rows)] == 1.0) and not snap["weights"][b, live:].any()
        if not options[0]:
            assert not snap["info"][b, 6:8].any()
    if not options[1]:
        assert not snap["offsets"].any()
    if not options[2]:
        assert not snap["Z_goal"].any()


def _first_difference(a, b):
    """The first key whose arrays are not bit-identical (None: the snapshots are equal)."""
    if list(a) != list(b):
        return f"keys {sorted(set(a) ^ set(b))}"
    for key in a:
        x, y = np.asarray(a[key]), np.asarray(b[key])
        if x.dtype != y.dtype or x.shape != y.shape:
            return f"{key}: {x.dtype}{x.shape} against {y.dtype}{y.shape}"
        if x.tobytes() != y.tobytes():
            where = np.argwhere(np.atleast_1d(x != y) | (np.atleast_1d(x != x) != np.atleast_1d(y != y)))
            at = tuple(int(i) for i in where[0]) if len(where) else ()
            return f"{key} (first at {at}, {len(where)} of {x.size} elements)"
    return None


# ----------------------------------------------------------------------------------------------------- running a call
def _set_options(ctx, options):
    eng = ctx.eng
    if options[2] and not ctx.goal_depth:
        eng.set_goal_depth(_goal_depth())
        ctx.goal_depth = True
    for name, value in zip(("robust_law", "subpatch", "interaction"), options):
        eng.set_option(name, value)


def _run_velocity(ctx, c):
    eng, n, size = ctx.eng, len(c["seeds"]), ctx.cfg.img_size
    eng.set_option("in_flight", c["in_flight"] or ctx.in_flight)
    _set_options(ctx, c["options"])
    eng.set_option("select_cells", c["select_cells"])
    eng.set_frame_size(*(c["geometry"] or (None, None)))
    K, mode = ctx.params.intrinsics(), hc.SELECT[c["mode"]]
    for u in range(c["updates"]):
        des, cur = _frames(c, size, u)
        shared = c["goal"] == "shared"
        if shared:
            des = des[:1]
        elif c["goal"] == "cached":
            eng.set_goal(des)
        if c["goal"] in ("cached", "cached_keep"):
            des = None
        z = _depths(n) if c["depth"] else None
        sel = _orders(c["order_seed"] + u, n, ctx.cfg.tokens) if c["mode"] == "order" else None
        if c["entry"] == "dev":
            v, st = eng.compute_velocity(cur, des, z, K, mode=mode, selection=sel, des_shared=shared, num_pairs=c["num_pairs"])
        else:
            v, st = eng.compute_velocity_host(cur, des, z, K, mode=mode, selection=sel, des_shared=shared, num_pairs=c["num_pairs"])
            if c["entry"] == "reselect":
                v, st = eng.reselect_host(_lib.SELECT_ORDER, _orders(c["order_seed"] + 500, n, ctx.cfg.tokens), num_pairs=c["num_pairs"])
    snap = _with_order(eng, _law_snapshot(eng, v, st, n), n, c["mode"] == "best")
    _check_promises(snap, c["options"])
    if c["frames"] == "synth" and c["depth"]:
        assert not snap["status"].any() and not snap["info"][:, 2].any(), (c, snap["status"], snap["info"])   # a live law, not a shortcut
    return snap, (v, st)


def _saliency(eng, frames, heads=(0, 1)):
    """vitvs_extract_saliency_dev (Engine.extract_saliency_maps asserts the reference's model name first)."""
    f = eng._frames(frames)
    out = torch.zeros((f.shape[0], eng.tokens), dtype=torch.float32, device=eng.device)
    idx = (C.c_int32 * len(heads))(*heads)
    rc = eng.lib.vitvs_extract_saliency_dev(eng.handle, f.shape[0], C.c_void_p(f.data_ptr()), len(heads), idx, C.c_void_p(out.data_ptr()),
                                            C.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream))
    return rc, out


def _run_forward(ctx, c):
    eng, op = ctx.eng, c["op"]
    eng.set_option("in_flight", ctx.in_flight)
    eng.set_frame_size()
    des, cur = _frames(c, ctx.cfg.img_size)
    frames = np.concatenate([des, cur])
    if op == "forward_tokens":
        return dict(tokens=_np(eng.forward_tokens(frames)))
    if op == "descriptors":
        return dict(desc=_np(eng.extract_descriptors(frames)))
    if op.startswith("binned:") or op.startswith("facet:"):
        return dict(desc=_np(eng.extract_descriptors(frames, facet=op.split(":")[1], bin=op.startswith("binned:"))))
    if op == "saliency":
        rc, out = _saliency(eng, frames)
        if ctx.precision == "f16x2":                                    # refused before its forward: nothing of the handle's changes
            assert rc == -5
            return dict(refused=np.array(rc))
        assert rc == 0
        return dict(saliency=_np(out))
    g = torch.Generator().manual_seed(c["seeds"][0])
    d1, d2 = torch.randn(ctx.cfg.tokens, ctx.cfg.dim, generator=g), torch.randn(ctx.cfg.tokens, ctx.cfg.dim, generator=g)
    if op == "correspond":
        return dict(zip(("nn_1", "nn_2", "sim_1", "S"), map(_np, eng.correspond(d1, d2, want_matrix=True))))
    assert op == "refine"
    return dict(offsets=_np(eng.refine(d1, d2, torch.randperm(ctx.cfg.tokens, generator=g))))


def _run_law(ctx, c):
    """vitvs_servo_from_nn_dev on planted tables; asserts that the call is what its row says (status, solver, rows of L)."""
    eng, g, k = ctx.eng, c["grid"], c["num_pairs"]
    t = g * g
    _set_options(ctx, hc.OFF)
    eng.set_option("select_cells", c["select_cells"])
    rng = np.random.default_rng(c["table_seed"])
    nn1, nn2, sim1, mutual = ls.tables(rng, t, (2 * t) // 3)
    depth, K, pick = ls.depth(rng), ls.intrinsics(rng, ctx.params), c["pick"]
    ident = np.arange(t)
    if c["mutual"] is not None:                                  # exactly that many mutual tokens: the others' partners point elsewhere
        keep = np.sort(rng.choice(mutual, size=c["mutual"], replace=False))
        for i in np.setdiff1d(mutual, keep):
            nn2[nn1[i]] = next(x for x in range(t) if nn1[x] != nn1[i])
        mutual = keep
        assert np.array_equal(np.nonzero(nn2[nn1] == ident)[0], mutual)
    moved = np.nonzero(nn1 != ident)[0]
    ids, want = None, _lib.STATUS_OK
    if pick == "mutual" and c["mode"] != "best":
        ids = rng.choice(mutual, size=k, replace=False)
    elif pick == "mutual":
        pass                                                           # BEST draws for itself: the k best mutual tokens, spread
    elif pick == "repeat1":
        ids = np.full(k, rng.choice(moved))
    elif pick == "repeat2":
        a, b = rng.choice(moved, size=2, replace=False)
        ids = np.where(np.arange(k) < k - 4, a, b) if k >= 32 else np.resize([a, b], k)
    elif pick == "few":
        ids, want = rng.choice(mutual, size=3, replace=False), _lib.STATUS_TOO_FEW
    elif pick == "no_mutual":
        nn1, nn2, sim1, want = (ident + 1) % t, (ident + 2) % t, np.full(t, 0.5, np.float32), _lib.STATUS_NO_CORRESPONDENCE
    elif pick == "all_mutual":
        nn1, nn2, sim1, want = ident, ident, np.full(t, 0.5, np.float32), _lib.STATUS_NO_CORRESPONDENCE
    else:
        assert pick == "same_image"
        sim1 = np.ones(t, np.float32)
    if not c["depth"]:
        depth, want = None, _lib.STATUS_NO_DEPTH
    mode = hc.SELECT[c["mode"]]
    sel = None
    if c["mode"] == "explicit":
        sel = [np.asarray(ids, np.int32)]
    elif c["mode"] == "order":
        sel = rng.permutation(t).astype(np.int32)
    v, st = eng.servo_from_nn(nn1, nn2, sim1, depth, K, mode=mode, selection=sel, num_pairs=k)
    snap = _with_order(eng, _law_snapshot(eng, v, st, 1), 1, c["mode"] == "best")
    _check_promises(snap)
    info = snap["info"][0]
    assert int(snap["status"][0]) == want, (c, snap["status"])
    if want == _lib.STATUS_OK:
        assert (int(info[5]) > hc.LDS_ROWS) == (hc.extent(c, "rows")[0]), (c, info)
        if pick == "same_image":
            assert int(info[2]) == 1 and not snap["v_c"].any()
        elif pick == "mutual" and c["mode"] == "best":
            # the order's mutual class is the planted tokens; a short one fills fewer rows than the call asks for
            assert int(info[0]) == len(mutual) >= (c["mutual"] or 0) and int(info[3]) == min(len(mutual), k), (c, info, len(mutual))
            assert np.array_equal(np.sort(snap["order"][0, :len(mutual)]), mutual) and (c["mutual"] is None or len(mutual) < k)
        elif pick == "mutual":
            assert int(info[4]) == -1, (c, "expected LDL^T", info)
        elif pick in ("repeat1", "repeat2"):
            assert 0 <= int(info[4]) <= MAX_SWEEPS, (c, "expected Jacobi", info)
    return snap, (v, st)


def _run_follow(ctx, c):
    eng, cam = ctx.eng, c["camera"]
    n, N, K = len(cam["seeds"]), c["n_iter"], ctx.params.intrinsics()
    _, (v, st) = _run_velocity(ctx, cam)
    ext, Ws = _rig(n)
    if c["law"] in ("pose", "pose_rig") and not ctx.goal_depth:
        eng.set_goal_depth(_goal_depth())
        ctx.goal_depth = True
    if c["law"] in ("rig", "rig_robust"):
        v_law, status, info = eng.rig_velocity(Ws, st, robust_iterations=N, K=K if N else None)
        out = dict(v=v_law, status=status, **info)
    elif c["law"] == "pose":
        v_law, info = eng.pose_velocity(K, st, robust_iterations=N, consensus=c["consensus"], seed=c["seed"])
        out = dict(v=v_law, **info)
    elif c["law"] == "pose_rig":
        v_law, status, info = eng.pose_rig_velocity(ext, K, st, robust_iterations=N)
        out = dict(v=v_law, status=status, **info)
    else:
        assert c["law"] == "homography"
        v_law, info = eng.homography_velocity(K, st, depth_scale=0.6, robust_iterations=N, consensus=c["consensus"], seed=c["seed"])
        out = dict(v=v_law, **info)
    snap = {"law." + k: _np(a) for k, a in out.items()}
    if c["consensus"]:                                           # a live consensus start on every pair, not the fallback without one
        assert c["law"] in hc.CONSENSUS_LAWS
        assert not snap["law.status"].any() and np.all(snap["law.winner"] > 0) and np.all(snap["law.start_weights"] >= 3), \
            (c, snap["law.status"], snap["law.winner"], snap["law.start_weights"])
    else:
        assert not snap.get("law.winner", np.zeros(1)).any()
    camera = _law_snapshot(eng, v, st, n)                    # the camera's law, read AFTER the follow-on law
    _check_promises(camera, cam["options"])
    snap.update({"camera." + k: a for k, a in camera.items()})
    return snap


ROLL_WINNERS = {}                                                # (precision, in_flight, seed, turn, goal, mode) -> k*, as observed


def _run_roll(ctx, c):
    """vitvs_roll_velocity[_dev]; asserts that the search picked what the row says (c["winner"]) with a live law behind it."""
    eng, size = ctx.eng, ctx.cfg.img_size
    eng.set_option("in_flight", ctx.in_flight)
    _set_options(ctx, hc.OFF)
    eng.set_option("select_cells", c["select_cells"])
    eng.set_frame_size()
    des, cur = _pair(c["seed"], "synth", None, size)
    cur = np.ascontiguousarray(np.rot90(des if c["at_goal"] else cur, c["turn"]))
    if c["goal"] == "cached":
        eng.set_goal(des[None])
    if c["goal"] != "own":
        des = None
    sel = _orders(c["order_seed"], 1, ctx.cfg.tokens) if c["mode"] == "order" else None
    call = eng.roll_velocity if c["entry"] == "dev" else eng.roll_velocity_host
    v, st, info = call(cur, des, _depths(1)[0], ctx.params.intrinsics(), mode=hc.SELECT[c["mode"]], selection=sel, num_pairs=c["num_pairs"])
    snap = _with_order(eng, _law_snapshot(eng, v, st, 1), 1, c["mode"] == "best")
    snap["status"] = snap["status"].astype(np.int32)
    snap.update({"roll." + k: np.asarray(a).copy() for k, a in info.items()})
    _check_promises(snap)
    ROLL_WINNERS[(ctx.precision, ctx.in_flight, c["seed"], c["turn"], c["goal"], c["mode"])] = info["roll"]
    if c["winner"] != "any":
        assert (info["roll"] > 0) if c["winner"] == "nonzero" else (info["roll"] == 0), (c, info)
        assert int(snap["status"][0]) == _lib.STATUS_OK, (c, snap["status"])
        assert info["same_image"] == c["at_goal"] and int(snap["info"][0, 2]) == int(c["at_goal"]), (c, info, snap["info"])
    return snap


def _run(ctx, c):
    if c["kind"] == "roll":
        return _run_roll(ctx, c)
    if c["kind"] == "seq":
        for part in c["calls"]:
            snap = _run(ctx, part)
        return snap
    if c["kind"] == "velocity":
        return _run_velocity(ctx, c)[0]
    if c["kind"] == "forward":
        return _run_forward(ctx, c)
    if c["kind"] == "law":
        return _run_law(ctx, c)[0]
    return _run_follow(ctx, c)


_FRESH = {}


def _fresh(kind, precision, in_flight, c):
    """P's snapshot on a handle that has only ever run P, computed once."""
    key = (kind, precision, in_flight, json.dumps(c, sort_keys=True))
    if key not in _FRESH:
        with Ctx(kind, precision, in_flight) as ctx:
            _FRESH[key] = _run(ctx, c)
    return _FRESH[key]


@pytest.fixture(scope="module", autouse=True)
def _forget():
    yield
    _FRESH.clear()
    # which candidate won the roll calls of this run (the rows assert the class of each; shown with -s)
    print("\nroll winners (seed, turn, goal, mode, k*):", sorted({(*key[2:], k) for key, k in ROLL_WINNERS.items()}))
    by_call = {}
    for key, k in ROLL_WINNERS.items():
        by_call.setdefault(key[2:], set()).add(k)
    print("roll calls whose winner depends on the precision or the plan:", {c: ks for c, ks in by_call.items() if len(ks) > 1})
    ROLL_WINNERS.clear()


def _same(got, want, what):
    diff = _first_difference(got, want)
    assert diff is None, f"{what}: differs from a fresh handle in {diff}"


def _dirty_then_probe(kind, precision, in_flight, name, d, p):
    want = _fresh(kind, precision, in_flight, p)
    with Ctx(kind, precision, in_flight) as ctx:
        dirt = _run(ctx, d)
        assert _first_difference(dirt, want) is not None, f"{name}: the dirtying call leaves what the probe leaves"
        _same(_run(ctx, p), want, name)
        _same(_run(ctx, p), want, name + " (the probe once more)")


def _rows(*axes):
    return [pytest.param(d, p, id=name) for name, d, p, axis in hc.ROWS if axis.partition("-")[0] in axes]


# ----------------------------------------------------------------------------------------------------- forward-side axes
@pytest.mark.parametrize("in_flight", IN_FLIGHT)
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("d,p", _rows("pairs", "in_flight", "geometry"))
def test_pairs_plan_hint_and_frame_geometry(d, p, precision, in_flight, request):
    """Axes 1 - 3 on the tiny model: other pair counts (the split-K slices of `part`, the 64-row tile padding, the arg-max keys
    behind n_pairs * T), another in_flight plan (slice count, attention split state and tickets), another frame geometry
    (the staging buffers are reallocated, the goal cache outlives the change)."""
    _dirty_then_probe("tiny", precision, in_flight, request.node.callspec.id, d, p)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("d,p", _rows("pairs", "in_flight"))
def test_pairs_and_plan_hint_at_real_width(d, p, precision, request):
    """ViT-S/16 224 at its real width (N and K choose the slice counts and the tile families), max_pairs = 4: the batched call
    reaches the many-row tiles in the 16-bit modes, the one-pair call does not."""
    _dirty_then_probe("real", precision, 1, request.node.callspec.id, d, p)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("d,p", _rows("pairs"))
def test_pairs_with_binned_descriptors(d, p, precision, request):
    """The same with use_feature_binning: the raw-Gram workspace [max_pairs][T][T] and the token norms of the stencil form."""
    _dirty_then_probe("tiny_binned", precision, 1, request.node.callspec.id, d, p)


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("d,p", _rows("pairs", "in_flight"))
def test_divided_attention_state_and_tickets(d, p, precision, request):
    """530 token rows per image: under the in_flight hint 1 the 16-bit attention merges the key ranges of a query block through
    the handle's split state and tickets, whose layout follows the image count; from 2 on it does not divide.  The tickets must
    be back at zero, and no state of another split may be read, whatever ran before."""
    out = (C.c_int32 * 6)()
    lib = _lib.load()
    code = {"bf16": _lib.BF16, "fp16": _lib.F16}[precision]
    before = lib.vitvs_op_plan_in_flight(1)
    divided = [lib.vitvs_op_attention_plan(code, n, 530, 2, out) == 0 and out[5] == 1 for n in (2, 5, 8)]
    lib.vitvs_op_plan_in_flight(3)
    whole = lib.vitvs_op_attention_plan(code, 2, 530, 2, out) == 0 and out[5] == 0
    lib.vitvs_op_plan_in_flight(before)
    assert all(divided) and whole, "the shape does not reach the divided plan it is here for"
    _dirty_then_probe("tiny_long", precision, 1, request.node.callspec.id, d, p)


@pytest.mark.parametrize("in_flight", IN_FLIGHT)
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("when", ["goal_before", "goal_after"])
@pytest.mark.parametrize("name,d,survives", [pytest.param(*row, id=row[0]) for row in hc.ENTRY_ROWS])
def test_entry_points_and_the_goal_cache(name, d, survives, when, precision, in_flight):
    """Axis 4.  P is a velocity call on the goal cached by set_goal (I_des = None).  include/vitvs.h: the cache is dropped by any
    call that forwards frames of its own choice or rewrites the descriptors (a velocity call WITH I_des, vitvs_extract_*,
    vitvs_correspond_dev) - then P is error -5, never a twist from a stale goal - and survives the calls that do neither
    (vitvs_reselect behind a call on the cached goal, vitvs_servo_from_nn_dev) - and a call the library REFUSES: f16x2 has no
    saliency kernel, and vitvs_extract_saliency_dev says so before it forwards anything.  The roll search follows the velocity
    call: with an I_des of its own it drops the cache, with I_des = NULL it matches the cached goal and keeps it."""
    survives = survives or (name == "extract_saliency_maps" and precision == "f16x2")
    p = hc.P1_CACHED
    want = _fresh("tiny", precision, in_flight, p)
    with Ctx("tiny", precision, in_flight) as ctx:
        if when == "goal_after":
            dirt = _run(ctx, dict(d, goal="own") if d["kind"] in ("velocity", "roll") else d)
            assert _first_difference(dirt, want) is not None
            _same(_run(ctx, p), want, name)
            return
        ctx.eng.set_goal(_frames(p, ctx.cfg.img_size)[0])
        dirt = _run(ctx, d)
        assert _first_difference(dirt, want) is not None
        keep = dict(p, goal="cached_keep")
        if survives:
            _same(_run(ctx, keep), want, name + ": the cached goal survives")
        else:
            with pytest.raises(VitvsError, match=r"\(-5\)"):
                _run(ctx, keep)
        _same(_run(ctx, p), want, name + ": the goal set again")


@pytest.mark.parametrize("in_flight", IN_FLIGHT)
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("d,p", _rows("graph"))
def test_graph_replay_around_eager_calls(d, p, precision, in_flight, request):
    """Axis 5.  P captured on a side stream, D eagerly (the default stream is never captured) with other arguments and sizes,
    P replayed, then P eagerly with replay off: all three equal the fresh handle's eager P.  A BEST probe's capture holds the
    launch that makes its visiting order; a roll call is never replayed and runs eagerly between the replays of a handle that is."""
    name = request.node.callspec.id
    want = _fresh("tiny", precision, in_flight, p)
    with Ctx("tiny", precision, in_flight) as ctx:
        eng, n, k = ctx.eng, len(p["seeds"]), p["num_pairs"]
        des, cur = _frames(p, ctx.cfg.img_size)
        cur_d, des_d = eng._frames(cur), eng._frames(des)
        z_d = torch.as_tensor(_depths(n)).to(eng.device).contiguous()
        k_d = torch.as_tensor(ctx.params.intrinsics(), dtype=torch.float64).reshape(1, 4).expand(n, 4).contiguous().to(eng.device)
        best = p["mode"] == "best"                               # (the order is made on the device: nothing comes from the caller)
        sel_d = None if best else torch.as_tensor(_orders(p["order_seed"], n, ctx.cfg.tokens)).to(eng.device)
        out_v = torch.zeros((n, 6), dtype=torch.float64, device=eng.device)
        out_s = torch.zeros(n, dtype=torch.int32, device=eng.device)
        side = torch.cuda.Stream(eng.device)
        eng.set_option("in_flight", in_flight)
        eng.set_option("graph_replay", 1)
        torch.cuda.synchronize()

        def replayed():
            out_v.fill_(-1.0)
            out_s.fill_(-1)
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                eng.compute_velocity_dev(cur_d, des_d, z_d, k_d, hc.SELECT[p["mode"]], sel_d, None, out_v=out_v, out_status=out_s, num_pairs=k)
            torch.cuda.synchronize()
            return _with_order(eng, _law_snapshot(eng, out_v, out_s, n), n, best)
        _same(replayed(), want, name + ": captured")
        dirt = _run(ctx, d)
        assert _first_difference(dirt, want) is not None
        _same(replayed(), want, name + ": replayed behind the eager calls")
        eng.set_option("graph_replay", 0)
        _run(ctx, d)
        _same(_run(ctx, p), want, name + ": eager, replay off")


# ----------------------------------------------------------------------------------------------------- law-side axes (fp32)
@pytest.mark.parametrize("d,p", _rows("rows", "solver", "status"))
def test_law_rows_solver_and_statuses(d, p, request):
    """Axes 6 - 8 through vitvs_servo_from_nn_dev on a 17 x 17 grid (max_rows 289): L in the global workspace or in LDS, LDL^T or
    the Jacobi SVD (which overwrites its working copy of L), every status that skips the law.  _run_law asserts that each call
    is what its row says: the status, the solver through info[4], the side of the LDS edge through info[5]."""
    _dirty_then_probe("law17", "fp32", 1, request.node.callspec.id, d, p)


@pytest.mark.parametrize("d,p", _rows("options"))
def test_law_options(d, p, request):
    """Axis 9: robust_law, subpatch and interaction (with a goal depth) on, then off, and the reverse; the getters return the fresh
    handle's values, the "off" values included (_check_promises)."""
    _dirty_then_probe("tiny", "fp32", 1, request.node.callspec.id, d, p)


@pytest.mark.parametrize("d,p", _rows("follow", "first_use"))
def test_follow_on_laws(d, p, request):
    """Axis 10: each follow-on law behind a large, re-weighted use and behind a small plain one, in both orders, and called for
    the first time (its block is allocated then) on a handle that has run 20 updates.  The camera's own v_c and detail block,
    read after the follow-on law, equal the fresh handle's as well."""
    _dirty_then_probe("tiny", "fp32", 1, request.node.callspec.id, d, p)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("d,p", [r for r in _rows("select") if r.values[0]["kind"] != "law"])
def test_best_selection_through_the_forward(d, p, precision, request):
    """Axis 12 through the forward: BEST's visiting order of n_pairs * T tokens in the handle's workspace behind a larger one, an
    ORDER call behind a BEST call (vitvs_last_order is refused again) and the reverse, select_cells 4 and 1 in both orders."""
    _dirty_then_probe("tiny", precision, 1, request.node.callspec.id, d, p)


@pytest.mark.parametrize("d,p", [r for r in _rows("select") if r.values[0]["kind"] == "law"])
def test_best_selection_on_planted_tables(d, p, request):
    """Axis 12 on planted tables (17 x 17 tokens): an order with 12 mutual tokens for 24 feature pairs behind one with 192, and the
    reverse - the short one's zero-padded rows borrow nothing from the long one's tail - and an order without any mutual token."""
    _dirty_then_probe("law17", "fp32", 1, request.node.callspec.id, d, p)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("d,p", _rows("consensus"))
def test_consensus_starts(d, p, precision, request):
    """Axis 14: the pose and the homography law with 4096, 256 and no hypotheses, with another seed, behind three cameras and
    two, in the law's one scratch block; _run_follow asserts that every consensus start is a live one."""
    _dirty_then_probe("tiny", precision, 1, request.node.callspec.id, d, p)


@pytest.mark.parametrize("in_flight", IN_FLIGHT)
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("d,p", _rows("roll"))
def test_roll_search(d, p, precision, in_flight, request):
    """Axis 13: a roll call forwards five images, fills the keys of four pairs, rewrites pair 0's in place from the winner's and
    leaves the flag `rolled` and a one-pair law behind; plain calls of one pair and of four pairs with four goals behind it, a
    roll call behind those, winner 0 (the pick's early return) behind winner 3, the pose law's consensus start on either side."""
    _dirty_then_probe("tiny", precision, in_flight, request.node.callspec.id, d, p)


def _refuse(ctx, kind):
    """One call the library rejects on the host (the refusals of the existing test_error_returns / test_*_refusals tests)."""
    eng, lib, dev = ctx.eng, ctx.eng.lib, ctx.eng.device
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)  # noqa: E731
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)  # noqa: E731
    des, cur = _frames(hc.P1, ctx.cfg.img_size)
    if kind == "num_pairs_above_max_rows":
        with pytest.raises(VitvsError, match=r"\(-5\)"):
            eng.compute_velocity_dev(eng._frames(cur), eng._frames(des), None, f64(1, 4), _lib.SELECT_DENSE, num_pairs=eng.max_rows + 1)
    elif kind == "half_a_geometry":
        assert lib.vitvs_set_frame_size(eng.handle, 0, 5) == -5
    elif kind == "null_pointer":
        assert lib.vitvs_rig_velocity_dev(eng.handle, 2, None, ptr(i32(2)), ptr(f64(6)), ptr(i32(1)), None, None, None) == -1
        assert lib.vitvs_compute_velocity_dev(eng.handle, 1, None, None, 0, None, ptr(f64(1, 4)), _lib.SELECT_DENSE, None, None, 0,
                                              ptr(f64(1, 6)), ptr(i32(1)), None) == -1
    elif kind == "robust_iterations_17":
        assert lib.vitvs_rig_robust_velocity_dev(eng.handle, 2, ptr(f64(2, 36)), ptr(i32(2)), ptr(f64(2, 4)), 17, ptr(f64(6)), ptr(i32(1)),
                                                 None, None, None, None, None) == -2
        assert lib.vitvs_pose_velocity_dev(eng.handle, 2, ptr(f64(2, 4)), ptr(i32(2)), 17, ptr(f64(2, 6)), ptr(i32(2)), None, None, None,
                                           None, None) == -2
    else:
        assert kind == "f16x2_saliency" and ctx.precision == "f16x2"
        assert _saliency(eng, np.stack([des[0], cur[0]]))[0] == -5
    torch.cuda.synchronize()


@pytest.mark.parametrize("precision", ["fp32", "f16x2"])
def test_refused_calls_leave_no_trace(precision):
    """Axis 11: between D and P one refused call of each kind (the f16x2 saliency refusal on an f16x2 handle, where it is one).
    P, the rig law behind it and the robust rig law behind that equal the fresh handle's: the tickets are where they should be."""
    cam = hc.velocity(hc.PROBE_SEEDS[:2])
    probes = [hc.follow("rig", 0, cam), hc.follow("rig_robust", 4, cam), hc.follow("rig", 0, cam)]
    want = [_fresh("tiny", precision, 1, p) for p in probes[:2]]
    want.append(want[0])
    with Ctx("tiny", precision, 1) as ctx:
        dirt = _run(ctx, hc.follow("rig_robust", 4, hc.velocity(hc.DIRT_SEEDS[:3], frames="noise", order_seed=12, num_pairs=130)))
        assert _first_difference(dirt, want[0]) is not None
        for kind in hc.REFUSALS:
            if kind != "f16x2_saliency" or precision == "f16x2":
                _refuse(ctx, kind)
        for i, (p, w) in enumerate(zip(probes, want)):
            _same(_run(ctx, p), w, f"probe {i} behind the refused calls")
            for kind in hc.REFUSALS[:4]:
                _refuse(ctx, kind)


# ----------------------------------------------------------------------------------------------------- one long mixed sequence
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_a_seeded_sequence_of_mixed_calls(precision):
    """60 calls drawn with a fixed seed from history_cases.POOL on ONE handle; each equals its snapshot from a handle that ran
    nothing else.  A mismatch names the step, the call, the call before it and the first differing array."""
    want = {name: _fresh("tiny", precision, 1, c) for name, c in hc.POOL}
    draws = np.random.default_rng(20250).integers(0, len(hc.POOL), size=60)
    draws[:len(hc.POOL)] = np.random.default_rng(7).permutation(len(hc.POOL))      # every call at least once
    with Ctx("tiny", precision, 1) as ctx:
        previous = "(none: a fresh handle)"
        for step, i in enumerate(draws):
            name, c = hc.POOL[int(i)]
            diff = _first_difference(_run(ctx, c), want[name])
            assert diff is None, f"step {step}: {name} after {previous} differs from a fresh handle in {diff}"
            previous = name
