"""Test infrastructure (never shipped): systems for the control laws' 6 x 6 solve with the conditioning as a knob, on both sides
of the hand-off from LDL^T to the Jacobi SVD (vit-vs_amd/csrc/solve.h; tests/solve_ref.py owns the threshold and the references).

Every camera case is one ``Engine.servo_from_nn`` call in EXPLICIT mode on a tiny handle (tests/law_support.TinyEngines).  The
interaction matrix is built at the CURRENT features, so a case designs the current tokens and matches every one of them to a goal
token displaced by -2 .. 2 patches (clipped to the grid, all distinct): e is then a non-zero, inconsistent right-hand side.  With a
constant depth Z the v_x column -1/Z and the w_y column -(1 + x^2) of L become parallel as the spread of x over the features
shrinks, and so do v_y and w_x: a long focal length or a cluster of features in one corner squares into the Gram matrix that LDL^T
factors.  The families:

  focal_flat      grid 14, 24 random tokens, depth 600 mm everywhere, f_x = f_y swept geometrically from 200 to 6e5 px (four points
                  per decade, eight per decade from 1e3 to 3e4, where the hand-off lies)
  focal_tilted    the same tokens under a depth plane that rises by 1, 5 and 20 % across the image along u and falls as much along v,
                  at five focal lengths: how fast the degeneracy lifts (from 5 % on the ratio stays above 2e-4 at any focal length)
  cluster         grid 32, random intrinsics, flat depth; the current tokens are all of a k x k window in a corner and all of one at
                  the centre, k = 16, 8, 5, 4, 3, 2 (k^2 pairs): the one-corner selection (off the axis the x^2 term keeps a corner
                  window better conditioned than the same window at the centre)
  collinear       grid 17, the depth pattern; 16 tokens of one grid row and one token j = 8, 4, 2, 1 patches off it (with varied
                  depth a line of features is not degenerate: the ratio is 2e-3 to 4e-3 at every j; the family is the control)
  many_rows       focal_flat's construction with 65 pairs on a handle of 80 rows (L in the global workspace, Jacobi's lanes over
                  several rows), at the sweep's focal lengths nearest the threshold on either side
  weighted        the same with 24 pairs and robust_law = 1 and 4: the hand-off is decided on the WEIGHTED Gram matrix and Jacobi
                  runs on sqrt(w) L; the focal lengths are chosen on the reference's weighted system
  rig             (RIG_CASES) two cameras of focal_flat rows with tokens of their own under the extrinsics of law_support, the
                  focal length nearest the threshold on either side for the STACK, through vitvs_op_rig_law

tests/test_solve_host.py asserts on the CPU what makes these a test of the hand-off; tests/test_gpu_solve_handoff.py runs them."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import vitvs_amd  # noqa: F401
from vitvs_amd import config, synth
import law_support as ls
import rig_ref as rg
import robust_ref as rr
import solve_ref as sv

GUARD = 2.0                      # no case's pivot ratio lies within this factor of the threshold
FLAT_MM = 600
TILTS = (0.01, 0.05, 0.20)
TILTED_FOCALS = (600.0, 1100.0, 6000.0, 20000.0, 200000.0)
CLUSTER_SIDES = (16, 8, 5, 4, 3, 2)
COLLINEAR_OFFSETS = (8, 4, 2, 1)
# The pivot ratio of focal_flat falls as f^-4, a factor 3.1 per point at eight per decade, and the guard band is a factor 4 wide: a
# point of the sweep always lands in it.  The sweep leaves out the points in this open interval; chosen for THRESHOLD = 1e-4, where
# two do (1.9e-4 at 1480 px, 6.1e-5 at 1970 px).
FOCAL_GAP = (1.4e3, 2.1e3)


def focal_sweep(lo=200.0, hi=6e5, fine=(1e3, 3e4)) -> list:
    """A geometric sweep from lo to hi, both included: the whole number of steps nearest four per decade, and the points half
    way between them inside ``fine`` (eight per decade there)."""
    steps = max(1, round(4 * np.log10(hi / lo)))
    out = []
    for k in range(2 * steps + 1):
        f = float(lo * (hi / lo) ** (k / (2 * steps)))
        if k % 2 == 0 or fine[0] <= f <= fine[1]:
            out.append(f)
    return out


@dataclasses.dataclass(frozen=True, eq=False)
class Case:
    name: str
    family: str
    g: int
    max_rows: int            # of the tiny handle
    current: tuple           # the designed current tokens
    seed: int                # of the displacements and the intrinsics
    depth: tuple             # ("flat",), ("tilt", share) or ("pattern",)
    focal: float | None      # replaces f_x = f_y of the random intrinsics
    robust: int = 0          # option robust_law

    @property
    def num_pairs(self) -> int:
        return len(self.current)

    @property
    def img(self) -> int:
        return 16 * self.g


def params_of(g: int) -> config.ServoParams:
    return config.ServoParams(dino_input_size=16 * g)          # TinyEngines.fetch's


@functools.lru_cache(maxsize=None)
def depth_image(key: tuple) -> np.ndarray:
    p = params_of(14)
    if key[0] == "pattern":
        return synth.depth_pattern()
    tilt = 0.0 if key[0] == "flat" else key[1]
    v, u = np.meshgrid(np.arange(p.v_max, dtype=np.float64), np.arange(p.u_max, dtype=np.float64), indexing="ij")
    z = FLAT_MM * (1.0 + tilt * (u / p.u_max - 0.5) - tilt * (v / p.v_max - 0.5))
    return np.round(z).astype(np.uint16)


@functools.lru_cache(maxsize=None)
def _tables_cached(g: int, current: tuple, seed: int):
    """(nn_1, nn_2, goal ids, K): every current token is the match of a goal token -2 .. 2 patches away (clipped, all distinct, not
    all in place); every other token matches itself; nn_2 inverts nn_1 where it can, so that some but not all tokens are mutual."""
    t = g * g
    rng = np.random.default_rng(seed)
    K = ls.intrinsics(rng, params_of(g))
    cur = np.asarray(current, np.int64)
    shifts = [(dr, dc) for dr in range(-2, 3) for dc in range(-2, 3)]
    for _ in range(1000):
        taken, ids = set(), []
        for c in cur.tolist():          # the first free one of the 25 displaced tokens, in a random order
            for s in rng.permutation(25):
                i = int(np.clip(c // g + shifts[s][0], 0, g - 1) * g + np.clip(c % g + shifts[s][1], 0, g - 1))
                if i not in taken:
                    break
            else:
                break
            taken.add(i)
            ids.append(i)
        ids = np.array(ids, np.int64)
        if len(ids) == len(cur) and np.count_nonzero(ids != cur) >= len(ids) // 2:
            break
    else:
        raise AssertionError("no distinct displaced goal tokens")
    nn1 = np.arange(t)
    nn1[ids] = cur
    nn2 = np.zeros(t, np.int64)
    nn2[nn1] = np.arange(t)
    assert 0 < np.count_nonzero(nn2[nn1] == np.arange(t)) < t
    return nn1, nn2, ids.astype(np.int32), K


def tables(c: Case):
    nn1, nn2, ids, K = _tables_cached(c.g, c.current, c.seed)
    if c.focal is not None:
        K = (c.focal, c.focal, K[2], K[3])
    return nn1, nn2, np.full(c.g * c.g, 0.5, np.float32), ids, K


def _system(c: Case) -> dict:
    nn1, _, _, ids, K = tables(c)
    p = params_of(c.g)
    s_star, s_, ref = ls.oracle(c.g, c.img, p, nn1, ids, c.num_pairs, depth_image(c.depth), K)
    L, e = ref["L"], ref["e"][:, 0]
    out = dict(s_star=s_star, s_=s_, ref=ref, L=L, e=e, w=np.ones(c.num_pairs), params=p, K=K)
    if c.robust:
        out["w"] = rr.robust_velocity(L, e, p.lambda_, c.robust, ls.s_min(p, c.img, K))["w"]
    sw = np.sqrt(np.repeat(out["w"], 2))
    out.update(Ls=sw[:, None] * L, es=sw * e)      # the system the final solve sees
    return out


@functools.lru_cache(maxsize=None)
def _system_cached(name: str) -> dict:
    return _system(BY_NAME[name])


def system(c: Case) -> dict:
    """The oracle's law of a case: s_star, s_, ref (servo_ref.velocity), L, e, the reference's final weights w, and (Ls, es) =
    sqrt(w) (L, e), the system of the final solve."""
    return _system_cached(c.name)


def straddle(make, focals):
    """(above, below): of ``focals`` the two whose systems ``make(f) -> L`` have the pivot ratios nearest the threshold on either
    side, outside the guard band."""
    ratios = [(sv.pivot_ratio(make(f)), f) for f in focals]
    above = min((r, f) for r, f in ratios if r >= GUARD * sv.THRESHOLD)
    below = max((r, f) for r, f in ratios if r <= sv.THRESHOLD / GUARD)
    return above[1], below[1]


def _random_tokens(g: int, n: int, seed: int) -> tuple:
    return tuple(int(x) for x in np.random.default_rng(seed).choice(g * g, size=n, replace=False))


def _window(g: int, k: int, r0: int, c0: int) -> tuple:
    return tuple((r0 + r) * g + c0 + c for r in range(k) for c in range(k))


def _fname(f: float) -> str:
    return f"{f:.3g}"


def _cases() -> list:
    out = []
    flat24 = _random_tokens(14, 24, 101)
    for f in focal_sweep():
        if not FOCAL_GAP[0] < f < FOCAL_GAP[1]:
            out.append(_focal_case("focal_flat", f))
    for tilt in TILTS:
        for f in TILTED_FOCALS:
            out.append(Case(f"focal_tilted-{round(100 * tilt)}pc-{_fname(f)}", "focal_tilted", 14, 24, flat24, 102, ("tilt", tilt), f))
    for k in CLUSTER_SIDES:
        for where, at in (("corner", 0), ("centre", (32 - k) // 2)):
            # the random intrinsics move the ratio by an order of magnitude: the first seed that keeps it out of the guard band
            for seed in range(200 + k, 1200, 100):
                c = Case(f"cluster-{where}-{k}", "cluster", 32, 256, _window(32, k, at, at), seed, ("flat",), None)
                if not sv.THRESHOLD / GUARD < sv.pivot_ratio(_system(c)["L"]) < sv.THRESHOLD * GUARD:
                    break
            out.append(c)
    for j in COLLINEAR_OFFSETS:
        row = tuple(8 * 17 + c for c in range(16)) + ((8 + j) * 17 + 7,)
        out.append(Case(f"collinear-{j}", "collinear", 17, 24, row, 300 + j, ("pattern",), None))
    for what in ("many_rows", "weighted-1", "weighted-4"):
        for f in straddle(lambda f: _system(_focal_case(what, f))["Ls"], FINE_SWEEP):      # noqa: B023
            out.append(_focal_case(what, f))
    return out


FINE_SWEEP = focal_sweep(fine=(200.0, 6e5))          # eight focal lengths per decade all the way


def _focal_case(what: str, f: float) -> Case:
    """focal_flat's construction at focal length f: with its 24 tokens, with 65 (many_rows) or under robust_law = 1 or 4."""
    tokens, seed, rows, robust = {"focal_flat": (_random_tokens(14, 24, 101), 102, 24, 0),
                                  "many_rows": (_random_tokens(14, 65, 103), 104, 80, 0),
                                  "weighted-1": (_random_tokens(14, 24, 101), 102, 24, 1),
                                  "weighted-4": (_random_tokens(14, 24, 101), 102, 24, 4)}[what]
    return Case(f"{what}-{_fname(f)}", what.split("-")[0], 14, rows, tokens, seed, ("flat",), f, robust)


def threshold_sweep():
    """(name, L, e) of the sweep the threshold is chosen from: the focal_flat, many_rows and weighted constructions
    at eight focal lengths per decade from 200 to 6e5 px, whatever side of the threshold they fall on."""
    for f in FINE_SWEEP:
        for what in ("focal_flat", "many_rows", "weighted-1", "weighted-4"):
            c = _focal_case(what, f)
            s = _system(c)
            yield c.name, s["Ls"], s["es"]


BY_NAME: dict = {}
CASES = _cases()
BY_NAME.update({c.name: c for c in CASES})
assert len(BY_NAME) == len(CASES)


# ----------------------------------------------------------------------------- the rig
def _rig_case(f: float) -> dict:
    """Two cameras, 24 focal_flat pairs each with tokens of their own, under law_support's extrinsics."""
    cams = [Case("rig-camera-0", "rig", 14, 24, _random_tokens(14, 24, 105), 106, ("flat",), f),
            Case("rig-camera-1", "rig", 14, 24, _random_tokens(14, 24, 107), 108, ("flat",), f)]
    systems = [_system(c) for c in cams]
    Ws = [rg.twist_matrix(R, t) for R, t in ls.extrinsics(n=2)]
    return dict(Ls=[s["L"] for s in systems], es=[s["e"] for s in systems], Ws=Ws, ld=48, lam=systems[0]["params"].lambda_)


def _rig_cases() -> dict:
    # (two viewpoints lift part of one camera's degeneracy: the stack's ratio falls more slowly than a camera's, and levels off near
    # 2e-8 from 1e6 to 6e6 px: a longer sweep finds both sides of any threshold down to 1e-9)
    fine = focal_sweep(hi=1e8, fine=(200.0, 1e8))
    stack = lambda f: rg.stacked(*[_rig_case(f)[k] for k in ("Ls", "es", "Ws")], [0, 0])[0]  # noqa: E731
    return {f"rig-{_fname(f)}": _rig_case(f) for f in straddle(stack, fine)}


RIG_CASES = _rig_cases()


def rig_system(case: dict):
    """(M, e) of a rig case: the stack the rig law solves."""
    return rg.stacked(case["Ls"], case["es"], case["Ws"], [0, 0])
