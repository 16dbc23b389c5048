"""Test infrastructure: the camera geometries the control law is tested at besides 640 x 480, and what makes each one a case.

The law maps a token to a camera pixel (oracle/servo_ref.py ``patch_centres`` + ``calculate_uv``: an fp32 patch centre times the
fp64 ratio ``u_max / S``, rounded half to even) and reads the depth image there.  The code states that map five times (servo.hip
``token_pixel``, ``refined_pixel`` and ``goal_depth_kernel``, api.hip's host-side depth sites and the patch pitches behind
``sigma_min``); at 640 x 480 no product is a rounding tie, no pixel falls outside the image and pixel (0, 0) is no patch centre,
so a wrong rounding rule, another order of the fp64 operations or a wrong bounds test cannot show there.  Each geometry below is
chosen, on the reference alone, so that one of them does; tests/test_geometry_host.py pins those properties, and
tests/test_gpu_geometry.py runs the device at them.

Like tests/robust_ref.py this is a reference's helper, never shipped."""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import config
from oracle import servo_ref as sr
import law_support as ls
import robust_ref as rr

# name: (grid, patch, u_max, v_max); the extractor's input side is grid * patch
GEOMETRIES = {
    "ties14": (14, 16, 350, 238),       # every product centre * scale is an exact rounding tie, on both axes (T = 196: prefetched depth)
    "ties17": (17, 16, 357, 255),       # the same at T = 289 > 256: direct depth reads
    "near308": (22, 14, 638, 462),      # dinov2's 308 / 14: 638 / 308 is no binary fraction, so the order of the fp64 operations shows
    "tiny": (14, 16, 13, 9),            # last row and column outside the image, shared pixels, pixel (0, 0) a patch centre
    "tiny17": (17, 16, 13, 9),          # the same on the direct depth path
    "portrait": (14, 16, 480, 640),     # pitch_v > pitch_u
    "hd": (14, 16, 1920, 1080),         # linear pixel indices above 2^16 * 16
    "base": (14, 16, 640, 480),         # the control: no ties, nothing outside
}
NEAR = 1e-9       # a product within this of a tie, and not on it, is a near tie


@dataclasses.dataclass(frozen=True)
class Geometry:
    name: str
    grid: int
    patch: int
    u_max: int
    v_max: int

    @property
    def img(self) -> int:
        return self.grid * self.patch

    @property
    def tokens(self) -> int:
        return self.grid * self.grid

    def params(self, **kw) -> config.ServoParams:
        return config.ServoParams(u_max=self.u_max, v_max=self.v_max, dino_input_size=self.img, **kw)

    def vit_config(self) -> config.ViTConfig:
        """The weight-less tiny configuration of tests/law_support.tiny_cfg, for this patch size."""
        base = config.vit_config("dino_vits16" if self.patch == 16 else "dinov2_vits14", self.img)
        assert base.patch == self.patch and base.grid == self.grid
        return dataclasses.replace(base, dim=128, depth=2, heads=2, layer=1, native_grid=base.grid)


def geometry(name: str) -> Geometry:
    return Geometry(name, *GEOMETRIES[name])


# ----------------------------------------------------------------------------- the map, one axis at a time
def centres(geo: Geometry) -> np.ndarray:
    """The fp32 patch centres of grid indices 0 .. grid - 1 as fp64 values (what ``calculate_uv`` multiplies)."""
    idx = torch.arange(geo.grid).reshape(-1, 1)
    return np.asarray(sr.patch_centres(idx, geo.img, geo.grid), np.float64).reshape(-1)


def products(geo: Geometry, axis: str, order: str = "reference") -> np.ndarray:
    """centre * scale along ``axis`` ("u" or "v"), in the reference's order ``c * (extent / S)`` or as ``c * extent / S``."""
    extent = geo.u_max if axis == "u" else geo.v_max
    c = centres(geo)
    if order == "reference":
        return np.array([x * (extent / geo.img) for x in c])
    assert order == "product_first"
    return np.array([x * extent / geo.img for x in c])


def round_reference(x: np.ndarray) -> np.ndarray:
    return np.array([round(float(v)) for v in x], np.int64)          # Python's round: half to even, as calculate_uv


def round_half_away(x: np.ndarray) -> np.ndarray:
    return np.floor(np.asarray(x) + 0.5).astype(np.int64)            # C's round() on the non-negative products of the map


def exact_ties(x: np.ndarray) -> np.ndarray:
    return (np.asarray(x) - np.floor(x)) == 0.5


def near_ties(x: np.ndarray) -> np.ndarray:
    d = np.abs((np.asarray(x) - np.floor(x)) - 0.5)
    return (d < NEAR) & (d != 0.0)


def token_pixels(geo: Geometry, ids=None) -> np.ndarray:
    """(u, v) of tokens' patch centres through the oracle (all tokens unless ``ids``)."""
    ids = np.arange(geo.tokens) if ids is None else ids
    return rr.token_pixels(ids, geo.grid, geo.img, geo.u_max, geo.v_max)


def outside(geo: Geometry, uv: np.ndarray) -> np.ndarray:
    """Rows of ``uv`` that get_depth reads as 100 m because they lie outside the image."""
    uv = np.asarray(uv)
    return (uv[:, 0] < 0) | (uv[:, 0] >= geo.u_max) | (uv[:, 1] < 0) | (uv[:, 1] >= geo.v_max)


# ----------------------------------------------------------------------------- depth images
def depth_image(geo: Geometry, rng=None, level: int = 0) -> np.ndarray:
    """uint16 millimetres [v_max, u_max]: synth.depth_pattern's ripple (shifted by ``level`` mm) with random holes when a generator
    is given, and NO hole on the image's border: pixel (0, 0), which a zero-padded row reads, the first column, which a read one
    past the end of a row would land on, and the last row and column are all depths, so that none of them can be mistaken for the
    100 m a hole or a pixel outside the image gives."""
    v, u = np.meshgrid(np.arange(geo.v_max, dtype=np.int64), np.arange(geo.u_max, dtype=np.int64), indexing="ij")
    z = (560 + level + (u * 7 + v * 13) % 101).astype(np.uint16)
    d = z.copy()
    if rng is not None:
        d.reshape(-1)[rng.integers(0, d.size, size=d.size // 7)] = 0
    for border in (np.s_[0, :], np.s_[-1, :], np.s_[:, 0], np.s_[:, -1]):
        d[border] = z[border]
    assert d[0, 0] != 0 and d[-1].all() and d[:, -1].all() and d[:, 0].all()
    return d


def intrinsics(geo: Geometry, rng=None, square: bool = False):
    """(fx, fy, cx, cy) in proportion to the image: focal lengths 0.6 .. 1.1 image widths (``square``: f_x = f_y), the principal
    point within 3 % of the centre."""
    rng = rng if rng is not None else np.random.default_rng(0)
    fx = float(rng.uniform(0.6, 1.1)) * geo.u_max
    fy = fx if square else float(rng.uniform(0.6, 1.1)) * geo.u_max
    return (fx, fy, geo.u_max / 2 + float(rng.uniform(-0.03, 0.03)) * geo.u_max, geo.v_max / 2 + float(rng.uniform(-0.03, 0.03)) * geo.v_max)


# ----------------------------------------------------------------------------- the law on random tables
TABLE_MODES = ("order", "dense", "explicit", "padded", "too_few")
PAIRS, LIVE = 24, 6       # the law's pairs; the ids of the "padded" mode, whose other PAIRS - LIVE rows are zero padding


def table_case(name: str, mode: str) -> dict:
    """Random arg-max tables (law_support.tables), a depth image without holes on its border and random intrinsics at a geometry,
    the selection of ``mode`` and the oracle's law on it: ORDER and EXPLICIT with PAIRS ids, DENSE (every mutual token), "padded"
    (EXPLICIT with LIVE of PAIRS ids: the other rows are pairs at pixel (0, 0), which read depth[0, 0]) and "too_few" (3 ids)."""
    geo = geometry(name)
    params, t, k = geo.params(), geo.tokens, PAIRS
    rng = np.random.default_rng(9000 + 10 * list(GEOMETRIES).index(name) + TABLE_MODES.index(mode))
    nn1, nn2, sim1, mutual = ls.tables(rng, t, int(rng.integers(t // 4, t // 2)))
    depth, K = depth_image(geo, rng), intrinsics(geo, rng)
    order = None
    if mode == "order":
        order = rng.permutation(t).astype(np.int32)
        mset = set(mutual.tolist())
        ids, rows = np.array([x for x in order if x in mset][:k], np.int32), k
    elif mode == "dense":
        ids, rows = mutual.astype(np.int32), len(mutual)
    else:
        n = {"explicit": k, "padded": LIVE, "too_few": 3}[mode]
        ids, rows = rng.choice(t, size=n, replace=False).astype(np.int32), k          # any tokens, mutual or not
        matched_outside = np.nonzero(outside(geo, token_pixels(geo, nn1)))[0]           # tokens whose match lies outside the image
        if mode == "padded" and len(matched_outside) and not np.isin(ids, matched_outside).any():
            ids[0] = matched_outside[0]                                                 # (tiny: six random ids can miss them all)
    s_star, s_, ref = ls.oracle(geo.grid, geo.img, params, nn1, ids, rows, depth, K)
    return dict(geo=geo, params=params, nn_1=nn1, nn_2=nn2, sim_1=sim1, mutual=mutual, depth=depth, K=K, order=order, ids=ids, rows=rows,
                s_star=s_star, s_uv=s_, ref=ref)


def goal_case(name: str, interaction: str) -> dict:
    """For the goal-depth table: tables, depth, a goal depth image and intrinsics at a geometry, and two EXPLICIT selections: every
    token once in a random order (T rows: every entry of the table below T is read, the tokens outside the image included) and
    LIVE of PAIRS ids (padded rows: entry T)."""
    geo = geometry(name)
    params, t = geo.params(), geo.tokens
    rng = np.random.default_rng(9500 + 10 * list(GEOMETRIES).index(name) + ("desired", "mean").index(interaction))
    nn1, nn2, sim1, mutual = ls.tables(rng, t, int(rng.integers(t // 4, t // 2)))
    return dict(geo=geo, params=params, nn_1=nn1, nn_2=nn2, sim_1=sim1, depth=depth_image(geo, rng), goal_depth=depth_image(geo, rng, level=137),
                K=intrinsics(geo, rng), every=rng.permutation(t).astype(np.int32), few=rng.choice(t, size=LIVE, replace=False).astype(np.int32))


def features(geo: Geometry, nn1, ids, rows):
    """(s_uv*, s_uv) of a selection through the oracle (zero padding up to ``rows``)."""
    ids = np.asarray(ids, np.int64)
    p1 = torch.from_numpy(np.stack([ids // geo.grid, ids % geo.grid], 1))
    p2 = torch.from_numpy(np.stack([nn1[ids] // geo.grid, nn1[ids] % geo.grid], 1))
    s_star, s_ = sr.calculate_uv(sr.patch_centres(p1, geo.img, geo.grid), sr.patch_centres(p2, geo.img, geo.grid), rows, geo.u_max,
                                 geo.v_max, geo.img)
    return np.asarray(s_star), np.asarray(s_)


BORDER_GEOMETRIES = ("base", "ties14")


def border_case(name: str) -> dict:
    """Sub-patch offsets at the image border: tables at a geometry, PAIRS ids whose matches lie in the last column, the last row, the
    first column and the first row (six of each, corners included as they come), the offset table that moves those matches half a
    pitch outwards, and the reference's refined features and law (tests/refine_ref.py)."""
    import refine_ref as rf
    geo = geometry(name)
    params, t, g = geo.params(), geo.tokens, geo.grid
    rng = np.random.default_rng(9800 + list(GEOMETRIES).index(name))
    nn1, nn2, sim1, _ = ls.tables(rng, t, int(rng.integers(t // 4, t // 2)))
    depth, K = depth_image(geo, rng), intrinsics(geo, rng)
    r, c = nn1 // g, nn1 % g
    ids = []
    for where in (c == g - 1, r == g - 1, c == 0, r == 0):
        pool = [i for i in np.nonzero(where)[0] if i not in ids]
        ids += [int(i) for i in rng.choice(pool, size=PAIRS // 4, replace=False)]
    ids = np.array(ids, np.int32)
    table = border_offsets(geo, nn1)
    s_star, s_ = rf.refined_features(ids, nn1, table, geo.img, g, geo.u_max, geo.v_max, rows=PAIRS)
    s_star, s_ = np.asarray(s_star), np.asarray(s_)
    return dict(geo=geo, params=params, nn_1=nn1, nn_2=nn2, sim_1=sim1, depth=depth, K=K, ids=ids, offsets=table, s_star=s_star, s_uv=s_,
                ref=rf.velocity(s_star, s_, depth, K, params.lambda_))


# ----------------------------------------------------------------------------- cases of the laws that read the patch pitches
ROBUST_ITERATIONS = 2
# case: (geometry, seed, f_x == f_y).  The seeds are chosen on the reference: tests/test_geometry_host.py says for what.  With
# f_x = f_y, sigma_min is half the LARGER pitch over f, so exchanging the pitches cannot show; "portrait_fxfy" is there for that.
ROBUST_CASES = {"portrait": ("portrait", 8101, True), "tiny": ("tiny", 8117, True), "hd": ("hd", 8102, True),
                "portrait_fxfy": ("portrait", 8300, False)}
LAW_SEED = 8209                                                    # the homography case on "portrait"
POSE_SEED = 8423                                                   # the pose case on "portrait" (pose_case)
LAW_ITERATIONS = 4


def pitch_sigma_min(geo: Geometry, K, swapped: bool = False) -> float:
    """sigma_min of the robust law at ``geo``; ``swapped``: with pitch_u and pitch_v exchanged, the mistake the cases are there for."""
    u, v = (geo.v_max, geo.u_max) if swapped else (geo.u_max, geo.v_max)
    return rr.sigma_min(geo.patch, u, v, geo.img, K[0], K[1])


def robust_case(name: str, num_pairs: int = 24) -> dict:
    """A planted-outlier scenario of ROBUST_CASES, the oracle's plain law on it and the robust law (N = 2) with the geometry's
    sigma_min (``rob``) and with three wrong ones: the pitches exchanged (``swapped``), pitch_u alone (``u_only``, what is right at
    640 x 480 with f_x = f_y) and no floor at all (``no_floor``)."""
    geo_name, seed, square = ROBUST_CASES[name]
    geo = geometry(geo_name)
    params = geo.params()
    rng = np.random.default_rng(seed)
    K = intrinsics(geo, rng, square=square)
    sc = rr.planted_scenario(rng, num_pairs, 0.125, params, K=K, g=geo.grid, holes=True)
    s_star, s_, ref = rr.oracle_law(sc, params)
    floors = dict(rob=pitch_sigma_min(geo, K), swapped=pitch_sigma_min(geo, K, True), u_only=0.5 * geo.patch * geo.u_max / geo.img / K[0],
                  no_floor=0.0)
    with np.errstate(divide="ignore", invalid="ignore"):                  # (no floor: a zero median divides by zero)
        laws = {k: rr.robust_velocity(ref["L"], ref["e"], params.lambda_, ROBUST_ITERATIONS, s) for k, s in floors.items()}
    return dict(geo=geo, params=params, sc=sc, s_star=s_star, s_uv=s_, ref=ref, s_min=floors["rob"], **laws)


def law_case(name: str = "portrait", num_pairs: int = 24, seed: int = LAW_SEED, plane_goal: bool = False) -> dict:
    """A planted-outlier scenario and a goal depth image at a geometry, for the pose and the homography law.  ``plane_goal``: the
    goal depth image is the scenario's own plane as the goal camera sees it (``plane_goal_depth``), so the inliers' 3-D points at
    the two poses differ by one rigid motion up to the patch quantisation, and the pose law's floor sigma_min, which is that
    quantisation's size, takes part; otherwise depth_image's ripple, which no rigid motion explains."""
    geo = geometry(name)
    params = geo.params()
    rng = np.random.default_rng(seed)
    sc = rr.planted_scenario(rng, num_pairs, 0.125, params, K=intrinsics(geo, rng), g=geo.grid, holes=True)
    return dict(geo=geo, params=params, sc=sc, goal_depth=plane_goal_depth(geo) if plane_goal else depth_image(geo, rng, level=137))


def plane_goal_depth(geo: Geometry, plane_z: float = 0.61) -> np.ndarray:
    """The goal camera's uint16 millimetre depth image of rr.planted_scenario's plane: it faces that camera at ``plane_z``, so every
    pixel reads plane_z, here with a ripple of +-3 mm (far below the floor) so that a wrong entry of the goal-depth table shows."""
    v, u = np.meshgrid(np.arange(geo.v_max, dtype=np.int64), np.arange(geo.u_max, dtype=np.int64), indexing="ij")
    return (round(plane_z * 1000.0) - 3 + (u * 7 + v * 13) % 7).astype(np.uint16)


def pose_case() -> dict:
    """The pose law's case on "portrait": its floor is reached, so the pitches decide the twist (tests/test_geometry_host.py)."""
    return law_case("portrait", seed=POSE_SEED, plane_goal=True)


def oracle_details(case: dict, rows: int) -> dict:
    """What ``Engine.last_details`` holds after the plain law on a case's scenario, as far as the follow-on laws' references read it
    (selected, s_uv, feat, info), from the oracle alone: the host test chooses the cases with it, the device test compares it."""
    sc, params = case["sc"], case["params"]
    s_star, s_, ref = rr.oracle_law(sc, params)
    n = len(sc["ids"])
    selected = np.full((1, rows), -1, np.int32)
    selected[0, :n] = sc["ids"]
    s_uv = np.zeros((1, rows, 4), np.int32)
    s_uv[0, :n, 0:2], s_uv[0, :n, 2:4] = s_star, s_
    feat = np.zeros((1, rows, 4))
    feat[0, :n, 0], feat[0, :n, 1:3], feat[0, :n, 3] = ref["Z"][:, 0], ref["s_xy"], sc["sim_1"][sc["ids"]]
    info = np.zeros((1, 8), np.int32)
    info[0, 1] = info[0, 3] = n
    return dict(selected=selected, s_uv=s_uv, feat=feat, info=info)


def swapped_pitches(pitches):
    return pitches[1], pitches[0]


# ----------------------------------------------------------------------------- sub-patch offsets at the border
def border_offsets(geo: Geometry, nn1: np.ndarray) -> np.ndarray:
    """The offset table [T, 2] = (dr, dc), indexed by goal token, that moves every match in the last row or column half a pitch
    outwards (+0.5) and every match in the first row or column half a pitch outwards (-0.5); 0 elsewhere."""
    g = geo.grid
    j = np.asarray(nn1, np.int64)
    table = np.zeros((geo.tokens, 2), np.float32)
    for axis, coord in enumerate((j // g, j % g)):
        table[coord == g - 1, axis] = 0.5
        table[coord == 0, axis] = -0.5
    return table
