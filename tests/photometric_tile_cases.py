"""Test infrastructure (never shipped): the inputs the tile photometric law's tests share.

"shadow": the disturbance of the closed loops, applied to every current frame: g = 0.6 where xx + 0.5 yy < 380 (pixel column and
row at 640 x 480), else 1; cur = clip(round(g rgb)).  About 45 % of the view behind a slanted edge, nothing saturates.

The op cases are small crops of test_gpu_photometric_robust_op.py's scene pair (640 x 480, a start 0.3 cm / 0.4 degrees from the
goal), half of each crop shaded by the 0.6 factor across a slanted edge through the crop's centre (in the crop's own normalised
coordinates, so that the 1042 x 16 crop is cut too).  The crop origins come from a search on the CPU over a grid of them (29 rows by
31 columns apart) for a reference with status OK, its half count at least 3 rows inside its median bin in every re-weighting
(margin_m), and then the fewest dead tiles: a texel of the scene is about a dozen pixels wide, so the tiles of a small crop are
often flat, and at level 2 most of them are.  That is the law's answer to such a crop, on both sides alike."""
import functools

import numpy as np

from vitvs_amd import config, synth
import photometric_tile_ref as tr
from planar_sim import PlanarScene, rodrigues

MU, LAM, SMIN = 0.01, 0.5, 0.01
PARAMS = config.ServoParams(dino_input_size=224, use_feature_binning=False)
START_CM, START_DEG = 0.3, 0.4


def shadow(rgb, factor=0.6, edge=380.0):
    """The closed loops' disturbance at the frame's own size."""
    yy, xx = np.mgrid[:rgb.shape[0], :rgb.shape[1]]
    g = np.where(xx + 0.5 * yy < edge, factor, 1.0)
    return np.clip(np.round(g[..., None] * rgb.astype(np.float64)), 0, 255).astype(np.uint8)


def shade_crop(rgb, factor=0.6):
    """Half of a crop behind a slanted edge through its centre."""
    H, W = rgb.shape[:2]
    yy, xx = np.mgrid[:H, :W]
    g = np.where((xx + 0.5 - W / 2) / W + 0.5 * (yy + 0.5 - H / 2) / H < 0, factor, 1.0)
    return np.clip(np.round(g[..., None] * rgb.astype(np.float64)), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def scene_pair():
    """(current frame, goal frame, goal depth) at 640 x 480, rendered on the CPU."""
    sc = PlanarScene(synth.texture(128, 11), 1.6 / 128, PARAMS, plane_z=0.61, device="cpu")
    goal_rgb, goal_depth = sc.render(np.eye(3), np.zeros(3))
    axis, direction = np.array([0.3, -0.4, 0.85]), np.array([0.6, -0.5, 0.6])
    rgb, _ = sc.render(rodrigues(axis / np.linalg.norm(axis) * np.deg2rad(START_DEG)),
                       direction / np.linalg.norm(direction) * START_CM / 100)
    return rgb, goal_rgb, goal_depth


# name: (H, W, level, (tiles_y, tiles_x), the crop's first row and column, depth: "z" / "holes" / "scalar", interaction, flat patch
# (pixel rows and columns of BOTH frames set to one grey, or None)).
CASES = {
    "24x32-l0-2x2": (24, 32, 0, (2, 2), 165, 520, "z", 1, None),
    "24x32-l0-3x5": (24, 32, 0, (3, 5), 49, 334, "z", 1, None),         # tile edges that do not divide the sides
    "23x29-l0-4x4": (23, 29, 0, (4, 4), 78, 303, "z", 0, None),         # odd sides, the narrow loads
    "48x64-l2-4x4-holes": (48, 64, 2, (4, 4), 165, 551, "holes", 1, None),
    "48x64-l2-8x8": (48, 64, 2, (8, 8), 165, 427, "z", 1, None),         # the most tiles
    "70x32-l0-8x2": (70, 32, 0, (8, 2), 136, 55, "z", 1, None),         # 9 bands per tile row: past the solve's 8 partials in flight
    "1042x16-l1-3x1": (1042, 16, 1, (3, 1), 0, 324, "z", 1, None),       # pooled 521 rows in two-row bands; the tile rows begin at the even
                                                                         # rows 174 and 348, where bands begin too: no band is cut
    "1042x16-l1-4x1": (1042, 16, 1, (4, 1), 0, 594, "z", 1, None),       # the tile rows begin at 131, 261 and 391: the bands of rows
                                                                         # 130 / 131, 260 / 261 and 390 / 391 lie across a tile-row edge
    "24x32-l0-rgb-2x2": (24, 32, 0, (2, 2), 136, 551, "scalar", 0, None),
    "48x64-l2-4x4-flat": (48, 64, 2, (4, 4), 165, 551, "z", 1, (12, 24, 16, 32)),    # tile (1, 1) is flat: dead
    "24x8-l0-2x8": (24, 8, 0, (2, 8), 107, 458, "z", 1, None),           # gx = pooled w: the border-only tile columns are dead
}


def case(name):
    return CASES[name]


def build(name, y0=None, x0=None):
    """(cur, des, Z or None, depth_scale, K) of a case (at another origin: the search's)."""
    H, W, level, _, cy0, cx0, depth, _, flat = case(name)
    y0, x0 = cy0 if y0 is None else y0, cx0 if x0 is None else x0
    rgb, goal, gdepth = scene_pair()

    def cut(img):
        img = img[y0:, x0:]
        while img.shape[0] < H:                                  # more rows than the scene has: the image and its first rows again
            img = np.concatenate([img, img[:H - img.shape[0]]])
        return np.ascontiguousarray(img[:H, :W])
    fx, fy, cx, cy = PARAMS.intrinsics()
    K = (fx, fy, cx - x0, cy - y0)
    cur, des, Z = shade_crop(cut(rgb)), cut(goal), cut(gdepth)
    if flat is not None:
        ya, yb, xa, xb = flat
        des = des.copy()
        des[ya:yb, xa:xb] = 90
        cur[ya:yb, xa:xb] = 90
    if depth == "holes":
        Z = Z.copy()
        Z[8:20, 24:36] = 0                                       # nine pooled pixels without a sample
        Z[30, ::3] = 0                                           # and blocks that miss some
    return cur, des, (None if depth == "scalar" else Z), (0.61 if depth == "scalar" else 0.0), K


@functools.lru_cache(maxsize=None)
def fixture(name):
    return build(name)


@functools.lru_cache(maxsize=None)
def reference(name, N, reverse=False, smin=SMIN):
    _, _, level, (gy, gx), _, _, _, inter, _ = case(name)
    cur, des, Z, scalar, K = fixture(name)
    return tr.velocity(cur, des, Z, scalar, K, level, inter, MU, LAM, gy, gx, N, smin, reverse=reverse)
