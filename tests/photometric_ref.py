"""Test infrastructure (never shipped): the photometric law (vit-vs_amd/csrc/photometric.hip) in fp64 numpy.

Per pair: frames uint8 [H, W, 3], an optional depth image uint16 [H, W] in millimetres (0 = hole) that belongs to the image the
gradients are taken of, a scalar depth in metres for the RGB-only case, K = (fx, fy, cx, cy), ``level`` 0 .. 3 (s = 2^level),
``interaction`` 0 (current) / 1 (desired), ``mu`` >= 0 and ``lam``.

  Y = 77 R + 150 G + 29 B (integers), summed over s x s blocks (h = H // s, w = W // s, the tail ignored), I = Ysum / (256 s^2);
  G = I_cur (interaction 0) or I_des (1); gx, gy its central differences; the one-pixel border of the pooled image takes no part;
  Z = mean of the block's non-zero depth samples / 1000 (no sample: a hole, no part), or the scalar everywhere;
  fx' = fx / s, cx' = (cx + 0.5) / s - 0.5, x = (c - cx') / fx', a = gx fx' (y, b likewise);
  L = [a/Z, b/Z, -(x a + y b)/Z, -(x y a + (1 + y^2) b), (1 + x^2) a + x y b, x b - y a],  e = I_cur - I_des;
  the 28 sums: H = sum L^T L (21, upper triangle, row-major), g = sum L^T e (6), c = sum e^2; n = the rows;
  v = -lam (H + mu diag(H))^-1 g by LDL^T under solve.h's pivot rule; TOO_FEW (v = 0) when n < 6 or a pivot fails; NO_DEPTH
  (v = 0) without a depth image and with a scalar <= 0.

The sums are numpy.sum (pairwise) over the rows in row-major order of the pooled image, or over the reverse of it
(``reverse=True``): the distance between the two is the yardstick for a sum in any other order.  (Not one row after the other:
against exactly rounded sums, math.fsum, a running fp64 sum of the 296 721 rows of a 640 x 480 frame at level 0 is off by 2.4e-12 of
sum |term| in the all-positive sum of L5^2, by the SAME amount in either direction, which its distance to its own reverse does not
show; numpy.sum is within 2e-16 of the exact sums there.)  ``abs`` is sum |term| of every sum, for the bound
(n + 16) 2^-53 sum |term| on a sum of n correctly formed terms added in any order."""
import numpy as np

from solve_ref import THRESHOLD

OK, TOO_FEW, NO_DEPTH = 0, 2, 3
TRIU = [(i, j) for i in range(6) for j in range(i, 6)]


def plan(height, width, level, max_pairs=1):
    """vitvs_op_photometric_plan restated: (pooled h, pooled w, rows per band, bands, LDS bytes, workspace bytes)."""
    h, w = height >> level, width >> level
    rows = max(1, min((2048 >> level) // w, h // 256))
    bands = (h + rows - 1) // rows
    lds = ((rows + 2) * w * 2 + rows * w) * 4 + 4 * 32 * 8
    return h, w, rows, bands, lds, max_pairs * bands * 256


def luminance(img):
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    p = img.astype(np.int64)
    return 77 * p[..., 0] + 150 * p[..., 1] + 29 * p[..., 2]


def pooled(img, level):
    """I [h, w] float64: exact, the divisor is a power of two."""
    s = 1 << level
    Y = luminance(img)
    h, w = Y.shape[0] // s, Y.shape[1] // s
    Ysum = Y[:h * s, :w * s].reshape(h, s, w, s).sum(axis=(1, 3))
    return Ysum.astype(np.float64) / (256.0 * s * s)


def pooled_depth(Z_mm, level):
    """(Z [h, w] in metres, NaN in a hole; hole mask)."""
    s = 1 << level
    Z = np.asarray(Z_mm)
    assert Z.dtype == np.uint16 and Z.ndim == 2
    h, w = Z.shape[0] // s, Z.shape[1] // s
    blk = Z[:h * s, :w * s].astype(np.int64).reshape(h, s, w, s)
    total = blk.sum(axis=(1, 3))
    count = (blk != 0).sum(axis=(1, 3))
    hole = count == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        Zm = total.astype(np.float64) / (count.astype(np.float64) * 1000.0)
    Zm[hole] = np.nan
    return Zm, hole


def rows(I_cur, I_des, Z_mm, depth_scale, K, level, interaction):
    """(L [n, 6], e [n], holes, h, w) in row-major order of the pooled image, or None for NO_DEPTH."""
    assert level in (0, 1, 2, 3) and interaction in (0, 1)
    if Z_mm is None and not depth_scale > 0.0:
        return None
    s = float(1 << level)
    fx, fy, cx, cy = (float(k) for k in K)
    Ic, Id = pooled(I_cur, level), pooled(I_des, level)
    h, w = Ic.shape
    assert h >= 3 and w >= 3
    G = Ic if interaction == 0 else Id
    gx = (G[1:-1, 2:] - G[1:-1, :-2]) / 2.0
    gy = (G[2:, 1:-1] - G[:-2, 1:-1]) / 2.0
    if Z_mm is None:
        Z, hole = np.full((h, w), float(depth_scale)), np.zeros((h, w), bool)
    else:
        Z, hole = pooled_depth(Z_mm, level)
    fxp, fyp = fx / s, fy / s
    cxp, cyp = (cx + 0.5) / s - 0.5, (cy + 0.5) / s - 0.5
    r, c = np.meshgrid(np.arange(1, h - 1, dtype=np.float64), np.arange(1, w - 1, dtype=np.float64), indexing="ij")
    x, y = (c - cxp) / fxp, (r - cyp) / fyp
    a, b = gx * fxp, gy * fyp
    Zi, part = Z[1:-1, 1:-1], ~hole[1:-1, 1:-1]
    e = (Ic - Id)[1:-1, 1:-1]
    x, y, a, b, Zi, e = (q[part] for q in (x, y, a, b, Zi, e))       # boolean indexing keeps the row-major order
    L = np.stack([a / Zi, b / Zi, -(x * a + y * b) / Zi, -(x * y * a + (1.0 + y * y) * b), (1.0 + x * x) * a + x * y * b,
                  x * b - y * a], axis=1)
    return L, e, int((~part).sum()), h, w


def _total(terms, reverse):
    if terms.shape[0] == 0:
        return 0.0
    return float(np.sum(np.ascontiguousarray(terms[::-1]) if reverse else terms))


def sums(I_cur, I_des, Z_mm, depth_scale, K, level, interaction, reverse=False):
    """dict(normal [28], abs [28], n, holes, h, w), or None for NO_DEPTH."""
    got = rows(I_cur, I_des, Z_mm, depth_scale, K, level, interaction)
    if got is None:
        return None
    L, e, holes, h, w = got
    terms = [L[:, i] * L[:, j] for i, j in TRIU] + [L[:, i] * e for i in range(6)] + [e * e]
    normal = np.array([_total(t, reverse) for t in terms])
    absum = np.array([_total(np.abs(t), False) for t in terms])
    return dict(normal=normal, abs=absum, n=int(L.shape[0]), holes=holes, h=h, w=w)


def unpack(normal):
    """(H [6, 6] symmetric, g [6], c) of the 28 sums."""
    normal = np.asarray(normal, np.float64).reshape(28)
    H = np.zeros((6, 6))
    for q, (i, j) in enumerate(TRIU):
        H[i, j] = H[j, i] = normal[q]
    return H, normal[21:27].copy(), float(normal[27])


def solve(normal, mu, lam):
    """(v [6], solved): v = -lam (H + mu diag(H))^-1 g by LDL^T in solve.h's order of operations and under its pivot rule
    (every d_j > THRESHOLD G_jj and G_jj > 0); not solved: v = 0."""
    H, g, _ = unpack(normal)
    G = H.copy()
    for i in range(6):
        G[i, i] = H[i, i] + mu * H[i, i]
    Lf, d = np.zeros((6, 6)), np.zeros(6)
    good = True
    with np.errstate(divide="ignore", invalid="ignore"):
        for j in range(6):
            dj = G[j, j] - sum(Lf[j, k] * Lf[j, k] * d[k] for k in range(j))
            good = good and bool(dj > THRESHOLD * G[j, j]) and bool(G[j, j] > 0.0)
            d[j] = dj
            for i in range(j + 1, 6):
                Lf[i, j] = (G[i, j] - sum(Lf[i, k] * Lf[j, k] * d[k] for k in range(j))) * (1.0 / dj)
        if not good:
            return np.zeros(6), False
        y, x = np.zeros(6), np.zeros(6)
        for i in range(6):
            y[i] = g[i] - sum(Lf[i, k] * y[k] for k in range(i))
        for i in range(5, -1, -1):
            x[i] = y[i] * (1.0 / d[i]) - sum(Lf[k, i] * x[k] for k in range(i + 1, 6))
    return -lam * x, True


def velocity(I_cur, I_des, Z_mm, depth_scale, K, level, interaction, mu, lam, reverse=False):
    """dict(v [6], status, normal [28], abs [28], info [8]): info = n, pooled h, pooled w, bands, holes, pivot failed, 0, 0."""
    H_, W_ = np.asarray(I_cur).shape[:2]
    h, w, _, bands, _, _ = plan(H_, W_, level)
    s = sums(I_cur, I_des, Z_mm, depth_scale, K, level, interaction, reverse)
    if s is None:
        return dict(v=np.zeros(6), status=NO_DEPTH, normal=np.zeros(28), abs=np.zeros(28),
                    info=np.array([0, h, w, bands, 0, 0, 0, 0], np.int32))
    v, failed = np.zeros(6), 0
    status = TOO_FEW
    if s["n"] >= 6:
        v, solved = solve(s["normal"], mu, lam)
        failed = 0 if solved else 1
        status = OK if solved else TOO_FEW
    return dict(v=v, status=status, normal=s["normal"], abs=s["abs"],
                info=np.array([s["n"], h, w, bands, s["holes"], failed, 0, 0], np.int32))
