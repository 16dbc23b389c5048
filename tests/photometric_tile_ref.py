"""Test infrastructure (never shipped): the tile photometric law (vit-vs_amd/csrc/photometric.hip) in fp64 numpy, on
photometric_robust_ref's functions.

Rows, L, e, D, holes, n, pooling, intrinsics, the 45 sums, the 2 x 2 C = l d l^T and its pivot rule, the histogram median, sigma,
Tukey's weights and the LM solve are the robust law's.  The lighting model is always on and LOCAL: one (gamma_k, beta_k) per tile of
a ``tiles_y`` x ``tiles_x`` = gy x gx grid (each 1 .. 8, gy <= pooled h, gx <= pooled w) over the pooled image.  The row at pooled
pixel (r, c) belongs to tile k = floor(r gy / h) gx + floor(c gx / w); the one-pixel border counts in the indexing and has no row.

  One solve: per tile in ascending k the 45 weighted sums over the tile's rows in row-major order, C_k factored by _c_factor.  A
  tile whose factor fails (flat, empty, all weights 0) is DEAD in this pass: it adds nothing, gamma_k = beta_k = 0, and its rows
  stay in the next re-weighting with those zeros.  The live tiles add, from zero and in ascending k,
      H' += A_k - B_k C_k^-1 B_k^T,   g' += b_k - B_k C_k^-1 d_k        (solve45's expressions and order per entry)
  x = -(H' + mu diag H')^-1 g' (photometric_ref.solve), (gamma_k, beta_k) = C_k^-1 (d_k + B_k^T x) per live tile.
  One re-weighting: rho = |((e + L.x) - gamma_k D) - beta_k| with the row's own tile's pair, then ONE histogram, median and sigma
  over all rows, and the weights as the robust law's.
  TOO_FEW (everything 0) when n < 6, fewer than 6 rows keep a weight, no tile is live, or the 6 x 6 pivot fails.

With gy = gx = 1 this is photometric_robust_ref.velocity(..., illumination=1) bit for bit (0.0 + t is t).
``reverse=True``: the rows of each tile reversed and the tiles taken in descending order: the yardstick for the device's sums."""
import numpy as np

import photometric_ref as pr
import photometric_robust_ref as rr

OK, TOO_FEW, NO_DEPTH = pr.OK, pr.TOO_FEW, pr.NO_DEPTH


def plan(height, width, level, tiles_y, tiles_x):
    """vitvs_op_photometric_tile_plan restated: (pooled h, pooled w, rows per band, bands, slots, LDS bytes of the rows launch, LDS
    bytes of the residual launch, workspace doubles per pair).  The bands are the plain law's.  A band of more than one row may lie
    across ONE tile-row boundary (rows <= h / 256 and a tile row has at least floor(h / 8) >= 64 rows by then): such a plan gives
    every band two slots, slot s for tile row floor(r0 gy / h) + s, r0 = the band's first row; one-row bands have one slot.  The
    partial of (band, slot, tile column) is 48 doubles at ((band slots + slot) gx + tile column) 48."""
    h, w, rows, bands, _, _ = pr.plan(height, width, level)
    slots = 2 if rows > 1 else 1
    lds = ((rows + 2) * w * 2 + rows * w) * 4 + 4 * 48 * 8
    return h, w, rows, bands, slots, lds, lds + 4096 * 4, bands * slots * tiles_x * 48


def tile_of_rows(shape, Z_mm, level, tiles_y, tiles_x):
    """k [n] of photometric_ref.rows' rows."""
    h, w = shape[0] >> level, shape[1] >> level
    r, c = np.meshgrid(np.arange(1, h - 1), np.arange(1, w - 1), indexing="ij")
    k = (r * tiles_y // h) * tiles_x + c * tiles_x // w
    part = np.ones((h - 2, w - 2), bool) if Z_mm is None else ~pr.pooled_depth(Z_mm, level)[1][1:-1, 1:-1]
    return k[part]


def tile_sums(L, e, D, w, tile, T, reverse=False):
    """(normal [T, 45], abs [T, 45]) of the rows of every tile."""
    normal, absum = np.zeros((T, 45)), np.zeros((T, 45))
    for k in range(T):
        m = tile == k
        normal[k], absum[k] = rr.weighted_sums(L[m], e[m], D[m], w[m], reverse)
    return normal, absum


def solve_tiles(normal, mu, lam, reverse=False):
    """(v [6], x [6], gamma_beta [T, 2], live [T] bool, solved) of the tiles' sums."""
    s = np.asarray(normal, np.float64).reshape(-1, 45)
    T = s.shape[0]
    live, fac = np.zeros(T, bool), [None] * T
    n28 = np.zeros(28)
    order = range(T - 1, -1, -1) if reverse else range(T)
    for k in order:
        A, b, B, C3, dd = s[k, :21], s[k, 21:27], s[k, 28:40].reshape(6, 2), s[k, 40:43], s[k, 43:45]
        l, d0, d1, good = rr._c_factor(C3)
        if not good:
            continue
        live[k], fac[k] = True, (l, d0, d1)
        u = [rr._c_solve(l, d0, d1, B[i, 0], B[i, 1]) for i in range(6)]
        for q, (i, j) in enumerate(pr.TRIU):
            n28[q] = n28[q] + (A[q] - (u[i][0] * B[j, 0] + u[i][1] * B[j, 1]))
        for i in range(6):
            n28[21 + i] = n28[21 + i] + (b[i] - (u[i][0] * dd[0] + u[i][1] * dd[1]))
    gb = np.zeros((T, 2))
    zero = (np.zeros(6), np.zeros(6), gb, np.zeros(T, bool), False)
    if not live.any():
        return zero
    v, solved = pr.solve(n28, mu, lam)
    if not solved:
        return zero
    x, _ = pr.solve(n28, mu, 1.0)
    for k in range(T):
        if not live[k]:
            continue
        B, dd = s[k, 28:40].reshape(6, 2), s[k, 43:45]
        r0, r1 = dd[0], dd[1]
        for i in range(6):
            r0 = r0 + B[i, 0] * x[i]
            r1 = r1 + B[i, 1] * x[i]
        gb[k] = [float(g) for g in rr._c_solve(*fac[k], r0, r1)]
    return v, x, gb, live, True


def velocity(I_cur, I_des, Z_mm, depth_scale, K, level, interaction, mu, lam, tiles_y=4, tiles_x=4, robust_iterations=4, sigma_min=1.0,
             reverse=False):
    """dict(v [6], status, normal [T, 45], abs [T, 45], info [8] (the robust law's), robust [4] = live tiles, dead tiles, last sigma
    (0: N = 0), the live tiles' final sum w added in ascending k; tiles [T, 4] = gamma_k, beta_k, the tile's final sum w, live;
    tile [n], tile_n [T]; passes = per solve dict(x, gamma_beta, live, sigma, bin); weights [n]; margin_t, margin_m, near_t)."""
    gy, gx = int(tiles_y), int(tiles_x)
    H_, W_ = np.asarray(I_cur).shape[:2]
    h, w_, _, bands, _, _ = pr.plan(H_, W_, level)
    assert 1 <= gy <= min(8, h) and 1 <= gx <= min(8, w_) and 0 <= robust_iterations <= 4 and sigma_min > 0
    T = gy * gx
    out = dict(v=np.zeros(6), status=NO_DEPTH, normal=np.zeros((T, 45)), abs=np.zeros((T, 45)),
               info=np.array([0, h, w_, bands, 0, 0, 0, 0], np.int32), robust=np.zeros(4), tiles=np.zeros((T, 4)), tile=np.zeros(0, int),
               tile_n=np.zeros(T, int), passes=[], weights=np.zeros(0), margin_t=np.inf, margin_m=1 << 30, near_t=0)
    got = rr.rows(I_cur, I_des, Z_mm, depth_scale, K, level, interaction)
    if got is None:
        return out
    L, e, D, holes, _, _ = got
    n = L.shape[0]
    tile = tile_of_rows((H_, W_), Z_mm, level, gy, gx)
    assert tile.shape[0] == n
    wts = np.ones(n)
    sigma, m, zeros, x, gb = 0.0, -1, 0, np.zeros(6), np.zeros((T, 2))
    out.update(status=TOO_FEW, weights=wts, tile=tile, tile_n=np.bincount(tile, minlength=T))
    out["info"][[0, 4]] = n, holes
    for k in range(robust_iterations + 1):
        if k > 0:
            rw = rr.reweight(_residuals(L, e, D, x, gb, tile), sigma_min)
            wts, sigma, m = rw["w"], rw["sigma"], rw["bin"]
            zeros = int(np.sum(wts == 0.0))
            out.update(weights=wts, margin_t=min(out["margin_t"], rw["margin_t"]), margin_m=min(out["margin_m"], rw["margin_m"]),
                       near_t=out["near_t"] + rw["near_t"])
        out["normal"], out["abs"] = tile_sums(L, e, D, wts, tile, T, reverse)
        out["info"][6:] = zeros, k
        if n < 6 or n - zeros < 6:
            return out
        v, x, gb, live, solved = solve_tiles(out["normal"], mu, lam, reverse)
        if not solved:
            out["info"][5] = 1
            return out
        out["passes"].append(dict(x=x, gamma_beta=gb, live=live, sigma=sigma, bin=m))
    total = 0.0
    for k in (range(T - 1, -1, -1) if reverse else range(T)):
        if live[k]:
            total = total + out["normal"][k, 42]
    out.update(v=v, status=OK, robust=np.array([float(live.sum()), float(T - live.sum()), sigma, total]),
               tiles=np.column_stack([gb, out["normal"][:, 42], live.astype(np.float64)]))
    return out


def _residuals(L, e, D, x, gb, tile):
    p = L[:, 0] * x[0]
    for i in range(1, 6):
        p = p + L[:, i] * x[i]
    return np.abs(((e + p) - gb[tile, 0] * D) - gb[tile, 1])
