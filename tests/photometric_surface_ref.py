"""Test infrastructure (never shipped): the surface photometric law (vit-vs_amd/csrc/photometric.hip) in fp64 numpy,
on photometric_robust_ref's functions.

Rows, L, e, D, holes, n, pooling, intrinsics, the histogram median, sigma, Tukey's weights and the 6 x 6 LM solve are the robust
law's.  The lighting model is a BILINEAR SPLINE of gains and biases on the nodes of a ``cells_y`` x ``cells_x`` = gy x gx grid (each
1 .. 8, gy <= pooled h, gx <= pooled w) over the pooled image: (gy + 1)(gx + 1) nodes, node a = i (gx + 1) + j, unknown 2a = gamma_a,
unknown 2a + 1 = beta_a, M = 2 (gy + 1)(gx + 1) <= 162.

  Per row at pooled pixel (r, c): cell (i, j) = (floor(r gy / h), floor(c gx / w)) (the tile law's tile), v = (r gy - i h) / h,
  u = (c gx - j w) / w (exact integer numerators, one division each), phi = [(1-v)(1-u), (1-v) u, v (1-u), v u] (1-v, 1-u and the
  products one rounding each) for the nodes (i, j), (i, j+1), (i+1, j), (i+1, j+1); I_cur ~ (1 + sum phi_a gamma_a) I_des + sum
  phi_a beta_a; m = [D phi0, phi0, D phi1, phi1, D phi2, phi2, D phi3, phi3] (D phi one rounding).
  Per cell the 120 weighted sums over its rows in row-major order, with wv = w * [L0 .. L5, e] and wm = w * m (one rounding each):
      A [0, 21) wv_i * L_j (upper triangle, row-major)   b [21, 27) wv_i * e   c [27] wv_e * e   B [28, 76) wv_i * m_k (6 x 8)
      C [76, 112) wm_k * m_l (k <= l, row-major)          d [112, 120) wm_k * e
  and, beside them, sum w.
  One solve: from zero and in ascending cell index the cells add into C_g (M x M), B_g (6 x M), d_g (M) and A, b, c (local unknown
  2 s + t of a cell = unknown 2 a_s + t of its s-th node).  The bordered system [[C_g, R^T], [R, S]], R = the six rows of B_g and
  d_g, S = [[A, b], [b^T, c]], is eliminated column by column in ascending j (right-looking; half-bandwidth 2 gx + 5): with
  d_j = the current C_jj, unknown j is live iff C_jj(assembled) > 0 and d_j > THRESHOLD C_jj(assembled), else DEAD in this pass
  (column skipped, value 0); a live column's l_i = W_ij (1 / d_j) and every entry (i, k) behind it loses (l_i l_k) d_j.  What is left
  of S is H' = A - B_g C_g^-1 B_g^T, g' = b - B_g C_g^-1 d_g; x = -(H' + mu diag H')^-1 g' (photometric_ref.solve);
  t_j = z_dj + sum_i z_ij x_i (i ascending; z = the eliminated R times 1 / d_j), q_j = t_j - sum l_ij q_i over i = j + bw .. j + 1
  in DESCENDING i: q = C_g^-1 (d_g + B_g^T x), the nodes' values.
  One re-weighting: rho = |((e + L.x) - gamma(r,c) D) - beta(r,c)|, gamma(r,c) = sum phi_a gamma_a in the order above, ONE
  histogram, median and sigma over all rows, the robust law's weights.
  TOO_FEW (everything 0) when n < 6, fewer than 6 rows keep a weight, every unknown is dead, or the 6 x 6 pivot fails.

``reverse=True``: the rows of each cell reversed and the cells taken in descending order: the yardstick for the device's sums."""
import numpy as np

import photometric_ref as pr
import photometric_robust_ref as rr
import photometric_tile_ref as tr
from solve_ref import THRESHOLD

OK, TOO_FEW, NO_DEPTH = pr.OK, pr.TOO_FEW, pr.NO_DEPTH
NS = 120
TRIU8 = [(k, l) for k in range(8) for l in range(k, 8)]
NAMES = (rr.NAMES[:28] + [f"B{i}m{k}" for i in range(6) for k in range(8)] + [f"C{k}{l}" for k, l in TRIU8]
         + [f"d{k}" for k in range(8)])
assert len(NAMES) == NS


def plan(height, width, level, cells_y, cells_x):
    """vitvs_op_photometric_surface_plan restated: the tile plan's bands, slots and LDS; 128 doubles per (band, slot, cell
    column) partial."""
    h, w, rows, bands, slots, lds, lds_res, _ = tr.plan(height, width, level, cells_y, cells_x)
    return h, w, rows, bands, slots, lds, lds_res, bands * slots * cells_x * 128


def weights_of_rows(shape, Z_mm, level, gy, gx):
    """(cell [n], phi [n, 4]) of photometric_ref.rows' rows."""
    h, w = shape[0] >> level, shape[1] >> level
    r, c = np.meshgrid(np.arange(1, h - 1), np.arange(1, w - 1), indexing="ij")
    i, j = r * gy // h, c * gx // w
    v = (r * gy - i * h).astype(np.float64) / float(h)
    u = (c * gx - j * w).astype(np.float64) / float(w)
    v1, u1 = 1.0 - v, 1.0 - u
    phi = np.stack([v1 * u1, v1 * u, v * u1, v * u], axis=-1)
    part = np.ones((h - 2, w - 2), bool) if Z_mm is None else ~pr.pooled_depth(Z_mm, level)[1][1:-1, 1:-1]
    return (i * gx + j)[part], phi[part]


def cell_nodes(k, gx):
    """the four nodes of cell k."""
    i, j = divmod(k, gx)
    a = i * (gx + 1) + j
    return [a, a + 1, a + gx + 1, a + gx + 2]


def _terms(L, e, D, phi, w):
    wv = [w * L[:, i] for i in range(6)] + [w * e]
    m = []
    for s in range(4):
        m += [D * phi[:, s], phi[:, s]]
    wm = [w * mk for mk in m]
    t = [wv[i] * L[:, j] for i, j in pr.TRIU] + [wv[i] * e for i in range(6)] + [wv[6] * e]
    t += [wv[i] * m[k] for i in range(6) for k in range(8)]
    t += [wm[k] * m[l] for k, l in TRIU8]
    t += [wm[k] * e for k in range(8)]
    return t


def cell_sums(L, e, D, phi, w, cell, T, reverse=False):
    """(normal [T, 120], abs [T, 120], sum w [T]) of the rows of every cell."""
    normal, absum, sw = np.zeros((T, NS)), np.zeros((T, NS)), np.zeros(T)
    for k in range(T):
        m = cell == k
        if not m.any():
            continue
        t = _terms(L[m], e[m], D[m], phi[m], w[m])
        normal[k] = [pr._total(q, reverse) for q in t]
        absum[k] = [pr._total(np.abs(q), False) for q in t]
        sw[k] = pr._total(w[m], reverse)
    return normal, absum, sw


def assemble(normal, gy, gx, reverse=False):
    """(C_g [M, M] symmetric, R [7, M] = B_g and d_g, S [7, 7] symmetric = A, b, c) of the cells' sums."""
    s = np.asarray(normal, np.float64).reshape(gy * gx, NS)
    M = 2 * (gy + 1) * (gx + 1)
    Cg, R, S28 = np.zeros((M, M)), np.zeros((7, M)), np.zeros(28)
    T = gy * gx
    for k in (range(T - 1, -1, -1) if reverse else range(T)):
        idx = [2 * a + t for a in cell_nodes(k, gx) for t in (0, 1)]
        S28 = S28 + s[k, :28]
        B = s[k, 28:76].reshape(6, 8)
        for loc, g in enumerate(idx):
            for i in range(6):
                R[i, g] = R[i, g] + B[i, loc]
            R[6, g] = R[6, g] + s[k, 112 + loc]
        for q, (a, b) in enumerate(TRIU8):
            Cg[idx[a], idx[b]] = Cg[idx[a], idx[b]] + s[k, 76 + q]
    Cg = np.triu(Cg) + np.triu(Cg, 1).T
    S = np.zeros((7, 7))
    for q, (i, j) in enumerate(pr.TRIU):
        S[i, j] = S[j, i] = S28[q]
    S[:6, 6] = S[6, :6] = S28[21:27]
    S[6, 6] = S28[27]
    return Cg, R, S


def eliminate(Cg, R, S, gx):
    """The bordered elimination: dict(W (the eliminated C_g, column j below the diagonal = l_ij d_j), Z [7, M] = the eliminated R
    times 1 / d_j, S' [7, 7], live [M], dinv [M], ratio [M] = d_j / C_jj (nan where C_jj <= 0))."""
    M = Cg.shape[0]
    bw = 2 * gx + 5
    W, R, S = Cg.copy(), R.copy(), S.copy()
    live, dinv, ratio = np.zeros(M, bool), np.zeros(M), np.full(M, np.nan)
    for j in range(M):
        c0, d = Cg[j, j], W[j, j]
        if c0 > 0.0:
            ratio[j] = d / c0
        if not (c0 > 0.0 and d > THRESHOLD * c0):
            continue
        live[j] = True
        di = 1.0 / d
        dinv[j] = di
        hi = min(M, j + bw + 1)
        lc, lr = W[j + 1:hi, j] * di, R[:, j] * di
        W[j + 1:hi, j + 1:hi] -= np.outer(lc, lc) * d
        R[:, j + 1:hi] -= np.outer(lr, lc) * d
        S -= np.outer(lr, lr) * d
    return dict(W=W, Z=R * dinv[None, :], S=S, live=live, dinv=dinv, ratio=ratio, bw=bw)


def back_substitute(el, x):
    """q [M] = C_g^-1 (d_g + B_g^T x) over the live unknowns, 0 at the dead ones."""
    W, Z, live, dinv, bw = el["W"], el["Z"], el["live"], el["dinv"], el["bw"]
    M = W.shape[0]
    q = np.zeros(M)
    for j in range(M - 1, -1, -1):
        if not live[j]:
            continue
        t = Z[6, j]
        for i in range(6):
            t = t + Z[i, j] * x[i]
        for i in range(min(M, j + bw + 1) - 1, j, -1):
            t = t - (W[i, j] * dinv[j]) * q[i]
        q[j] = t
    return q


def solve_cells(normal, gy, gx, mu, lam, reverse=False):
    """(v [6], x [6], q [M], live [M] bool, ratio [M], solved) of the cells' sums."""
    Cg, R, S = assemble(normal, gy, gx, reverse)
    el = eliminate(Cg, R, S, gx)
    M = Cg.shape[0]
    zero = (np.zeros(6), np.zeros(6), np.zeros(M), np.zeros(M, bool), el["ratio"], False)
    if not el["live"].any():
        return zero
    n28 = np.array([el["S"][i, j] for i, j in pr.TRIU] + [el["S"][i, 6] for i in range(6)] + [el["S"][6, 6]])
    v, solved = pr.solve(n28, mu, lam)
    if not solved:
        return zero
    x, _ = pr.solve(n28, mu, 1.0)
    return v, x, back_substitute(el, x), el["live"], el["ratio"], True


def lighting_of_rows(q, cell, phi, gx):
    """(gamma [n], beta [n]) of the rows: the phi-sums over the four nodes, in node order."""
    nodes = np.array([cell_nodes(k, gx) for k in range(int(cell.max()) + 1 if cell.size else 0)]).reshape(-1, 4)[cell]
    g = phi[:, 0] * q[2 * nodes[:, 0]]
    b = phi[:, 0] * q[2 * nodes[:, 0] + 1]
    for s in range(1, 4):
        g = g + phi[:, s] * q[2 * nodes[:, s]]
        b = b + phi[:, s] * q[2 * nodes[:, s] + 1]
    return g, b


def _residuals(L, e, D, x, g, b):
    p = L[:, 0] * x[0]
    for i in range(1, 6):
        p = p + L[:, i] * x[i]
    return np.abs(((e + p) - g * D) - b)


def velocity(I_cur, I_des, Z_mm, depth_scale, K, level, interaction, mu, lam, cells_y=4, cells_x=4, robust_iterations=4, sigma_min=1.0,
             reverse=False):
    """dict(v [6], status, normal [T, 120], abs [T, 120], info [8] (the robust law's), robust [4] = live unknowns, dead unknowns,
    last sigma (0: N = 0), the final sum w added over the cells in ascending index; nodes [nodes, 4] = gamma_a, beta_a, gamma_a
    live, beta_a live; cell [n], cell_n [T]; passes = per solve dict(x, q, live, ratio, sigma, bin); weights [n]; margin_t,
    margin_m, near_t)."""
    gy, gx = int(cells_y), int(cells_x)
    H_, W_ = np.asarray(I_cur).shape[:2]
    h, w_, _, bands, _, _ = pr.plan(H_, W_, level)
    assert 1 <= gy <= min(8, h) and 1 <= gx <= min(8, w_) and 0 <= robust_iterations <= 4 and sigma_min > 0
    T, nodes = gy * gx, (gy + 1) * (gx + 1)
    out = dict(v=np.zeros(6), status=NO_DEPTH, normal=np.zeros((T, NS)), abs=np.zeros((T, NS)),
               info=np.array([0, h, w_, bands, 0, 0, 0, 0], np.int32), robust=np.zeros(4), nodes=np.zeros((nodes, 4)),
               cell=np.zeros(0, int), cell_n=np.zeros(T, int), passes=[], weights=np.zeros(0), margin_t=np.inf, margin_m=1 << 30,
               near_t=0)
    got = rr.rows(I_cur, I_des, Z_mm, depth_scale, K, level, interaction)
    if got is None:
        return out
    L, e, D, holes, _, _ = got
    n = L.shape[0]
    cell, phi = weights_of_rows((H_, W_), Z_mm, level, gy, gx)
    assert cell.shape[0] == n
    wts = np.ones(n)
    sigma, m, zeros, x, q = 0.0, -1, 0, np.zeros(6), np.zeros(2 * nodes)
    out.update(status=TOO_FEW, weights=wts, cell=cell, cell_n=np.bincount(cell, minlength=T))
    out["info"][[0, 4]] = n, holes
    for k in range(robust_iterations + 1):
        if k > 0:
            g, b = lighting_of_rows(q, cell, phi, gx)
            rw = rr.reweight(_residuals(L, e, D, x, g, b), sigma_min)
            wts, sigma, m = rw["w"], rw["sigma"], rw["bin"]
            zeros = int(np.sum(wts == 0.0))
            out.update(weights=wts, margin_t=min(out["margin_t"], rw["margin_t"]), margin_m=min(out["margin_m"], rw["margin_m"]),
                       near_t=out["near_t"] + rw["near_t"])
        out["normal"], out["abs"], sw = cell_sums(L, e, D, phi, wts, cell, T, reverse)
        out["info"][6:] = zeros, k
        if n < 6 or n - zeros < 6:
            return out
        v, x, q, live, ratio, solved = solve_cells(out["normal"], gy, gx, mu, lam, reverse)
        if not solved:
            out["info"][5] = 1
            return out
        out["passes"].append(dict(x=x, q=q, live=live, ratio=ratio, sigma=sigma, bin=m))
    total = 0.0
    for k in (range(T - 1, -1, -1) if reverse else range(T)):
        total = total + sw[k]
    qq, ll = q.reshape(nodes, 2), live.reshape(nodes, 2).astype(np.float64)
    out.update(v=v, status=OK, robust=np.array([float(live.sum()), float(live.size - live.sum()), sigma, total]),
               nodes=np.column_stack([qq, ll]))
    return out
