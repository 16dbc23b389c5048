"""Test infrastructure (never shipped): the robust photometric law (vit-vs_amd/csrc/photometric.hip) in fp64 numpy,
on photometric_ref.rows / pooled / solve.

Rows, L, e, holes, n, pooling and intrinsics are the plain law's (photometric_ref).  D = the pooled goal luminance at the row's pixel.
Parameters: ``illumination`` 0 / 1, ``robust_iterations`` N = 0 .. 4, ``sigma_min`` > 0 grey levels.

  w = 1 for every row; then N + 1 weighted solves with a re-weighting between two of them.
  One solve: with wv = w * [L0 .. L5, e, D] (one rounding each), the 45 sums
      A  [0, 21)   wv_i * L_j, upper triangle row-major      b  [21, 27)  wv_i * e        c  [27]  wv_e * e
      B  [28, 40)  (wv_i * D, wv_i) for i = 0 .. 5           C  [40, 43)  wv_D * D, wv_D, w
      d  [43, 45)  wv_D * e, wv_e
  with ``illumination``: C = [[DD, Dm], [Dm, Sw]] = l d l^T (d0 = DD, l = Dm (1 / d0), d1 = Sw - l l d0) under solve.h's pivot rule,
  u_i = C^-1 B_i, H'_ij = A_ij - (u_i0 B_j0 + u_i1 B_j1), g'_i = b_i - (u_i0 d_0 + u_i1 d_1); else H' = A, g' = b;
  x = -(H' + mu diag H')^-1 g' (photometric_ref.solve), (gamma, beta) = C^-1 (d + B^T x) or 0.
  One re-weighting: rho = |((e + L.x) - gamma D) - beta| (L.x added in column order), q = min(floor(16 rho), 4095), m = the first
  bin whose cumulative count reaches ceil(n / 2), median = (m + 0.5) / 16, sigma = max(1.4826 median, sigma_min),
  t = rho / (4.6851 sigma), w = (1 - t t)^2 if t < 1 else 0.
  v = lam x of the last solve.  TOO_FEW (v = 0, gamma = beta = sigma = sum w = 0) when n < 6, fewer than 6 rows keep a weight, or a
  pivot fails in any pass: the passes end there.  NO_DEPTH as the plain law.

``reverse=True``: every pass's sums over the rows in reversed order, as photometric_ref's."""
import numpy as np

import photometric_ref as pr
from robust_ref import MAD_SCALE, TUKEY_C
from solve_ref import THRESHOLD

OK, TOO_FEW, NO_DEPTH = pr.OK, pr.TOO_FEW, pr.NO_DEPTH
BINS, BIN_SCALE = 4096, 16.0
NAMES = ([f"A{i}{j}" for i, j in pr.TRIU] + [f"b{i}" for i in range(6)] + ["c"] + [f"B{i}{k}" for i in range(6) for k in "D1"]
         + ["CDD", "CD", "Cw", "dD", "d1"])
assert len(NAMES) == 45


def rows(I_cur, I_des, Z_mm, depth_scale, K, level, interaction):
    """photometric_ref.rows and D [n]: (L, e, D, holes, h, w), or None for NO_DEPTH."""
    got = pr.rows(I_cur, I_des, Z_mm, depth_scale, K, level, interaction)
    if got is None:
        return None
    L, e, holes, h, w = got
    Id = pr.pooled(I_des, level)
    part = np.ones((h - 2, w - 2), bool) if Z_mm is None else ~pr.pooled_depth(Z_mm, level)[1][1:-1, 1:-1]
    D = Id[1:-1, 1:-1][part]
    assert D.shape[0] == L.shape[0]
    return L, e, D, holes, h, w


def weighted_sums(L, e, D, w, reverse=False):
    """(normal45, abs45)."""
    wv = [w * L[:, i] for i in range(6)] + [w * e, w * D]
    terms = [wv[i] * L[:, j] for i, j in pr.TRIU] + [wv[i] * e for i in range(6)] + [wv[6] * e]
    for i in range(6):
        terms += [wv[i] * D, wv[i]]
    terms += [wv[7] * D, wv[7], w, wv[7] * e, wv[6]]
    return (np.array([pr._total(t, reverse) for t in terms]), np.array([pr._total(np.abs(t), False) for t in terms]))


def _c_factor(C3):
    """(l, d0, d1, good) of the 2 x 2 C = (DD, Dm, Sw) under solve.h's pivot rule."""
    DD, Dm, Sw = (float(c) for c in C3)
    with np.errstate(divide="ignore", invalid="ignore"):
        d0 = DD
        good = bool(d0 > THRESHOLD * DD) and bool(DD > 0.0)
        l = Dm * (np.float64(1.0) / d0)
        d1 = Sw - l * l * d0
        good = good and bool(d1 > THRESHOLD * Sw) and bool(Sw > 0.0)
    return l, d0, d1, good


def _c_solve(l, d0, d1, p, q):
    y1 = q - l * p
    z1 = y1 * (1.0 / d1)
    return p * (1.0 / d0) - l * z1, z1


def solve45(normal45, mu, lam, illumination):
    """(v [6], x [6], gamma, beta, solved) of the 45 sums."""
    s = np.asarray(normal45, np.float64).reshape(45)
    A, b, B, C3, dd = s[:21], s[21:27], s[28:40].reshape(6, 2), s[40:43], s[43:45]
    zero = (np.zeros(6), np.zeros(6), 0.0, 0.0, False)
    n28 = np.zeros(28)
    if illumination:
        l, d0, d1, good = _c_factor(C3)
        if not good:
            return zero
        u = [_c_solve(l, d0, d1, B[i, 0], B[i, 1]) for i in range(6)]
        for q, (i, j) in enumerate(pr.TRIU):
            n28[q] = A[q] - (u[i][0] * B[j, 0] + u[i][1] * B[j, 1])
        for i in range(6):
            n28[21 + i] = b[i] - (u[i][0] * dd[0] + u[i][1] * dd[1])
    else:
        n28[:27] = s[:27]
    v, solved = pr.solve(n28, mu, lam)
    if not solved:
        return zero
    x, _ = pr.solve(n28, mu, 1.0)
    gamma = beta = 0.0
    if illumination:
        r0, r1 = dd[0], dd[1]
        for i in range(6):
            r0 = r0 + B[i, 0] * x[i]
            r1 = r1 + B[i, 1] * x[i]
        gamma, beta = (float(g) for g in _c_solve(l, d0, d1, r0, r1))
    return v, x, gamma, beta, True


def residuals(L, e, D, x, gamma, beta):
    p = L[:, 0] * x[0]
    for i in range(1, 6):
        p = p + L[:, i] * x[i]
    return np.abs(((e + p) - gamma * D) - beta)


def reweight(rho, sigma_min):
    """dict(w, sigma, bin, margin_t, margin_m, near_t) of the residuals."""
    n = rho.shape[0]
    with np.errstate(invalid="ignore"):
        q = np.where(rho < BINS / BIN_SCALE, np.floor(BIN_SCALE * np.minimum(rho, BINS / BIN_SCALE)), BINS - 1).astype(np.int64)
    hist = np.bincount(q, minlength=BINS)
    cum = np.cumsum(hist)
    need = (n + 1) // 2
    m = int(np.searchsorted(cum, need, side="left"))
    before = int(cum[m - 1]) if m > 0 else 0
    margin_m = min(need - before - 1, int(cum[m]) - need)
    sigma = max(MAD_SCALE * ((m + 0.5) / BIN_SCALE), sigma_min)
    t = rho / (TUKEY_C * sigma)
    u = 1.0 - t * t
    w = np.where(t < 1.0, u * u, 0.0)
    return dict(w=w, sigma=float(sigma), bin=m, margin_t=float(np.min(np.abs(t - 1.0))), margin_m=int(margin_m),
                near_t=int(np.sum(np.abs(t - 1.0) < 1e-9)))


def velocity(I_cur, I_des, Z_mm, depth_scale, K, level, interaction, mu, lam, illumination=1, robust_iterations=4, sigma_min=1.0,
             reverse=False):
    """dict(v [6], status, normal [45], abs [45], info [8], robust [4] = gamma, beta, last sigma (0: N = 0), final sum w;
    passes = per solve dict(x, gamma, beta, sigma, bin) (sigma, bin of the re-weighting in front of it; 0, -1 in pass 0);
    weights [n]; margin_t, margin_m, near_t over all re-weightings): info = n, pooled h, pooled w, bands, holes, a pivot failed,
    rows of final weight 0, re-weightings run."""
    assert illumination in (0, 1) and 0 <= robust_iterations <= 4 and sigma_min > 0
    H_, W_ = np.asarray(I_cur).shape[:2]
    h, w_, _, bands, _, _ = pr.plan(H_, W_, level)
    out = dict(v=np.zeros(6), status=NO_DEPTH, normal=np.zeros(45), abs=np.zeros(45), info=np.array([0, h, w_, bands, 0, 0, 0, 0], np.int32),
               robust=np.zeros(4), passes=[], weights=np.zeros(0), margin_t=np.inf, margin_m=1 << 30, near_t=0)
    got = rows(I_cur, I_des, Z_mm, depth_scale, K, level, interaction)
    if got is None:
        return out
    L, e, D, holes, _, _ = got
    n = L.shape[0]
    wts = np.ones(n)
    sigma, m, zeros, x, gamma, beta = 0.0, -1, 0, np.zeros(6), 0.0, 0.0
    out.update(status=TOO_FEW, weights=wts)
    out["info"][[0, 4]] = n, holes
    for k in range(robust_iterations + 1):
        if k > 0:
            rw = reweight(residuals(L, e, D, x, gamma, beta), sigma_min)
            wts, sigma, m = rw["w"], rw["sigma"], rw["bin"]
            zeros = int(np.sum(wts == 0.0))
            out.update(weights=wts, margin_t=min(out["margin_t"], rw["margin_t"]), margin_m=min(out["margin_m"], rw["margin_m"]),
                       near_t=out["near_t"] + rw["near_t"])
        out["normal"], out["abs"] = weighted_sums(L, e, D, wts, reverse)
        out["info"][6:] = zeros, k
        if n < 6 or n - zeros < 6:
            return out
        v, x, gamma, beta, solved = solve45(out["normal"], mu, lam, illumination)
        if not solved:
            out["info"][5] = 1
            return out
        out["passes"].append(dict(x=x, gamma=gamma, beta=beta, sigma=sigma, bin=m))
    out.update(v=v, status=OK, robust=np.array([gamma, beta, sigma, out["normal"][42]]))
    return out


def few_weights_pair(seed=559):
    """(cur, des, K): a 4 x 7 pair of random frames (10 rows at level 0 with a scalar depth of 0.6 m, found by a search over seeds):
    without illumination, mu 0.01, the first solve fits five rows so much better than the other five that, with sigma_min 1e-3, the
    first re-weighting leaves a weight to those five alone (the closest t to 1 is 0.25 away)."""
    rng = np.random.default_rng(seed)
    des = rng.integers(0, 256, (4, 7, 3)).astype(np.uint8)
    cur = rng.integers(0, 256, (4, 7, 3)).astype(np.uint8)
    return cur, des, (6.0, 6.0, 3.5, 2.0)
