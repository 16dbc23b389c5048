"""Test infrastructure (never shipped): the photometric rig law (vit-vs_amd/csrc/photometric.hip) in fp64 numpy, on
photometric_robust_ref's rows, sums, 2 x 2 elimination, residuals and re-weighting and on photometric_ref.solve.

``n_cams`` cameras of one rigid rig; camera i has its own frames, depth, K and the twist transform W_i = cVr[i]
(servo.twist_matrix: v_cam_i = W_i v_rig).  ``live`` [n_cams] of 0 / 1 or None: a dead camera takes no part in anything.  The
parameters are the robust photometric law's.

  w = 1 for every row; then N + 1 weighted solves with a re-weighting between two of them.
  One solve.  Per live camera with at least one row, in ascending camera order:
      the 45 sums S_i of photometric_robust_ref over its own rows;
      with ``illumination`` C_i = l d l^T and H'_i, g'_i exactly as photometric_robust_ref.solve45 forms them (a failed pivot of
      any such camera fails the call); else H'_i = A_i, g'_i = b_i;
      M[a][k] = sum_b H'_i[a][b] W_i[b][k],  T_i[j][k] = sum_a W_i[a][j] M[a][k] (j <= k),  (W^T g')[k] = sum_a W_i[a][k] g'_i[a],
      every sum from its first product on, the index ascending;
      H_r += T_i, g_r += W_i^T g'_i, c_r += S_i[27], from 0.
  x = -(H_r + mu diag H_r)^-1 g_r (photometric_ref.solve), x_i[a] = sum_k W_i[a][k] x[k],
  (gamma_i, beta_i) = C_i^-1 (d_i + B_i^T x_i) or 0.
  One re-weighting: rho = |((e + L.x_i) - gamma_i D) - beta_i| of every row of every live camera into ONE histogram, the median bin
  at ceil(n_total / 2), one sigma, and Tukey weights as photometric_robust_ref.reweight.  ``scale="camera"`` (the reference only,
  for the comparison of tests/test_photometric_rig_host.py): each camera's own histogram, median at ceil(n_i / 2) and sigma.
  v_rig = lam x of the last solve.  TOO_FEW (v_rig = 0, every gamma, beta, sigma, sum w = 0) when n_total < 6, fewer than 6 rows of
  the stack keep a weight, or a pivot (a camera's 2 x 2, the 6 x 6) fails in any pass: the passes end there.  NO_DEPTH as the
  plain law (no depth images and a scalar <= 0).  A live camera without a row (all holes) adds nothing and fails nothing.

``reverse=True``: every camera's sums over its rows in reversed order AND the cameras added in descending order."""
import numpy as np

import photometric_ref as pr
import photometric_robust_ref as rr

OK, TOO_FEW, NO_DEPTH = pr.OK, pr.TOO_FEW, pr.NO_DEPTH


def camera_system(S, W, illumination):
    """(T [21], Wg [6], factor = (l, d0, d1) or None, good) of one camera's 45 sums."""
    s = np.asarray(S, np.float64).reshape(45)
    A, b, B, C3, dd = s[:21], s[21:27], s[28:40].reshape(6, 2), s[40:43], s[43:45]
    n27 = np.zeros(27)
    factor = None
    if illumination:
        l, d0, d1, good = rr._c_factor(C3)
        if not good:
            return None, None, None, False
        factor = (l, d0, d1)
        u = [rr._c_solve(l, d0, d1, B[i, 0], B[i, 1]) for i in range(6)]
        for q, (i, j) in enumerate(pr.TRIU):
            n27[q] = A[q] - (u[i][0] * B[j, 0] + u[i][1] * B[j, 1])
        for i in range(6):
            n27[21 + i] = b[i] - (u[i][0] * dd[0] + u[i][1] * dd[1])
    else:
        n27[:] = s[:27]
    H = np.zeros((6, 6))
    for q, (i, j) in enumerate(pr.TRIU):
        H[i, j] = H[j, i] = n27[q]
    g = n27[21:27]
    W = np.asarray(W, np.float64).reshape(6, 6)
    M = np.zeros((6, 6))
    for a in range(6):
        for k in range(6):
            t = H[a, 0] * W[0, k]
            for bb in range(1, 6):
                t = t + H[a, bb] * W[bb, k]
            M[a, k] = t
    T = np.zeros(21)
    for q, (j, k) in enumerate(pr.TRIU):
        t = W[0, j] * M[0, k]
        for a in range(1, 6):
            t = t + W[a, j] * M[a, k]
        T[q] = t
    Wg = np.zeros(6)
    for k in range(6):
        t = W[0, k] * g[0]
        for a in range(1, 6):
            t = t + W[a, k] * g[a]
        Wg[k] = t
    return T, Wg, factor, True


def camera_step(W, x):
    W = np.asarray(W, np.float64).reshape(6, 6)
    out = np.zeros(6)
    for a in range(6):
        t = W[a, 0] * x[0]
        for k in range(1, 6):
            t = t + W[a, k] * x[k]
        out[a] = t
    return out


def _lighting(S, factor, xi):
    s = np.asarray(S, np.float64)
    B, dd = s[28:40].reshape(6, 2), s[43:45]
    r0, r1 = dd[0], dd[1]
    for i in range(6):
        r0 = r0 + B[i, 0] * xi[i]
        r1 = r1 + B[i, 1] * xi[i]
    return tuple(float(g) for g in rr._c_solve(*factor, r0, r1))


def velocity(I_cur, I_des, Z_mm, depth_scale, K, cVr, live, level, interaction, mu, lam, illumination=1, robust_iterations=4,
             sigma_min=1.0, reverse=False, scale="stack"):
    """I_cur, I_des: sequences of n_cams frames; Z_mm: a sequence of depth images or None; K [n_cams][4]; cVr [n_cams][6][6].
    dict(v [6], status, normal [n_cams][45], abs [n_cams][45], rig_normal [28], info [8] = live cameras, n_total, rows of final
    weight 0, re-weightings run, holes, a pivot failed, pooled h, pooled w; robust [n_cams][4] = gamma_i, beta_i, last sigma, sum
    w_i; n [n_cams], zeros [n_cams]; passes = per solve dict(x, gamma, beta, sigma, bin); bin = the last median bin (-1: none);
    margin_t, margin_m, near_t over all re-weightings as photometric_robust_ref's; margin_e = the smallest distance of any row's
    16 rho from a bin edge, in bins, over all re-weightings)."""
    assert illumination in (0, 1) and 0 <= robust_iterations <= 4 and sigma_min > 0 and scale in ("stack", "camera")
    nc = len(I_cur)
    K = np.asarray(K, np.float64).reshape(nc, 4)
    cVr = np.asarray(cVr, np.float64).reshape(nc, 6, 6)
    alive = [i for i in range(nc) if live is None or live[i]]
    H_, W_ = np.asarray(I_cur[0]).shape[:2]
    h, w_ = H_ >> level, W_ >> level
    out = dict(v=np.zeros(6), status=NO_DEPTH, normal=np.zeros((nc, 45)), abs=np.zeros((nc, 45)), rig_normal=np.zeros(28),
               info=np.array([len(alive), 0, 0, 0, 0, 0, h, w_], np.int32), robust=np.zeros((nc, 4)), n=np.zeros(nc, np.int64),
               zeros=np.zeros(nc, np.int64), passes=[], bin=-1, margin_t=np.inf, margin_m=1 << 30, margin_e=np.inf, near_t=0)
    if Z_mm is None and not depth_scale > 0.0:
        return out
    cams = {}
    for i in alive:
        L, e, D, holes, _, _ = rr.rows(I_cur[i], I_des[i], None if Z_mm is None else Z_mm[i], depth_scale, K[i], level, interaction)
        cams[i] = dict(L=L, e=e, D=D, w=np.ones(L.shape[0]), x=np.zeros(6), gamma=0.0, beta=0.0)
        out["n"][i] = L.shape[0]
        out["info"][4] += holes
    n_total = int(out["n"].sum())
    out["status"] = TOO_FEW
    out["info"][1] = n_total
    order = alive[::-1] if reverse else alive
    sigmas = {i: 0.0 for i in alive}
    for k in range(robust_iterations + 1):
        if k > 0:
            rho = {i: rr.residuals(c["L"], c["e"], c["D"], c["x"], c["gamma"], c["beta"]) for i, c in cams.items()}
            for r in rho.values():
                q = rr.BIN_SCALE * r[r < rr.BINS / rr.BIN_SCALE]
                if q.shape[0]:
                    out["margin_e"] = min(out["margin_e"], float(np.min(np.abs(q - np.rint(q)))))
            if scale == "stack":
                rw = rr.reweight(np.concatenate([rho[i] for i in alive]), sigma_min)
                at = 0
                for i in alive:
                    cams[i]["w"] = rw["w"][at:at + rho[i].shape[0]]
                    at += rho[i].shape[0]
                    sigmas[i] = rw["sigma"]
                rws = [rw]
            else:
                rws = []
                for i in alive:
                    if rho[i].shape[0]:
                        rw = rr.reweight(rho[i], sigma_min)
                        cams[i]["w"], sigmas[i] = rw["w"], rw["sigma"]
                        rws.append(rw)
            for rw in rws:
                out.update(margin_t=min(out["margin_t"], rw["margin_t"]), margin_m=min(out["margin_m"], rw["margin_m"]),
                           near_t=out["near_t"] + rw["near_t"], bin=rw["bin"])
            for i in alive:
                out["zeros"][i] = int(np.sum(cams[i]["w"] == 0.0))
        for i in alive:
            c = cams[i]
            out["normal"][i], out["abs"][i] = rr.weighted_sums(c["L"], c["e"], c["D"], c["w"], reverse)
        zeros = int(out["zeros"].sum())
        out["info"][2:4] = zeros, k
        if n_total < 6 or n_total - zeros < 6:
            return out
        rn = np.zeros(28)
        factors = {}
        for i in order:
            if out["n"][i] == 0:
                continue
            T, Wg, factors[i], good = camera_system(out["normal"][i], cVr[i], illumination)
            if not good:
                out["info"][5] = 1
                return out
            rn[:21] += T
            rn[21:27] += Wg
            rn[27] += out["normal"][i][27]
        out["rig_normal"] = rn
        v, solved = pr.solve(rn, mu, lam)
        if not solved:
            out["info"][5] = 1
            return out
        x, _ = pr.solve(rn, mu, 1.0)
        for i in alive:
            c = cams[i]
            c["x"] = camera_step(cVr[i], x)
            c["gamma"], c["beta"] = _lighting(out["normal"][i], factors[i], c["x"]) if (illumination and out["n"][i]) else (0.0, 0.0)
        out["passes"].append(dict(x=x, gamma=[cams[i]["gamma"] for i in alive], beta=[cams[i]["beta"] for i in alive],
                                  sigma=dict(sigmas), bin=out["bin"]))
    out.update(v=v, status=OK)
    for i in alive:
        if out["n"][i]:
            out["robust"][i] = cams[i]["gamma"], cams[i]["beta"], sigmas[i], out["normal"][i][42]
    return out
