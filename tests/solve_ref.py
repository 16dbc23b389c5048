"""Test infrastructure (never shipped): a high-precision reference for the 6 x 6 solve every control law ends in
(vit-vs_amd/csrc/solve.h, and servo.hip's inline copy of it for the plain law), and the device's pivot rule restated.

solve.h solves the normal equations G = L^T L, g = L^T e by LDL^T and hands over to a one-sided Jacobi SVD of L itself when a
pivot fails ``d_j > THRESHOLD * G_jj``.  G has the condition number cond(L)^2, so just above the threshold LDL^T is the
normal-equations solver at the conditioning where it loses its digits.  To judge that, numpy.linalg.pinv in fp64 (the oracle's
solver) is not enough: it has an error of its own, which grows with cond(L) as well.  ``exact_solution`` is the same least-squares
problem at 50 decimal digits, where the normal equations are harmless (cond(L) <= 1e8 squares to 1e16, 34 digits short of 1e50),
rounded once to fp64.

``THRESHOLD`` lives here and nowhere else in tests/: law_support.ldlt_passes and rig_ref.ldlt_margin read it, so the restatement
and the cases chosen around it cannot drift apart."""
import mpmath
import numpy as np

THRESHOLD = 1e-4        # solve.h kPivotThreshold: LDL^T solves when every pivot d_j > THRESHOLD * G_jj, else the Jacobi SVD does
DIGITS = 50


def exact_solution(L, e) -> np.ndarray:
    """argmin_x |L x - e|_2 of fp64 L (R x 6, full column rank) and e (R), computed at 50 digits and rounded once to fp64."""
    L = np.asarray(L, np.float64)
    e = np.asarray(e, np.float64).reshape(-1)
    assert L.ndim == 2 and L.shape[0] == e.shape[0]
    with mpmath.workdps(DIGITS):
        A = mpmath.matrix(L.tolist())
        b = mpmath.matrix(e.tolist())
        x = mpmath.lu_solve(A.T * A, A.T * b)
        return np.array([float(x[i]) for i in range(L.shape[1])])


def ldlt_factor(L):
    """(d [6], diag G [6], Lf [6, 6]) of G = L^T L = Lf D Lf^T in fp64, in solve.h's order of operations (no pivot test: a zero or
    negative pivot gives infinities or NaNs further on, as on the device, where the test then discards them)."""
    L = np.asarray(L, np.float64)
    G = L.T @ L
    Lf, dpiv = np.zeros((6, 6)), np.zeros(6)
    with np.errstate(divide="ignore", invalid="ignore"):
        for j in range(6):
            d = G[j, j] - sum(Lf[j, k] ** 2 * dpiv[k] for k in range(j))
            dpiv[j] = d
            for i in range(j + 1, 6):
                Lf[i, j] = (G[i, j] - sum(Lf[i, k] * Lf[j, k] * dpiv[k] for k in range(j))) / d
    return dpiv, np.diag(G).copy(), Lf


def ldlt_passes(L) -> bool:
    """The device's pivot test on the normal equations of L (rows x 6), restated in fp64."""
    d, diag, _ = ldlt_factor(L)
    return bool(all(d[j] > THRESHOLD * diag[j] and diag[j] > 0 for j in range(6)))


def pivot_ratio(L) -> float:
    """The smallest d_j / G_jj of the LDL^T of L^T L, in ldlt_passes' arithmetic (0 for a zero column or a pivot that is not
    positive: LDL^T passes exactly when this is above THRESHOLD, up to the rounding of one division)."""
    d, diag, _ = ldlt_factor(L)
    if not (diag > 0).all():
        return 0.0
    ratios = d / diag
    return float(max(np.min(ratios), 0.0)) if np.isfinite(ratios).all() else 0.0


def ldlt_solution(L, e) -> np.ndarray:
    """solve_ldlt restated in fp64 and forced past its pivot test: the factorisation above and the two substitutions, with one
    reciprocal per pivot as on the device.  What LDL^T would return for a system the hand-off takes away from it."""
    L = np.asarray(L, np.float64)
    rhs = L.T @ np.asarray(e, np.float64).reshape(-1)
    d, _, Lf = ldlt_factor(L)
    with np.errstate(divide="ignore", invalid="ignore"):
        dinv = 1.0 / d
        y, x = np.zeros(6), np.zeros(6)
        for i in range(6):
            y[i] = rhs[i] - sum(Lf[i, k] * y[k] for k in range(i))
        for i in range(5, -1, -1):
            x[i] = y[i] * dinv[i] - sum(Lf[k, i] * x[k] for k in range(i + 1, 6))
    return x


def pinv_solution(L, e) -> np.ndarray:
    """numpy.linalg.pinv(L) e in fp64: the solver of oracle/servo_ref and of every fp64 reference in tests/."""
    return np.linalg.pinv(np.asarray(L, np.float64)) @ np.asarray(e, np.float64).reshape(-1)


def rel_l2(a, b) -> float:
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))
