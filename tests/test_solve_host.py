"""What makes tests/test_gpu_solve_handoff.py a test of the hand-off from LDL^T to the Jacobi SVD, asserted on the CPU from the
oracle's system of every case of tests/solve_cases.py (the weighted family: the reference's weighted system; the rig: the stack).

The cases crowd both sides of the pivot threshold and none sits within a factor 2 of it (the device adds G in 8 slices x 4 chains,
not in numpy's order: which solver ran may only be asserted outside a guard band); numpy.linalg.pinv in fp64 can judge every case
that is held to the absolute bar; and an fp64 restatement of LDL^T, forced past the pivot test, is visibly wrong below the
threshold, so a hand-off that came too late could not hide.  The last test prints the sweep the threshold is chosen from
(DESIGN.md §5)."""
import numpy as np
import pytest

import solve_cases as sc
import solve_ref as sv

VC_BAR = 1e-9            # the project's bar for a twist (relative L2)
PINV_BAR = 1e-10         # a case is held to VC_BAR only where fp64 pinv is this close to the 50-digit solution


def _systems():
    """name -> (L, e) of the final solve, camera cases and rig stacks alike."""
    out = {c.name: (sc.system(c)["Ls"], sc.system(c)["es"]) for c in sc.CASES}
    out.update({name: sc.rig_system(case) for name, case in sc.RIG_CASES.items()})
    return out


@pytest.fixture(scope="module")
def table():
    """name -> dict(ratio, cond, ldlt, pinv): pivot ratio, cond(L), and the errors of forced LDL^T and of pinv against the
    50-digit solution.  Computed once for the module."""
    out = {}
    for name, (L, e) in _systems().items():
        x = sv.exact_solution(L, e)
        assert np.linalg.norm(x) > 0, name
        out[name] = dict(ratio=sv.pivot_ratio(L), cond=float(np.linalg.cond(L)), ldlt=sv.rel_l2(sv.ldlt_solution(L, e), x),
                         pinv=sv.rel_l2(sv.pinv_solution(L, e), x))
    return out


def test_exact_solution_is_the_least_squares_solution():
    """On a well-conditioned system with a residual the 50-digit solution agrees with fp64 lstsq to rounding and its residual is
    orthogonal to the columns of L; on a consistent system it returns the planted solution."""
    rng = np.random.default_rng(1)
    L, e = rng.standard_normal((48, 6)), rng.standard_normal(48)
    x = sv.exact_solution(L, e)
    assert sv.rel_l2(x, np.linalg.lstsq(L, e, rcond=None)[0]) <= 1e-14
    assert np.max(np.abs(L.T @ (e - L @ x))) <= 1e-13
    planted = np.array([1.0, -2.0, 0.5, 3.0, -1.0, 0.25])
    L = rng.integers(-8, 9, size=(48, 6)).astype(np.float64)          # L planted is exact in fp64
    assert np.array_equal(sv.exact_solution(L, L @ planted), planted)


def test_pivot_ratio_is_the_pivot_test():
    for name, (L, _) in _systems().items():
        assert sv.ldlt_passes(L) == (sv.pivot_ratio(L) > sv.THRESHOLD), name
    assert sv.pivot_ratio(np.zeros((8, 6))) == 0.0 and not sv.ldlt_passes(np.zeros((8, 6)))
    L = np.random.default_rng(2).standard_normal((8, 6))
    L[:, 4] = L[:, 1]                                                  # an exactly repeated column: the pivot cancels
    assert sv.pivot_ratio(L) <= 1e-15 and not sv.ldlt_passes(L)


def test_the_cases_cover_the_hand_off(table):
    t = sv.THRESHOLD
    ratios = np.array([row["ratio"] for row in table.values()])
    assert np.count_nonzero((ratios >= t) & (ratios <= 100 * t)) >= 6
    assert np.count_nonzero((ratios >= t / 100) & (ratios < t)) >= 4
    assert np.count_nonzero(ratios > 1e-3) >= 4
    assert all(row["cond"] <= 1e8 for row in table.values())
    # every family that names a side of the threshold has a case on it
    for family in ("many_rows", "weighted-1", "weighted-4", "rig"):
        sides = {table[name]["ratio"] > t for name in table if name.startswith(family)}
        assert sides == {True, False}, family


def test_no_case_sits_in_the_guard_band(table):
    """Fails when the threshold moves until the sweep's points are chosen again: that is its purpose."""
    for name, row in table.items():
        assert not (sv.THRESHOLD / sc.GUARD < row["ratio"] < sv.THRESHOLD * sc.GUARD), (name, row["ratio"])


def test_the_reference_can_judge(table):
    """A case whose fp64 pinv is further than 1e-10 from the 50-digit solution is held to 8 x pinv's own error instead of the
    absolute bar; at most a quarter of the cases may be of that kind."""
    relative = [name for name, row in table.items() if row["pinv"] > PINV_BAR]
    assert len(relative) <= len(table) // 4, relative
    for name, row in table.items():
        if name not in relative:
            assert 8 * row["pinv"] <= VC_BAR, name                    # the bar of such a case is VC_BAR itself


def test_a_late_hand_off_would_show(table):
    below = {name: row for name, row in table.items() if row["ratio"] < sv.THRESHOLD}
    visible = [name for name, row in below.items() if row["ldlt"] > 10 * VC_BAR]
    assert len(visible) >= 3, {name: row["ldlt"] for name, row in below.items()}


def test_the_sweep_the_threshold_comes_from(table):
    """Where LDL^T has to hand over for its twists to keep the bar with a margin: 10 x the largest pivot ratio at which forced fp64
    LDL^T misses VC_BAR / 10, over every case and over solve_cases.threshold_sweep (eight focal lengths per decade for each focal
    construction).  The threshold is not below that; DESIGN.md §5 quotes this sweep."""
    rows = [(row["ratio"], name, row["ldlt"]) for name, row in table.items()]
    for name, L, e in sc.threshold_sweep():
        rows.append((sv.pivot_ratio(L), name, sv.rel_l2(sv.ldlt_solution(L, e), sv.exact_solution(L, e))))
    worst = max(ratio for ratio, _, err in rows if err > VC_BAR / 10)
    for ratio, name, err in sorted(rows, reverse=True):
        print(f"{name:32s} pivot ratio {ratio:.2e}  forced LDL^T {err:.2e}")
    print(f"largest pivot ratio with a forced LDL^T error above {VC_BAR / 10:.0e}: {worst:.2e}")
    assert sv.THRESHOLD >= 10 * worst, (sv.THRESHOLD, worst)
    # and where LDL^T does run, the restatement keeps VC_BAR / 10
    assert all(err <= VC_BAR / 10 for ratio, _, err in rows if ratio > sv.THRESHOLD)
