"""The control laws' 6 x 6 solve across the hand-off from LDL^T to the Jacobi SVD (solve.h, servo.hip's inline copy), on the GPU
against a 50-digit solution of the device's own system.

The suite elsewhere meets this solver at cond(L) < 1e3 or at exact rank deficiency.  The cases of tests/solve_cases.py lie in
between, on both sides of the pivot test ``d > THRESHOLD G_jj`` (tests/test_solve_host.py pins, on the CPU, that they crowd the
threshold, keep a factor 2 away from it, and that a late hand-off would show).  Per case: the status, R and the weights' count;
which solver ran (info[4]; the rig's info[2]) against ``solve_ref.pivot_ratio`` of the device's own system; the device's L and e
against the oracle's within 1e-13; and the twist against ``solve_ref.exact_solution`` of THE DEVICE'S OWN L, e (with the weights
the device reports, for the robust law), so that the number is the solver's alone.  The bar is
max(1e-9, 8 x the error of numpy.linalg.pinv on the same system): the project's bar wherever fp64 pinv itself can judge it, and a
small fixed multiple of LAPACK's own error where the conditioning puts that past 1e-9 (one-sided Jacobi and LAPACK's SVD are both
backward-stable orthogonal methods; the factor 8 was set in advance, not measured).

Each case records pivot ratio, cond(L), solver, the device's error and pinv's as junit properties
(`--junitxml=FILE -o junit_family=legacy`).

Worst device error per family and solver, measured on an MI355X (cases; worst error, where; LDL^T | Jacobi):

    family         LDL^T                                      Jacobi
    focal_flat      4   2.6e-13  f 1110 px,  ratio 5.9e-4      15  2.0e-9   f 6e5 px, cond 2.8e7 (pinv 3.4e-9)
    focal_tilted   12   1.2e-12  5 %, f 6000, ratio 2.3e-4      3  2.9e-14
    cluster         6   1.6e-12  corner 3 x 3, ratio 2.2e-4     6  1.4e-13
    collinear       4   1.0e-13  (ratio 2e-3 at every offset: with varied depth a line of features is not degenerate)
    many_rows       1   1.2e-12  ratio 2.0e-4                   1  1.0e-14
    weighted        2   5.3e-13  ratio 6.0e-4                   2  1.8e-14
    rig             2   2.5e-13  ratio 3.0e-4                   2  1.7e-13
    (Jacobi on focal_flat up to cond(L) 2.8e6: 6.3e-11 at most, and below pinv's own error from cond(L) 1.6e3 on)

With the threshold at 1e-8, where it was when this module was written, the same families (the sweep's gap and the straddling
cases placed around 1e-8) measured, LDL^T just above the hand-off | Jacobi just below it:

    focal_flat     f 14.6e3 px, ratio 2.05e-8, cond 1.6e4:  2.3e-9 (fails)    |  f 25.8e3 px:  3.3e-12
    many_rows      ratio 2.2e-8:                             2.0e-9 (fails)    |  6.5e-13
    weighted       robust_law 1: 7.7e-9, 4: 2.0e-8 (fail)                      |  3.0e-12, 1.9e-12
    rig            ratio 2.06e-8, cond 1.8e5:                9.1e-7 (fails)    |  2.9e-12
    LDL^T further up: 8.9e-10 at ratio 6.4e-8, 6.0e-10 at 2.0e-7, 1.2e-10 at 2.0e-6, 3.0e-11 at 6.2e-6, 5.4e-12 at 2.0e-5,
    2.8e-12 at 6.1e-5, 9.5e-13 at 1.9e-4: about 5e-17 / ratio, a third of what the fp64 restatement on the CPU predicts
    (1.6e-8 at 2.05e-8), which named the right place and the right order of magnitude.

That measurement moved the threshold to 1e-4.  The module's 58 tests take 3 s.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib
import law_support as ls
from law_support import TinyEngines, close_engines  # noqa: F401
import solve_cases as sc
import solve_ref as sv

pytestmark = pytest.mark.gpu

ENGINES = TinyEngines()           # this module's tiny handles: close_engines closes them at its teardown

LDLT = -1
MAX_SWEEPS = 40
VC_BAR, L_BAR = 1e-9, 1e-13
PINV_FACTOR = 8


def _judge(name, family, record_property, L, e, v, lam, sweeps):
    """The solver that ran and the twist's error, for the system (L, e) the device solved."""
    ratio, cond = sv.pivot_ratio(L), float(np.linalg.cond(L))
    assert not (sv.THRESHOLD / sc.GUARD < ratio < sv.THRESHOLD * sc.GUARD), (name, "inside the guard band", ratio)
    x = sv.exact_solution(L, e)
    err = sv.rel_l2(v, -lam * x)
    pinv_err = sv.rel_l2(sv.pinv_solution(L, e), x)
    solver = "ldlt" if sweeps == LDLT else "jacobi"
    for key, value in (("family", family), ("pivot_ratio", ratio), ("cond", cond), ("solver", solver), ("sweeps", sweeps),
                       ("device_error", err), ("pinv_error", pinv_err)):
        record_property(key, value)
    print(f"{name}: family {family} pivot ratio {ratio:.2e} cond {cond:.2e} solver {solver} sweeps {sweeps} "
          f"device error {err:.2e} pinv error {pinv_err:.2e}")
    if ratio > sv.THRESHOLD:
        assert sweeps == LDLT, (name, "expected LDL^T", ratio, sweeps)
    else:
        assert 0 <= sweeps <= MAX_SWEEPS, (name, "expected Jacobi", ratio, sweeps)
    assert err <= max(VC_BAR, PINV_FACTOR * pinv_err), (name, solver, ratio, err, pinv_err)


@pytest.mark.parametrize("name", [c.name for c in sc.CASES])
def test_camera_law_across_the_hand_off(name, record_property):
    c = sc.BY_NAME[name]
    eng, params = ENGINES.fetch(c.g, c.max_rows, reset=ls.LAW_OPTIONS)
    eng.set_option("robust_law", c.robust)
    nn1, nn2, sim1, ids, K = sc.tables(c)
    rows = c.num_pairs
    v, st = eng.servo_from_nn(nn1, nn2, sim1, sc.depth_image(c.depth), K, mode=_lib.SELECT_EXPLICIT, selection=[ids], num_pairs=rows)
    det = eng.last_details(1)
    eng.set_option("robust_law", 0)
    want = sc.system(c)
    info = det["info"][0]
    assert int(st) == _lib.STATUS_OK, (name, int(st))
    assert int(info[5]) == 2 * rows and int(info[3]) == rows and int(info[6]) == c.robust, (name, info)
    assert det["selected"][0, :rows].tolist() == ids.tolist(), name
    suv = det["s_uv"][0, :rows]
    assert np.array_equal(suv[:, 0:2], want["s_star"]) and np.array_equal(suv[:, 2:4], want["s_"]), name
    L, e = det["L"][0, :6, :2 * rows].T, det["L"][0, 6, :2 * rows]
    np.testing.assert_allclose(L, want["L"], rtol=0, atol=L_BAR, err_msg=name)
    np.testing.assert_allclose(e, want["e"], rtol=0, atol=L_BAR, err_msg=name)
    w = det["weights"][0, :rows]
    if c.robust:
        assert 0 < np.count_nonzero(w) and np.ptp(w) > 0 and int(info[7]) == np.count_nonzero(w == 0), (name, info)
    else:
        assert np.all(w == 1.0), name
    sw = np.sqrt(np.repeat(w, 2))
    _judge(name, c.family, record_property, sw[:, None] * L, sw * e, v.cpu().numpy(), params.lambda_, int(info[4]))


@pytest.mark.parametrize("name", list(sc.RIG_CASES))
def test_rig_law_across_the_hand_off(name, record_property):
    """rig.hip calls the same solve_ldlt and solve_jacobi on the stack of the cameras' rows: through vitvs_op_rig_law, which takes
    the rows directly, as one launch and as the two plain launches of vitvs_op_rig_two_launches (the same bits)."""
    case = sc.RIG_CASES[name]
    lib, dev = _lib.load(), torch.device("cuda", 0)
    n, ld = len(case["Ls"]), case["ld"]
    packed = np.zeros((n, 7, ld))
    for i, (L, e) in enumerate(zip(case["Ls"], case["es"])):
        assert L.shape == (ld, 6)
        packed[i, :6], packed[i, 6] = L.T, e
    rows = torch.full((n,), ld, dtype=torch.int32, device=dev)
    L_d = torch.as_tensor(packed).to(dev)
    W_d = torch.as_tensor(np.stack([W.reshape(36) for W in case["Ws"]])).to(dev)
    scratch = torch.zeros(lib.vitvs_op_rig_scratch_bytes(n, ld), dtype=torch.uint8, device=dev)
    M, e = sc.rig_system(case)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    outs = []
    for two in (0, 1):
        v = torch.full((6,), np.nan, dtype=torch.float64, device=dev)
        st = torch.full((9,), -7, dtype=torch.int32, device=dev)                     # rig_status | rig_info [8]
        assert lib.vitvs_op_rig_two_launches(two) == 0
        try:
            rc = lib.vitvs_op_rig_law(n, p(rows), p(L_d), ld, p(W_d), case["lam"], p(scratch), p(v), p(st), p(st[1:]), None,
                                      C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        finally:
            assert lib.vitvs_op_rig_two_launches(0) == two
        assert rc == 0, rc
        st = st.cpu().numpy()
        assert int(st[0]) == 0 and (int(st[1]), int(st[2])) == (n, n * ld), (name, st)
        outs.append((v.cpu().numpy(), int(st[3])))
        _judge(f"{name}, {'two launches' if two else 'one launch'}", "rig", record_property, M, e, outs[-1][0], case["lam"], outs[-1][1])
    assert np.array_equal(outs[0][0].view(np.int64), outs[1][0].view(np.int64)) and outs[0][1] == outs[1][1], name
