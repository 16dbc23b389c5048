"""The rig law's kernel at its seam (vitvs_op_rig_law: rig.hip on caller systems, no handle, no forward) against the fp64 numpy
statement of tests/rig_ref.py.  Bars: v_rig <= 1e-9 relative L2 (the project's bar for v_c); the normal equations within
1e-12 sqrt(G_aa G_bb) of numpy's M^T M (n 2^-53 at the largest case's 4096 rows is 4.6e-13); statuses, counts and the solver
exact.  The shapes are the smallest at which each mechanism can fail: 1, 2, 3, 8 and 9 cameras (at 9 two workgroups share an
XCD: the fan-in meets both placements), 2 / 4 / 48 / 130 / 258 rows per camera (one pair; the < 4 region; the usual 24 pairs;
past 128 rows; past one row per thread), one 2 x 2048-row case, mixed counts with an empty camera first, in the middle and last
(the prefix offsets, the camera-order sum), both solvers, nobody contributing, the same buffers reused back to back (the
hand-off's stale-line case) and determinism.  Every case names the solver its fp64 reference takes and keeps the reference's own
LDL^T pivots >= 100 x away from the pivot test (solve_ref.THRESHOLD) on either side (checked on the CPU by the first test)."""
import ctypes as C

import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib

import rig_ref as rg

gpu = pytest.mark.gpu
LAM = 0.35
COUNTS = (1, 2, 3, 8, 9)
ROWS = (2, 4, 48, 130, 258)


def _system(rng, rows):
    return rg.camera_system(rng, (rows + 1) // 2)[:rows] if rows else np.zeros((0, 6))


def _consistent_e(rng, Ls, Ws, noise=1e-3):
    v_star = rng.standard_normal(6)
    return [L @ W @ v_star + noise * rng.standard_normal(L.shape[0]) for L, W in zip(Ls, Ws)]


def _random_case(seed, rows_per_cam, ld=None):
    rng = np.random.default_rng(seed)
    n = len(rows_per_cam)
    Ws = [rg.twist_matrix(*rg.random_extrinsic(rng)) for _ in range(n)]
    Ls = [_system(rng, r) for r in rows_per_cam]
    return dict(Ls=Ls, es=_consistent_e(rng, Ls, Ws), Ws=Ws, ld=ld or max(max(rows_per_cam), 1))


def _cases():
    """name -> (case, the solver its reference takes: 'ldlt' / 'jacobi' / 'none')"""
    out = {}
    for n in COUNTS:
        for r in ROWS:
            # fewer than 6 rows in all cannot have rank 6: those stacks are the rank-deficient end of the grid
            out[f"{n}x{r}"] = (_random_case(1000 * n + r, [r] * n), "jacobi" if n * r < 6 else "ldlt")
    out["2x2048"] = (_random_case(77, [2048, 2048]), "ldlt")
    out["mixed_empty_first"] = (_random_case(78, [0, 48, 130, 2, 258, 7, 48, 4, 48], ld=260), "ldlt")
    out["mixed_empty_middle"] = (_random_case(79, [258, 4, 0, 0, 48, 130, 2, 9], ld=258), "ldlt")
    out["mixed_empty_last"] = (_random_case(80, [130, 48, 0], ld=136), "ldlt")
    # rank-deficient stacks: one camera with 2 pairs at the rig origin (rank 4)
    rng = np.random.default_rng(81)
    L = _system(rng, 4)
    out["one_camera_two_pairs"] = (dict(Ls=[L], es=[0.05 * rng.standard_normal(4)], Ws=[np.eye(6)], ld=8), "jacobi")
    # ... every camera 47 all-zero padded rows and one live row (rank <= 3)
    rng = np.random.default_rng(82)
    Ls, es = [], []
    for _ in range(3):
        L = np.zeros((48, 6))
        L[0] = _system(rng, 2)[0]
        e = np.zeros(48)
        e[0] = 0.05 * rng.standard_normal()
        Ls.append(L)
        es.append(e)
    out["padded_rows_one_live"] = (dict(Ls=Ls, es=es, Ws=[rg.twist_matrix(*rg.random_extrinsic(rng)) for _ in range(3)], ld=48), "jacobi")
    # ... 3 cameras x 2 pairs with equal extrinsics seeing the same two features: the stack repeats one camera's 4 rows (rank 4)
    rng = np.random.default_rng(83)
    W = rg.twist_matrix(*rg.random_extrinsic(rng))
    L = _system(rng, 4)
    e = 0.05 * rng.standard_normal(4)
    out["three_equal_cameras"] = (dict(Ls=[L] * 3, es=[e] * 3, Ws=[W] * 3, ld=4), "jacobi")
    # ... and with equal extrinsics but features of their own: six points, full rank
    rng = np.random.default_rng(84)
    Ls = [_system(rng, 4) for _ in range(3)]
    out["three_cameras_equal_extrinsics"] = (dict(Ls=Ls, es=_consistent_e(rng, Ls, [W] * 3), Ws=[W] * 3, ld=4), "ldlt")
    out["nobody"] = (_random_case(85, [0, 0, 0], ld=16), "none")
    return out


CASES = _cases()


def _reference(case):
    return rg.rig_law(case["Ls"], case["es"], case["Ws"], rg.statuses(case), LAM)


def _pack(case):
    """(rows int32 [n], L float64 [n][7][ld] column-major, W float64 [n][36]) as the op takes them."""
    n, ld = len(case["Ls"]), case["ld"]
    rows = np.array([L.shape[0] for L in case["Ls"]], np.int32)
    Lp = np.full((n, 7, ld), np.nan)                                # rows a camera does not have must never be read
    for i, (L, e) in enumerate(zip(case["Ls"], case["es"])):
        Lp[i, :6, :rows[i]] = L.T
        Lp[i, 6, :rows[i]] = e
    return rows, Lp, np.stack([np.asarray(W).reshape(36) for W in case["Ws"]])


def _back_to_back_cases(n=9, ld=140):
    """12 systems for the same buffers: other rows per camera each time, every third one nine equal cameras of two pairs (rank 4)."""
    rng = np.random.default_rng(90)
    cases = []
    for k in range(12):
        if k % 3 == 2:
            W = rg.twist_matrix(*rg.random_extrinsic(rng))
            L = _system(rng, 4)
            e = 0.05 * rng.standard_normal(4)
            cases.append(dict(Ls=[L] * n, es=[e] * n, Ws=[W] * n, ld=ld))
        else:
            cases.append(_random_case(900 + k, [int(r) for r in rng.choice([0, 2, 4, 48, 130, 136], size=n)], ld=ld))
    return cases


def test_every_case_is_a_fair_test_of_the_solver_it_names():
    for k, case in enumerate(_back_to_back_cases()):
        margin = rg.ldlt_margin(_reference(case)["M"])
        assert (margin <= 0.01) if k % 3 == 2 else (margin >= 100), (k, margin)
    for name, (case, solver) in CASES.items():
        ref = _reference(case)
        if solver == "none":
            assert ref["rows"] == 0, name
            continue
        margin = rg.ldlt_margin(ref["M"])
        assert (margin >= 100) if solver == "ldlt" else (margin <= 0.01), (name, solver, margin)


class Op:
    """Device buffers for one geometry (n_cams, ld) and the call."""

    def __init__(self, n, ld, dev):
        self.lib, self.n, self.ld, self.dev = _lib.load(), n, ld, dev
        nbytes = self.lib.vitvs_op_rig_scratch_bytes(n, ld)
        assert nbytes == 256 + 8 * (32 * n + 14 * n * ld)
        self.scratch = torch.zeros(nbytes, dtype=torch.uint8, device=dev)          # zeroed once, before the first call only
        self.rows = torch.zeros(n, dtype=torch.int32, device=dev)
        self.L = torch.zeros((n, 7, ld), dtype=torch.float64, device=dev)
        self.W = torch.zeros((n, 36), dtype=torch.float64, device=dev)
        self.v = torch.full((6,), np.nan, dtype=torch.float64, device=dev)
        self.st = torch.full((9,), -7, dtype=torch.int32, device=dev)             # rig_status | rig_info [8]
        self.normal = torch.full((28,), np.nan, dtype=torch.float64, device=dev)

    def load(self, rows, Lp, W):
        self.rows.copy_(torch.as_tensor(rows))
        self.L.copy_(torch.as_tensor(Lp))
        self.W.copy_(torch.as_tensor(W))

    def call(self):
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        rc = self.lib.vitvs_op_rig_law(self.n, p(self.rows), p(self.L), self.ld, p(self.W), LAM, p(self.scratch), p(self.v),
                                       p(self.st), p(self.st[1:]), p(self.normal),
                                       C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream))
        assert rc == 0, rc

    def results(self):
        st = self.st.cpu().numpy()
        return dict(v=self.v.cpu().numpy(), status=int(st[0]), info=st[1:], normal=self.normal.cpu().numpy())


def _check(name, got, ref, solver):
    info = got["info"]
    assert got["status"] == ref["status"], (name, got["status"], ref["status"])
    assert (int(info[0]), int(info[1])) == (ref["cameras"], ref["rows"]), (name, info)
    assert not info[5:].any(), (name, info)
    if solver == "none":
        assert np.array_equal(got["v"], np.zeros(6)) and int(info[2]) == 0, (name, got["v"], info)
        assert not got["normal"].any(), name
        return 0.0
    assert (int(info[2]) == -1) if solver == "ldlt" else (0 <= int(info[2]) <= 40), (name, solver, info)
    want = rg.normal_packed(ref["M"], ref["e"])
    G = ref["G"]
    scale = np.sqrt(np.diag(G))
    bound = np.concatenate([np.outer(scale, scale)[np.triu_indices(6)], scale * np.linalg.norm(ref["e"]), [0.0]]) * 1e-12
    assert (np.abs(got["normal"] - want) <= bound).all(), (name, np.abs(got["normal"] - want), bound)
    err = float(np.linalg.norm(got["v"] - ref["v_rig"]) / np.linalg.norm(ref["v_rig"]))
    assert err <= 1e-9, (name, err, got["v"], ref["v_rig"])
    return err


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_op_equals_the_reference(name):
    case, solver = CASES[name]
    dev = torch.device("cuda", 0)
    op = Op(len(case["Ls"]), case["ld"], dev)
    op.load(*_pack(case))
    op.call()
    err = _check(name, op.results(), _reference(case), solver)
    print(f"{name}: {solver}, sweeps {int(op.results()['info'][2])}, v_rig rel err {err:.2e}")


@gpu
def test_optional_outputs_may_be_null_and_bad_arguments_are_refused():
    case, _ = CASES["3x48"]
    dev = torch.device("cuda", 0)
    op = Op(3, 48, dev)
    op.load(*_pack(case))
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    lib = op.lib
    assert lib.vitvs_op_rig_law(3, p(op.rows), p(op.L), 48, p(op.W), LAM, p(op.scratch), p(op.v), p(op.st), None, None, None) == 0
    torch.cuda.synchronize()
    ref = _reference(case)
    assert np.linalg.norm(op.v.cpu().numpy() - ref["v_rig"]) <= 1e-9 * np.linalg.norm(ref["v_rig"])
    assert int(op.st[0]) == 0 and int(op.st[1]) == -7 and bool(torch.isnan(op.normal).all())       # untouched
    assert lib.vitvs_op_rig_law(3, None, p(op.L), 48, p(op.W), LAM, p(op.scratch), p(op.v), p(op.st), None, None, None) == -1
    assert lib.vitvs_op_rig_law(3, p(op.rows), p(op.L), 48, p(op.W), LAM, None, p(op.v), p(op.st), None, None, None) == -1
    assert lib.vitvs_op_rig_law(0, p(op.rows), p(op.L), 48, p(op.W), LAM, p(op.scratch), p(op.v), p(op.st), None, None, None) == -2
    assert lib.vitvs_op_rig_law(257, p(op.rows), p(op.L), 48, p(op.W), LAM, p(op.scratch), p(op.v), p(op.st), None, None, None) == -2
    assert lib.vitvs_op_rig_law(3, p(op.rows), p(op.L), 0, p(op.W), LAM, p(op.scratch), p(op.v), p(op.st), None, None, None) == -2
    assert lib.vitvs_op_rig_scratch_bytes(0, 48) == -2


@gpu
def test_rows_beyond_ld_are_clamped_and_negative_rows_do_not_contribute():
    """Bounds: whatever the rows array says, no camera reads past its ld rows or writes past the stacked workspace."""
    case, _ = CASES["3x48"]
    dev = torch.device("cuda", 0)
    op = Op(3, 48, dev)
    rows, Lp, W = _pack(case)
    op.load(np.array([4800, -5, 48], np.int32), Lp, W)
    op.call()
    keep = dict(Ls=[case["Ls"][0], np.zeros((0, 6)), case["Ls"][2]], es=[case["es"][0], np.zeros(0), case["es"][2]], Ws=case["Ws"], ld=48)
    _check("clamped", op.results(), _reference(keep), "ldlt")


@gpu
def test_the_same_buffers_with_new_contents_back_to_back():
    """The stale-line case of the hand-off: 12 calls on one stream into the same scratch, inputs and outputs, each with other
    rows per camera (other offsets in the stacked workspace), other contents and, every third call, a rank-deficient stack (the
    Jacobi path reads the stacked rows other workgroups wrote).  No host synchronisation in between; every call equals its own
    reference."""
    dev = torch.device("cuda", 0)
    n, ld = 9, 140
    cases = _back_to_back_cases()
    packed = [[torch.as_tensor(a).to(dev) for a in _pack(c)] for c in cases]
    refs = [_reference(c) for c in cases]
    op = Op(n, ld, dev)
    outs = []
    torch.cuda.synchronize()
    for rows, Lp, W in packed:
        op.rows.copy_(rows)
        op.L.copy_(Lp)
        op.W.copy_(W)
        op.call()
        outs.append((op.v.clone(), op.st.clone(), op.normal.clone()))
    torch.cuda.synchronize()
    for k, ((v, st, normal), ref) in enumerate(zip(outs, refs)):
        st = st.cpu().numpy()
        _check(f"call {k}", dict(v=v.cpu().numpy(), status=int(st[0]), info=st[1:], normal=normal.cpu().numpy()), ref,
               "jacobi" if k % 3 == 2 else "ldlt")
    assert int(op.scratch[:4].view(torch.int32)[0]) == 0             # the ticket is left zero


@gpu
@pytest.mark.parametrize("name", ["mixed_empty_first", "three_equal_cameras"])
def test_bit_reproducible(name):
    """The cameras' sums are added in camera order, not in arrival order: the same inputs give the same bits, 10 times."""
    case, _ = CASES[name]
    dev = torch.device("cuda", 0)
    op = Op(len(case["Ls"]), case["ld"], dev)
    op.load(*_pack(case))
    outs = []
    for _ in range(10):
        op.call()
        outs.append((op.v.clone(), op.normal.clone(), op.st.clone()))
    torch.cuda.synchronize()
    for v, normal, st in outs[1:]:
        assert torch.equal(v.view(torch.int64), outs[0][0].view(torch.int64))
        assert torch.equal(normal.view(torch.int64), outs[0][1].view(torch.int64))
        assert torch.equal(st, outs[0][2])


@gpu
def test_two_plain_launches_give_the_same_bits():
    """The measured alternative to the in-launch fan-in (vitvs_op_rig_two_launches): same kernel code, same order of sums."""
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    for name in ("8x48", "mixed_empty_first", "one_camera_two_pairs"):
        case, _ = CASES[name]
        op = Op(len(case["Ls"]), case["ld"], dev)
        op.load(*_pack(case))
        op.call()
        one = op.results()
        assert lib.vitvs_op_rig_two_launches(1) == 0
        try:
            op.call()
        finally:
            assert lib.vitvs_op_rig_two_launches(0) == 1
        two = op.results()
        assert np.array_equal(one["v"].view(np.int64), two["v"].view(np.int64)), name
        assert np.array_equal(one["normal"].view(np.int64), two["normal"].view(np.int64)) and np.array_equal(one["info"], two["info"])
