"""The pose rig law's kernel at its seam (vitvs_op_pose_rig_law: pose_rig.hip on caller-given camera-frame points, no handle, no
forward) against the fp64 numpy statement of tests/pose_rig_ref.py.

Bars (§5f's): v_rig, R, t and the weights <= 1e-9, sigma <= 1e-12, the moments <= 1e-12 relative (of the same sums over the
absolute values of their terms), the status and rig_info exact.  As in tests/test_gpu_pose_op.py every solve of every case is
asserted on the CPU to have a relative eigen-gap >= 1e-6 or, where the case is a degenerate one, <= 1e-10, and every residual to
stay >= 1e-6 away from the rejection edge, so that neither a status nor a zero weight can flip.

Shapes: cameras x rows of 1 x 3, 1 x 4, 2 x 2, 3 x 24, 8 x 24, 2 x 130, 3 x 258 and 5 x 260 (1300 stack rows: past the 1024 one
pass of the 4-per-thread median covers, and past one row per thread), each with N = 0 / 1 / 4 / 16; extrinsics up to 0.5 rad and
0.2 m, rotations up to pi - 1e-3, coplanar clouds, cameras that do not contribute (status != OK, their rows NaN) first / in the
middle / last, nobody contributing, unusable rows first / in the middle / last, odd and even usable counts, tied residuals, fewer
than 3 usable rows, a collinear stack and one that is degenerate only once its outliers are rejected."""
import ctypes as C

import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib

import pose_ref as pr
import pose_rig_ref as rr

gpu = pytest.mark.gpu
LAM = 0.35
N_ITERS = (0, 1, 4, 16)
SMIN = 0.004


def _from_rig(X, rig):
    """Rig-frame points [n_cams, rows, 3] in their cameras' frames."""
    return np.stack([(X[i] - ti) @ Ri for i, (Ri, ti) in enumerate(rig)])


def _case(seed, n_cams, rows, angle, usable=None, status=None, coplanar=False, outliers=0, noise=0.002, ties=0, degenerate=False):
    """A seeded rig and displacement at the given rotation angle; goal points 0.5 - 0.8 m in front of the rig (or on the plane
    z = 0.61 of the rig frame), the current points + noise, `outliers` usable rows of camera 0 moved by 0.1 - 0.4 m, the first
    `ties` usable rows of the last camera repeated in its following `ties` usable rows (equal residuals, bit for bit)."""
    rng = np.random.default_rng(seed)
    rig = rr.seeded_rig(rng, n_cams)
    R, t = rr.seeded_displacement(rng, angle, 0.08)
    Z = np.full((n_cams, rows), 0.61) if coplanar else rng.uniform(0.5, 0.8, (n_cams, rows))
    X = np.stack([rng.uniform(-0.4, 0.4, (n_cams, rows)) * Z, rng.uniform(-0.3, 0.3, (n_cams, rows)) * Z, Z], 2)
    P, Q = rr.camera_points(X, rig, R, t)
    P = P + rng.standard_normal(P.shape) * noise
    usable = np.ones((n_cams, rows), np.int32) if usable is None else np.asarray(usable, np.int32).reshape(n_cams, rows)
    status = np.zeros(n_cams, np.int32) if status is None else np.asarray(status, np.int32)
    if outliers:
        live = np.nonzero(usable[0] > 0)[0]
        bad = rng.choice(live, outliers, replace=False)
        P[0, bad] += np.stack([rr.unit(d) for d in rng.standard_normal((outliers, 3))]) * rng.uniform(0.1, 0.4, (outliers, 1))
    if ties:
        live = np.nonzero(usable[-1] > 0)[0]
        P[-1, live[ties:2 * ties]], Q[-1, live[ties:2 * ties]] = P[-1, live[:ties]], Q[-1, live[:ties]]
    P[usable <= 0], Q[usable <= 0] = 0.0, 0.0
    return dict(P=P, Q=Q, usable=usable, rig=rig, status=status, degenerate=degenerate)


def _line_case(with_outliers):
    """A stack whose points lie on ONE line of the rig frame (3 cameras x 3 rows), or 9 such inliers and one row per camera far off
    the line: a full-rank stack until the re-weighting has thrown the three out."""
    rng = np.random.default_rng(77)
    rig = rr.seeded_rig(rng, 3)
    line = np.outer(np.linspace(-0.3, 0.3, 9), rr.unit([1.0, -1.0, 0.2])) + np.array([0.0, 0.0, 0.6])
    R, t = pr.rodrigues(rr.unit([0.2, 0.5, -0.3]) * 0.5), np.array([0.03, -0.02, 0.04])
    Pr, Qr = pr.points_in_camera(line, R, t).reshape(3, 3, 3), line.reshape(3, 3, 3)
    if with_outliers:
        Po = Pr[:, 0] + np.array([[0.3, 0.2, 0.1], [-0.2, 0.3, 0.2], [0.1, -0.3, 0.25]])
        Qo = Qr[:, 0] + np.array([[-0.2, 0.3, -0.1], [0.3, 0.1, 0.2], [-0.1, -0.2, 0.3]])
        Pr, Qr = np.concatenate([Pr, Po[:, None]], 1), np.concatenate([Qr, Qo[:, None]], 1)
    rows = Pr.shape[1]
    return dict(P=_from_rig(Pr, rig), Q=_from_rig(Qr, rig), usable=np.ones((3, rows), np.int32), rig=rig,
                status=np.zeros(3, np.int32), degenerate=True)


def _cases():
    out = {}
    out["1x3"] = _case(1, 1, 3, 1.0)
    out["1x4_coplanar_near_pi"] = _case(2, 1, 4, np.pi - 1e-3, coplanar=True, noise=0.0)
    out["2x2"] = _case(3, 2, 2, 0.6)
    f24 = np.stack([pr.unusable_flags(24, "first", 5), pr.unusable_flags(24, "middle", 4), pr.unusable_flags(24, "last", 3)])      # 19 + 20 + 21 usable
    out["3x24"] = _case(4, 3, 24, 0.4, f24, outliers=5)
    out["3x24_odd_near_pi"] = _case(5, 3, 24, np.pi - 1e-3, np.stack([pr.unusable_flags(24, "last", 4)] + [np.ones(24, np.int32)] * 2),
                                    coplanar=True)
    out["3x24_odd_near_pi"]["usable"][1, 7] = 0                                                   # 20 + 23 + 24 usable: an odd count
    out["3x24_odd_near_pi"]["P"][1, 7] = out["3x24_odd_near_pi"]["Q"][1, 7] = 0.0
    for where, st in (("first", [2, 0, 0]), ("middle", [0, 1, 0]), ("last", [0, 0, 3])):
        out[f"3x24_out_{where}"] = _case(6, 3, 24, 2.0, f24, status=st, outliers=0 if where == "first" else 4)
    out["3x24_nobody"] = _case(7, 3, 24, 0.5, status=[2, 1, 3])
    out["8x24"] = _case(8, 8, 24, 1.2, status=[0, 0, 0, 2, 0, 0, 0, 0], outliers=8)
    out["2x130_coplanar"] = _case(9, 2, 130, 2.5, np.stack([pr.unusable_flags(130, "middle", 7), pr.unusable_flags(130, "first", 2)]), coplanar=True,
                                  outliers=20)
    out["3x258_ties"] = _case(10, 3, 258, 0.7, np.stack([pr.unusable_flags(258, "first", 2)] * 3), outliers=60, ties=40)
    out["5x260"] = _case(11, 5, 260, 1.3, np.stack([pr.unusable_flags(260, "last", 37)] * 5), outliers=100, ties=3)
    two = np.zeros((3, 24), np.int32)
    two[0, 3], two[2, 20] = 1, 1
    out["3x24_two_usable"] = _case(12, 3, 24, 0.5, two, degenerate=True)
    out["3x3_collinear"] = _line_case(False)
    out["3x4_degenerate_after_rejection"] = _line_case(True)
    return out


CASES = _cases()
_REFS = {}


def _reference(name, n_iter):
    """One fp64 reference per (case, N), computed once and shared."""
    key = (name, n_iter)
    if key not in _REFS:
        c = CASES[name]
        with np.errstate(all="ignore"):
            ref = rr.pose_rig_law(c["P"], c["Q"], c["usable"], c["rig"], c["status"], LAM, n_iter, SMIN)
            Ps, Qs, _, _, _ = rr.stack_points(c["P"], c["Q"], c["usable"], c["rig"], c["status"])
            ref["moments_abs"] = rr.moments(np.abs(Ps), np.abs(Qs), ref["weights"].reshape(-1))
        _REFS[key] = ref
    return _REFS[key]


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_keep_their_margins(name):
    """No GPU: every solve's gap is >= 1e-6 or (degenerate cases only) <= 1e-10; no residual within 1e-6 of the rejection edge."""
    for n_iter in N_ITERS:
        ref = _reference(name, n_iter)
        for g in ref["gaps"]:
            assert g >= 1e-6 or (CASES[name]["degenerate"] and g <= 1e-10), (name, n_iter, ref["gaps"])
        assert ref["edge"] >= 1e-6, (name, n_iter, ref["edge"])
        if name == "3x24_nobody":
            assert ref["status"] == 3 and list(ref["info"]) == [0, 0, 0, 0, 0, 0, 0, 3]
        elif not CASES[name]["degenerate"]:
            assert ref["status"] == pr.OK and ref["info"][3] == n_iter
    if name == "3x4_degenerate_after_rejection":
        assert _reference(name, 0)["status"] == pr.OK
        last = _reference(name, 16)
        assert last["status"] == pr.TOO_FEW and last["info"][5] == 1 and last["info"][4] >= 3
    if name == "3x24_two_usable":
        assert all(_reference(name, n)["status"] == pr.TOO_FEW and _reference(name, n)["info"][5] == 0 for n in N_ITERS)
    if name == "3x3_collinear":
        assert all(_reference(name, n)["status"] == pr.TOO_FEW and _reference(name, n)["info"][5] == 1 for n in N_ITERS)
    if name == "3x258_ties":
        assert _reference(name, 4)["info"][4] >= 60
    if name == "3x24_odd_near_pi":
        assert _reference(name, 0)["info"][1] == 67
    if name.startswith("3x24_out_"):
        assert list(_reference(name, 4)["info"][[0, 7]]) == [2, max(CASES[name]["status"])]


class _Op:
    """The op's device buffers for n cameras of ld rows."""

    def __init__(self, n, ld):
        self.lib, self.dev, self.n, self.ld = _lib.load(), torch.device("cuda", 0), n, ld
        f64 = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=self.dev)   # noqa: E731
        self.P, self.Q, self.rtc = f64(n, ld, 3), f64(n, ld, 3), f64(n, 12)
        self.usable = torch.zeros((n, ld), dtype=torch.int32, device=self.dev)
        self.cam = torch.zeros(n, dtype=torch.int32, device=self.dev)
        self.scratch = torch.zeros(self.lib.vitvs_op_pose_rig_scratch_bytes(n, ld), dtype=torch.uint8, device=self.dev)
        self.v, self.pose, self.moments, self.weights, self.sigma = f64(6), f64(12), f64(18), f64(n, ld), f64(1)
        self.st = torch.full((1,), -1, dtype=torch.int32, device=self.dev)
        self.info = torch.full((8,), -1, dtype=torch.int32, device=self.dev)

    def load(self, case):
        P, Q = case["P"].copy(), case["Q"].copy()
        dead = (case["usable"] <= 0) | (case["status"] != 0)[:, None]
        P[dead] = np.nan                                        # what an unusable row or a camera that does not contribute holds
        Q[dead] = np.nan                                        # must never reach a sum
        self.P.copy_(torch.from_numpy(P))
        self.Q.copy_(torch.from_numpy(Q))
        self.usable.copy_(torch.from_numpy(case["usable"]))
        self.cam.copy_(torch.from_numpy(case["status"]))
        self.rtc.copy_(torch.from_numpy(rr.rtc_rows(case["rig"])))
        return self

    def call(self, n_iter, smin=SMIN, outputs=True, cam=True):
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        opt = (lambda t: p(t)) if outputs else (lambda t: None)
        return self.lib.vitvs_op_pose_rig_law(self.n, self.ld, p(self.P), p(self.Q), p(self.usable), p(self.rtc),
                                              p(self.cam) if cam else None, LAM, n_iter, smin, p(self.scratch), p(self.v), p(self.st),
                                              opt(self.pose), opt(self.info), opt(self.moments), opt(self.weights), opt(self.sigma),
                                              C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream))

    def results(self):
        pose = self.pose.cpu().numpy()
        return dict(v=self.v.cpu().numpy(), status=int(self.st.cpu()[0]), R=pose[:9].reshape(3, 3), t=pose[9:],
                    info=self.info.cpu().numpy(), weights=self.weights.cpu().numpy(), sigma=float(self.sigma.cpu()[0]),
                    moments=self.moments.cpu().numpy())


def _compare(got, ref, tag):
    where = f"{tag} (gaps {['%.2e' % g for g in ref['gaps']]})"
    assert got["status"] == ref["status"], where
    assert np.array_equal(got["info"], ref["info"]), (where, got["info"], ref["info"])
    for key in ("v", "R", "t", "weights"):
        err = float(np.abs(got[key] - ref[key]).max())
        assert err <= 1e-9, (where, key, err)
    assert abs(got["sigma"] - ref["sigma"]) <= 1e-12, (where, got["sigma"], ref["sigma"])
    if "moments_abs" in ref:
        assert (np.abs(got["moments"] - ref["moments"]) <= 1e-12 * ref["moments_abs"]).all(), (where, got["moments"], ref["moments"])


@gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_equals_the_reference(name):
    case = CASES[name]
    op = _Op(*case["usable"].shape).load(case)
    for n_iter in N_ITERS:
        assert op.call(n_iter) == 0
        _compare(op.results(), _reference(name, n_iter), f"{name} N={n_iter}")


@gpu
def test_a_null_camera_status_means_all_ok():
    case = CASES["3x24"]
    op = _Op(3, 24).load(case)
    op.cam.fill_(2)                                             # not read
    assert op.call(4, cam=False) == 0
    _compare(op.results(), _reference("3x24", 4), "cam_status NULL")


@gpu
def test_ten_runs_have_equal_bits():
    for name in ("3x24", "5x260"):
        case = CASES[name]
        op = _Op(*case["usable"].shape).load(case)
        first = None
        for _ in range(10):
            assert op.call(4) == 0
            got = op.results()
            first = first or got
            for key in ("v", "R", "t", "weights", "sigma", "info", "status", "moments"):
                assert np.array_equal(got[key], first[key], equal_nan=True), (name, key)


@gpu
def test_twelve_calls_back_to_back():
    """The same inputs' addresses and ONE scratch block, no synchronisation between the calls: every call's stack is rewritten by
    the next."""
    names = ["3x24", "3x24_out_middle", "3x24_two_usable", "3x24_nobody"] * 3
    ops = [_Op(3, 24) for _ in names]                          # outputs of their own
    shared = ops[0]
    stage = [_Op(3, 24).load(CASES[name]) for name in names]
    for k, src in enumerate(stage):
        op = ops[k]
        for key in ("P", "Q", "usable", "cam", "rtc"):
            getattr(shared, key).copy_(getattr(src, key))
            setattr(op, key, getattr(shared, key))
        op.scratch = shared.scratch
        assert op.call(4 if k % 2 else 0) == 0
    torch.cuda.synchronize()
    for k, name in enumerate(names):
        _compare(ops[k].results(), _reference(name, 4 if k % 2 else 0), f"call {k} {name}")


@gpu
def test_captured_graph_replays():
    op = _Op(3, 24).load(CASES["3x24"])
    assert op.call(4) == 0                                      # (warm-up outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert op.call(4) == 0
    for _ in range(2):
        op.v.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        _compare(op.results(), _reference("3x24", 4), "replay")
    # new points, poses and statuses at the same addresses: the replay reads them
    op.load(CASES["3x24_out_last"])
    graph.replay()
    torch.cuda.synchronize()
    _compare(op.results(), _reference("3x24_out_last", 4), "replay on new points")


@gpu
def test_null_outputs_and_error_returns():
    op = _Op(3, 24).load(CASES["3x24"])
    assert op.call(4, outputs=False) == 0
    torch.cuda.synchronize()
    ref = _reference("3x24", 4)
    assert np.abs(op.v.cpu().numpy() - ref["v"]).max() <= 1e-9 and int(op.st.cpu()[0]) == ref["status"]
    assert torch.isnan(op.pose).all() and (op.info == -1).all() and torch.isnan(op.weights).all() and torch.isnan(op.sigma).all()
    assert torch.isnan(op.moments).all()
    nobody = _Op(3, 24).load(CASES["3x24_nobody"])             # the early exit with NULL outputs
    assert nobody.call(4, outputs=False) == 0
    torch.cuda.synchronize()
    assert int(nobody.st.cpu()[0]) == 3 and not nobody.v.cpu().numpy().any() and torch.isnan(nobody.pose).all()
    lib, p = op.lib, lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    args = lambda **kw: [kw.get("n", 3), kw.get("ld", 24), kw.get("P", p(op.P)), kw.get("Q", p(op.Q)), kw.get("u", p(op.usable)),   # noqa: E731
                         kw.get("rtc", p(op.rtc)), None, LAM, kw.get("N", 4), SMIN, kw.get("s", p(op.scratch)), kw.get("v", p(op.v)),
                         kw.get("st", p(op.st)), None, None, None, None, None, None]
    for missing in ("P", "Q", "u", "rtc", "s", "v", "st"):
        assert lib.vitvs_op_pose_rig_law(*args(**{missing: None})) == -1, missing
    for bad in (dict(n=0), dict(ld=0), dict(N=-1), dict(N=17)):
        assert lib.vitvs_op_pose_rig_law(*args(**bad)) == -2, bad
    assert lib.vitvs_op_pose_rig_law(*args(n=8, ld=2000, N=1)) == -3   # the plan's: rho and w of 16000 rows are past 160 KiB of LDS


@gpu
def test_the_pose_law_keeps_its_bits():
    """vitvs_op_pose_law (pose.hip, which runs pose_core.h's pose_align as the rig law does) before and after the rig law's
    launches."""
    import test_gpu_pose_op as single
    case = single.CASES["3x24"]
    one = single._Op(3, 24).load(case)
    assert one.call(4) == 0
    before = one.results()
    rig = _Op(5, 260).load(CASES["5x260"])
    assert rig.call(4) == 0 and rig.call(0) == 0
    assert one.call(4) == 0
    after = one.results()
    for key in before:
        assert np.array_equal(before[key], after[key], equal_nan=True), key
    single._compare(after, single._reference("3x24", 4), "the pose law beside the rig law")


# (case of tests/test_gpu_pose_op.py, its pair): 3 rows, <= 256 rows with unusable rows and outliers, > 256 rows with ties
_ONE_CAMERA = (("1x3", 0), ("3x24", 0), ("1x130_coplanar", 0), ("1x258_ties", 0))


def _one_camera_case(name, pair):
    import test_gpu_pose_op as single
    c = single.CASES[name]
    return dict(P=c["P"][pair:pair + 1], Q=c["Q"][pair:pair + 1], usable=c["usable"][pair:pair + 1],
                rig=[(np.eye(3), np.zeros(3))], status=np.zeros(1, np.int32), degenerate=c["degenerate"])


@pytest.mark.parametrize("name,pair", _ONE_CAMERA)
def test_one_camera_cases_make_the_identity_exact(name, pair):
    """No GPU: ((1 p0 + 0 p1) + 0 p2) + 0 is p0 bit for bit only for a finite p0 that is not +-0 (and finite p1, p2)."""
    c = _one_camera_case(name, pair)
    live = c["usable"][0] > 0
    assert live.sum() >= 3
    for X in (c["P"][0][live], c["Q"][0][live]):
        assert np.isfinite(X).all() and (X != 0.0).all(), name


@gpu
@pytest.mark.parametrize("name,pair", _ONE_CAMERA)
def test_a_one_camera_rig_at_the_identity_has_the_pose_laws_bits(name, pair):
    """One camera with rTc = (I, 0): the rig frame is the camera's frame and the stack is the pose law's point block, bit for bit,
    so pose_rig_kernel and pose_kernel run pose_align on the same numbers.  v, R, t, the weights, sigma and the shared info fields
    (usable rows, sweeps, re-weightings, zero weights, degenerate, holes) must be EQUAL for N = 0, 4 and 16."""
    import test_gpu_pose_op as single
    c = _one_camera_case(name, pair)
    live = c["usable"][0] > 0
    for X in (c["P"][0][live], c["Q"][0][live]):                # (before the GPU is touched)
        assert np.isfinite(X).all() and (X != 0.0).all(), name
    ld = c["usable"].shape[1]
    one = single._Op(1, ld).load(c)
    rig = _Op(1, ld).load(c)
    for n_iter in (0, 4, 16):
        assert one.call(n_iter) == 0 and rig.call(n_iter) == 0
        a, b = one.results(), rig.results()
        tag = f"{name} N={n_iter}"
        assert a["status"][0] == b["status"], tag
        for key in ("v", "R", "t", "weights", "sigma"):
            assert np.array_equal(np.asarray(a[key][0]), np.asarray(b[key]).reshape(np.shape(a[key][0]))), (tag, key, a[key][0], b[key])
        assert np.array_equal(a["info"][0][:6], b["info"][1:7]), (tag, a["info"][0], b["info"])
        assert b["info"][0] == 1 and b["info"][7] == 0, (tag, b["info"])
