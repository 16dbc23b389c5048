"""The pose law's kernel at its seam (vitvs_op_pose_law: pose.hip on caller-given points, no handle, no forward) against the fp64
numpy statement of tests/pose_ref.py.

Bars: v_pose, R, t and the weights <= 1e-9, sigma <= 1e-12, the status and pose_info (usable rows, Jacobi sweeps, re-weightings,
zero weights, degenerate flag, holes) exact.  The 4 x 4 eigenvector is as good as eps / gap: every solve of every case is asserted
on the CPU to have a relative eigen-gap >= 1e-6 (100 x the test's 1e-8) or, where the case is a degenerate one, <= 1e-10, and
every residual to stay >= 1e-6 away from the rejection edge rho = c sigma, so that neither a status nor a zero weight can flip.

Shapes: pairs x rows of 1 x 3 (the fewest rows), 1 x 4, 3 x 24 (several workgroups), 1 x 130, 1 x 258 (past one row per thread)
and 1 x 1100 (past four rows per thread: the median's second pass), each with N = 0 / 1 / 4 / 16 re-weightings; rotations up to
pi - 1e-3, coplanar clouds, unusable rows first / in the middle / last, odd and even usable counts, tied residuals, fewer than 3
usable rows, exactly collinear clouds and a cloud that is degenerate only once its outliers are rejected."""
import ctypes as C

import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib

import pose_ref as pr

gpu = pytest.mark.gpu
LAM = 0.35
N_ITERS = (0, 1, 4, 16)
SMIN = 0.004


def _pair(seed, rows, angle, usable=None, coplanar=False, outliers=0, noise=0.002, ties=0):
    """One pair's (P, Q, usable): a seeded pose at the given rotation angle, Q at 0.5 - 0.8 m (or on the plane z = 0.61),
    P = the same points in the camera + noise, `outliers` usable rows moved by 0.1 - 0.4 m, the first `ties` usable rows repeated in
    the following `ties` usable rows (equal residuals, bit for bit)."""
    rng = np.random.default_rng(seed)
    R, t = pr.rodrigues(pr.unit(rng.standard_normal(3)) * angle), rng.uniform(-0.08, 0.08, 3)
    Z = np.full(rows, 0.61) if coplanar else rng.uniform(0.5, 0.8, rows)
    Q = np.stack([rng.uniform(-0.4, 0.4, rows) * Z, rng.uniform(-0.3, 0.3, rows) * Z, Z], 1)
    P = pr.points_in_camera(Q, R, t) + rng.standard_normal((rows, 3)) * noise
    usable = np.ones(rows, np.int32) if usable is None else np.asarray(usable, np.int32)
    live = np.nonzero(usable > 0)[0]
    if outliers:
        bad = rng.choice(live[2 * ties:], outliers, replace=False)
        P[bad] += np.stack([pr.unit(d) for d in rng.standard_normal((outliers, 3))]) * rng.uniform(0.1, 0.4, (outliers, 1))
    if ties:
        P[live[ties:2 * ties]], Q[live[ties:2 * ties]] = P[live[:ties]], Q[live[:ties]]
    P[usable <= 0], Q[usable <= 0] = 0.0, 0.0
    return P, Q, usable


def _case(*pairs, degenerate=False):
    P, Q, u = (np.stack(x) for x in zip(*pairs))
    return dict(P=P, Q=Q, usable=u, degenerate=degenerate)


def _collinear(rows):
    line = np.outer(np.linspace(-0.3, 0.3, rows), pr.unit([1.0, -1.0, 0.2])) + np.array([0.0, 0.0, 0.6])
    R, t = pr.rodrigues(pr.unit([0.2, 0.5, -0.3]) * 0.5), np.array([0.03, -0.02, 0.04])
    return pr.points_in_camera(line, R, t), line


def _cases():
    out = {}
    out["1x3"] = _case(_pair(1, 3, 1.0))
    out["1x4_coplanar_near_pi"] = _case(_pair(2, 4, np.pi - 1e-3, coplanar=True, noise=0.0))
    out["3x24"] = _case(_pair(3, 24, 0.4, pr.unusable_flags(24, "first", 5), outliers=4),               # 19 usable
                        _pair(4, 24, 2.0, pr.unusable_flags(24, "middle", 4), outliers=3),              # 20 usable
                        _pair(5, 24, np.pi - 1e-3, pr.unusable_flags(24, "last", 3), coplanar=True))    # 21 usable
    out["1x130_coplanar"] = _case(_pair(6, 130, 2.5, pr.unusable_flags(130, "middle", 7), coplanar=True, outliers=20))
    out["1x258_ties"] = _case(_pair(7, 258, 0.7, pr.unusable_flags(258, "first", 2), outliers=30, ties=40))
    out["1x1100"] = _case(_pair(8, 1100, 1.3, pr.unusable_flags(1100, "last", 37), outliers=150, ties=3))
    out["1x24_two_usable"] = _case(_pair(9, 24, 0.5, pr.unusable_flags(24, "first", 22)), degenerate=True)
    P, Q = _collinear(24)
    out["1x24_collinear"] = _case((P, Q, np.ones(24, np.int32)), degenerate=True)
    # 9 collinear inliers and 3 rows far off the line: a full-rank cloud until the re-weighting has thrown the three out
    P, Q = _collinear(9)
    P = np.concatenate([P, P[:3] + np.array([[0.3, 0.2, 0.1], [-0.2, 0.3, 0.2], [0.1, -0.3, 0.25]])])
    Q = np.concatenate([Q, Q[:3] + np.array([[-0.2, 0.3, -0.1], [0.3, 0.1, 0.2], [-0.1, -0.2, 0.3]])])
    out["1x12_degenerate_after_rejection"] = _case((P, Q, np.ones(12, np.int32)), degenerate=True)
    return out


CASES = _cases()
_REFS = {}


def _reference(name, n_iter):
    """One fp64 reference per (case, N), computed once and shared."""
    key = (name, n_iter)
    if key not in _REFS:
        c = CASES[name]
        with np.errstate(all="ignore"):
            _REFS[key] = [pr.pose_law(c["P"][b], c["Q"][b], c["usable"][b], LAM, n_iter, SMIN) for b in range(len(c["P"]))]
    return _REFS[key]


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_keep_their_margins(name):
    """No GPU: every solve's gap is >= 1e-6 or (degenerate cases only) <= 1e-10; no residual within 1e-6 of the rejection edge."""
    for n_iter in N_ITERS:
        for ref in _reference(name, n_iter):
            for g in ref["gaps"]:
                assert g >= 1e-6 or (CASES[name]["degenerate"] and g <= 1e-10), (name, n_iter, ref["gaps"])
            assert ref["edge"] >= 1e-6, (name, n_iter, ref["edge"])
            if not CASES[name]["degenerate"]:
                assert ref["status"] == pr.OK and ref["info"][2] == n_iter
    if name == "1x12_degenerate_after_rejection":
        assert _reference(name, 0)[0]["status"] == pr.OK
        last = _reference(name, 16)[0]
        assert last["status"] == pr.TOO_FEW and last["info"][4] == 1 and last["info"][3] >= 3
    if name == "1x24_two_usable":
        assert all(_reference(name, n)[0]["status"] == pr.TOO_FEW and _reference(name, n)[0]["info"][4] == 0 for n in N_ITERS)
    if name == "1x258_ties":
        assert _reference(name, 4)[0]["info"][3] >= 30


class _Op:
    """The op's device buffers for n pairs of ld rows."""

    def __init__(self, n, ld):
        self.lib, self.dev, self.n, self.ld = _lib.load(), torch.device("cuda", 0), n, ld
        f64 = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=self.dev)   # noqa: E731
        self.P, self.Q = f64(n, ld, 3), f64(n, ld, 3)
        self.usable = torch.zeros((n, ld), dtype=torch.int32, device=self.dev)
        self.scratch = torch.zeros(self.lib.vitvs_op_pose_scratch_bytes(n, ld), dtype=torch.uint8, device=self.dev)
        self.v, self.pose, self.weights, self.sigma = f64(n, 6), f64(n, 12), f64(n, ld), f64(n)
        self.st = torch.full((n,), -1, dtype=torch.int32, device=self.dev)
        self.info = torch.full((n, 8), -1, dtype=torch.int32, device=self.dev)

    def load(self, case):
        P, Q = case["P"].copy(), case["Q"].copy()
        P[case["usable"] <= 0] = np.nan                         # what an unusable row holds must never reach a sum
        Q[case["usable"] <= 0] = np.nan
        self.P.copy_(torch.from_numpy(P))
        self.Q.copy_(torch.from_numpy(Q))
        self.usable.copy_(torch.from_numpy(case["usable"]))
        return self

    def call(self, n_iter, smin=SMIN, outputs=True):
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        opt = (lambda t: p(t)) if outputs else (lambda t: None)
        return self.lib.vitvs_op_pose_law(self.n, self.ld, p(self.P), p(self.Q), p(self.usable), LAM, n_iter, smin, p(self.scratch),
                                          p(self.v), p(self.st), opt(self.pose), opt(self.info), opt(self.weights), opt(self.sigma),
                                          C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream))

    def results(self):
        pose = self.pose.cpu().numpy()
        return dict(v=self.v.cpu().numpy(), status=self.st.cpu().numpy(), R=pose[:, :9].reshape(-1, 3, 3), t=pose[:, 9:],
                    info=self.info.cpu().numpy(), weights=self.weights.cpu().numpy(), sigma=self.sigma.cpu().numpy())


def _compare(got, refs, tag):
    for b, ref in enumerate(refs):
        where = f"{tag} pair {b} (gaps {['%.2e' % g for g in ref['gaps']]})"
        assert got["status"][b] == ref["status"], where
        assert np.array_equal(got["info"][b], ref["info"]), (where, got["info"][b], ref["info"])
        for key in ("v", "R", "t", "weights"):
            err = float(np.abs(got[key][b] - ref[key]).max())
            assert err <= 1e-9, (where, key, err)
        assert abs(got["sigma"][b] - ref["sigma"]) <= 1e-12, (where, got["sigma"][b], ref["sigma"])


@gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_equals_the_reference(name):
    case = CASES[name]
    op = _Op(*case["usable"].shape).load(case)
    for n_iter in N_ITERS:
        assert op.call(n_iter) == 0
        _compare(op.results(), _reference(name, n_iter), f"{name} N={n_iter}")


@gpu
def test_ten_runs_have_equal_bits():
    for name in ("3x24", "1x1100"):
        case = CASES[name]
        op = _Op(*case["usable"].shape).load(case)
        first = None
        for _ in range(10):
            assert op.call(4) == 0
            got = op.results()
            first = first or got
            for key in ("v", "R", "t", "weights", "sigma", "info", "status"):
                assert np.array_equal(got[key], first[key], equal_nan=True), (name, key)


@gpu
def test_twelve_calls_back_to_back():
    """The same buffers, no synchronisation between the calls: every call's workspace rows are rewritten by the next."""
    names = ["3x24", "1x24_collinear", "1x24_two_usable"] * 4
    ops = [_Op(3, 24) for _ in names]                          # outputs of their own, ONE scratch block and one set of inputs
    shared = ops[0]
    stage = []
    for k, name in enumerate(names):
        case = CASES[name]
        n = len(case["P"])
        full = dict(P=np.zeros((3, 24, 3)), Q=np.zeros((3, 24, 3)), usable=np.zeros((3, 24), np.int32))
        for key in full:
            full[key][:n] = case[key]
        stage.append((_Op(3, 24).load(full), n))
    for k, (name, (src, n)) in enumerate(zip(names, stage)):
        op = ops[k]
        shared.P.copy_(src.P)
        shared.Q.copy_(src.Q)
        shared.usable.copy_(src.usable)
        op.P, op.Q, op.usable, op.scratch, op.n = shared.P, shared.Q, shared.usable, shared.scratch, n
        assert op.call(4 if k % 2 else 0) == 0
    torch.cuda.synchronize()
    for k, (name, (src, n)) in enumerate(zip(names, stage)):
        got = {key: val[:n] for key, val in ops[k].results().items()}
        _compare(got, _reference(name, 4 if k % 2 else 0), f"call {k} {name}")


@gpu
def test_captured_graph_replays():
    case = CASES["3x24"]
    op = _Op(3, 24).load(case)
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
    # new points at the same addresses: the replay reads them
    other = _case(_pair(30, 24, 1.1, outliers=3), _pair(31, 24, 0.2), _pair(32, 24, 2.9, coplanar=True))
    op.load(other)
    graph.replay()
    torch.cuda.synchronize()
    with np.errstate(all="ignore"):
        refs = [pr.pose_law(other["P"][b], other["Q"][b], other["usable"][b], LAM, 4, SMIN) for b in range(3)]
    assert all(min(r["gaps"]) >= 1e-6 and r["edge"] >= 1e-6 for r in refs)
    _compare(op.results(), refs, "replay on new points")


@gpu
def test_null_outputs_and_error_returns():
    case = CASES["3x24"]
    op = _Op(3, 24).load(case)
    assert op.call(4, outputs=False) == 0
    torch.cuda.synchronize()
    refs = _reference("3x24", 4)
    assert np.abs(op.v.cpu().numpy() - np.stack([r["v"] for r in refs])).max() <= 1e-9
    assert list(op.st.cpu().numpy()) == [r["status"] for r in refs]
    assert torch.isnan(op.pose).all() and (op.info == -1).all() and torch.isnan(op.weights).all() and torch.isnan(op.sigma).all()
    lib, p = op.lib, lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    args = lambda **kw: [kw.get("n", 3), kw.get("ld", 24), kw.get("P", p(op.P)), kw.get("Q", p(op.Q)), kw.get("u", p(op.usable)),   # noqa: E731
                         LAM, kw.get("N", 4), SMIN, kw.get("s", p(op.scratch)), kw.get("v", p(op.v)), kw.get("st", p(op.st)),
                         None, None, None, None, None]
    for missing in ("P", "Q", "u", "s", "v", "st"):
        assert lib.vitvs_op_pose_law(*args(**{missing: None})) == -1, missing
    for bad in (dict(n=0), dict(ld=0), dict(N=-1), dict(N=17)):
        assert lib.vitvs_op_pose_law(*args(**bad)) == -2, bad
    assert lib.vitvs_op_pose_law(*args(ld=20000, N=1)) == -3    # the plan's: rho and w of 20000 rows are past 160 KiB of LDS
