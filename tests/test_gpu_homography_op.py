"""The homography law's kernel at its seam (vitvs_op_homography_law: homography.hip on caller-given points, no handle, no forward)
against the fp64 numpy statement of tests/homography_ref.py.

Bars: v_h, H and the weights <= 1e-9, sigma <= 1e-12, the status and h_info (usable rows, Jacobi sweeps, re-weightings, zero
weights, degenerate flag, rows mapped behind the camera) exact.  The 9 x 9 eigenvector is as good as eps over the relative gap
behind the smallest eigenvalue: every solve of every case is asserted on the CPU to have its second-smallest eigenvalue >= 1e-4 of
trace(M) (10^4 x the law's 1e-8) or, where the case is a degenerate one, <= 1e-10, and every residual to stay >= 1e-6 away from the
rejection edge rho = c sigma, so that neither a status nor a zero weight can flip.

Shapes: pairs x rows of 1 x 4 (the fewest rows), 1 x 5, 3 x 24 (several workgroups), 1 x 130, 1 x 258 (past one row per thread)
and 1 x 1100 (past four rows per thread: the median's second pass), each with N = 0 / 1 / 4 / 16 re-weightings; unusable rows
first / in the middle / last, odd and even usable counts, tied residuals, a point mapped behind the camera, fewer than 4 usable
rows, exactly collinear sets, a set that is degenerate only once its outliers are rejected, and one whose first fit maps most points
behind the camera (an infinite median)."""
import ctypes as C

import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib

import homography_ref as hr

gpu = pytest.mark.gpu
LAM = 0.35
ZHAT = 0.61
N_ITERS = (0, 1, 4, 16)
SMIN = 0.004


def _pair(seed, rows, usable=None, outliers=0, noise=0.002, ties=0, rot=0.3):
    """One pair's (m, ms, usable): a seeded pose, points on the plane z = 0.61 seen from it (+ noise) and from the goal, `outliers`
    usable rows moved by 0.1 - 0.4 per axis, the first `ties` usable rows repeated in the following `ties` usable rows (equal
    residuals, bit for bit)."""
    rng = np.random.default_rng(seed)
    R, t = hr.rodrigues(rng.normal(0.0, rot, 3)), rng.normal(0.0, 0.05, 3)
    X = np.stack([rng.uniform(-0.3, 0.3, rows), rng.uniform(-0.3, 0.3, rows), np.full(rows, 0.61)], 1)
    m, ms = hr.project(X, R, t) + rng.standard_normal((rows, 2)) * noise, X[:, :2] / 0.61
    usable = np.ones(rows, np.int32) if usable is None else np.asarray(usable, np.int32)
    live = np.nonzero(usable > 0)[0]
    if outliers:
        bad = rng.choice(live[2 * ties:], outliers, replace=False)
        m[bad] += rng.uniform(0.1, 0.4, (outliers, 2)) * rng.choice([-1.0, 1.0], (outliers, 2))
    if ties:
        m[live[ties:2 * ties]], ms[live[ties:2 * ties]] = m[live[:ties]], ms[live[:ties]]
    m[usable <= 0], ms[usable <= 0] = 0.0, 0.0
    return m, ms, usable


def _flags(rows, where, n_off):
    """`n_off` unusable rows first / in the middle / last (flags 0 and -1 alternate: both mean unusable)."""
    u = np.ones(rows, np.int32)
    start = {"first": 0, "middle": (rows - n_off) // 2, "last": rows - n_off}[where]
    u[start:start + n_off] = np.where(np.arange(n_off) % 2 == 0, 0, -1)
    return u


def _case(*pairs, degenerate=False):
    m, ms, u = (np.stack(x) for x in zip(*pairs))
    return dict(m=m, ms=ms, usable=u, degenerate=degenerate)


def _collinear(rows):
    """Points of one line of the plane, seen from a seeded pose and from the goal."""
    s = np.linspace(-0.3, 0.3, rows)
    X = np.stack([s, 0.05 - 0.6 * s, np.full(rows, 0.61)], 1)
    R, t = hr.rodrigues([0.1, -0.2, 0.3]), np.array([0.03, -0.02, 0.04])
    return hr.project(X, R, t), X[:, :2] / 0.61


def _behind():
    """24 rows of which one current point lies so far out that the fitted H maps it behind the camera (third component <= 0)."""
    m, ms, u = _pair(12, 24, rot=0.0)
    R, t = hr.rodrigues([0.0, 0.5, 0.0]), np.array([0.02, -0.01, 0.03])
    X = np.concatenate([ms * 0.61, np.full((24, 1), 0.61)], 1)
    m = hr.project(X, R, t)
    m[5] = (6.0, 0.3)
    return m, ms, u


def _cases():
    out = {}
    out["1x4"] = _case(_pair(1, 4))
    out["1x5"] = _case(_pair(2, 5))
    out["3x24"] = _case(_pair(3, 24, _flags(24, "first", 5), outliers=3),                # 19 usable
                        _pair(4, 24, _flags(24, "middle", 4), outliers=3),               # 20 usable
                        _pair(5, 24, _flags(24, "last", 3)))                             # 21 usable
    out["1x130"] = _case(_pair(6, 130, _flags(130, "middle", 7), outliers=15))
    out["1x258_ties"] = _case(_pair(7, 258, _flags(258, "first", 2), outliers=30, ties=40))
    out["1x1100"] = _case(_pair(8, 1100, _flags(1100, "last", 37), outliers=120, ties=3))
    out["1x24_behind"] = _case(_behind())
    out["1x24_three_usable"] = _case(_pair(9, 24, _flags(24, "first", 21)), degenerate=True)
    m, ms = _collinear(24)
    out["1x24_collinear"] = _case((m, ms, np.ones(24, np.int32)), degenerate=True)
    # 9 collinear inliers and 3 rows off the line, each matched 0.1 - 0.15 off: a full-rank set until the re-weighting has thrown
    # two of the three out (a line and one point leave H free)
    m, ms = _collinear(9)
    R, t = hr.rodrigues([0.1, -0.2, 0.3]), np.array([0.03, -0.02, 0.04])
    X3 = np.array([[0.2, 0.25, 0.61], [-0.25, 0.1, 0.61], [0.05, -0.28, 0.61]])
    m3 = hr.project(X3, R, t) + np.array([[0.12, 0.1], [-0.1, 0.15], [0.1, -0.12]])
    out["1x12_degenerate_after_rejection"] = _case((np.concatenate([m, m3]), np.concatenate([ms, X3[:, :2] / 0.61]),
                                                    np.ones(12, np.int32)), degenerate=True)
    # the same line and 3 rows matched so far off that the first fit maps 10 of the 12 points behind the camera: the median of the
    # residuals is +inf, every finite residual keeps weight 1 and every infinite one gets 0, and 2 rows are too few
    m = np.concatenate([m, np.array([[0.25, 0.3], [-0.3, 0.2], [0.1, -0.35]])])
    ms = np.concatenate([ms, np.array([[-0.2, 0.25], [0.3, -0.1], [-0.25, -0.3]])])
    out["1x12_most_behind"] = _case((m, ms, np.ones(12, np.int32)), degenerate=True)
    return out


CASES = _cases()
_REFS = {}


def _reference(name, n_iter):
    """One fp64 reference per (case, N), computed once and shared."""
    key = (name, n_iter)
    if key not in _REFS:
        c = CASES[name]
        _REFS[key] = [hr.homography_law(c["m"][b], c["ms"][b], c["usable"][b], LAM, ZHAT, n_iter, SMIN) for b in range(len(c["m"]))]
    return _REFS[key]


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_keep_their_margins(name):
    """No GPU: every solve's second-smallest eigenvalue is >= 1e-4 of the trace or (degenerate cases only) <= 1e-10; no residual
    within 1e-6 of the rejection edge."""
    for n_iter in N_ITERS:
        for ref in _reference(name, n_iter):
            for g in ref["ratios"]:
                assert g >= 1e-4 or (CASES[name]["degenerate"] and g <= 1e-10), (name, n_iter, ref["ratios"])
            assert ref["edge"] >= 1e-6, (name, n_iter, ref["edge"])
            if not CASES[name]["degenerate"]:
                assert ref["status"] == hr.OK and ref["info"][2] == n_iter
                assert min(ref["gaps"]) >= 1e-4, (name, n_iter, ref["gaps"])             # the eigenvector is as good as eps / gap
    if name == "1x12_degenerate_after_rejection":
        assert _reference(name, 0)[0]["status"] == hr.OK
        last = _reference(name, 16)[0]
        assert last["status"] == hr.TOO_FEW and last["info"][4] == 1 and last["info"][3] >= 2
    if name == "1x12_most_behind":
        assert _reference(name, 0)[0]["status"] == hr.OK
        last = _reference(name, 4)[0]
        assert last["status"] == hr.TOO_FEW and list(last["info"][2:6]) == [1, 10, 0, 10] and np.isinf(last["sigma"])
    if name == "1x24_three_usable":
        assert all(_reference(name, n)[0]["status"] == hr.TOO_FEW and _reference(name, n)[0]["info"][4] == 0 for n in N_ITERS)
    if name == "1x24_collinear":
        assert all(_reference(name, n)[0]["status"] == hr.TOO_FEW and _reference(name, n)[0]["info"][4] == 1 for n in N_ITERS)
    if name == "1x258_ties":
        assert _reference(name, 4)[0]["info"][3] >= 30
    if name == "1x24_behind":
        assert all(_reference(name, n)[0]["info"][5] == 1 and _reference(name, n)[0]["weights"][5] == 0.0 for n in (1, 4, 16))
    if name == "3x24":
        assert [int(r["info"][0]) for r in _reference(name, 0)] == [19, 20, 21]          # odd and even usable counts


class _Op:
    """The op's device buffers for n pairs of ld rows."""

    def __init__(self, n, ld):
        self.lib, self.dev, self.n, self.ld = _lib.load(), torch.device("cuda", 0), n, ld
        f64 = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=self.dev)   # noqa: E731
        self.m, self.ms = f64(n, ld, 2), f64(n, ld, 2)
        self.usable = torch.zeros((n, ld), dtype=torch.int32, device=self.dev)
        self.scratch = torch.zeros(self.lib.vitvs_op_homography_scratch_bytes(n, ld), dtype=torch.uint8, device=self.dev)
        self.v, self.H, self.weights, self.sigma = f64(n, 6), f64(n, 9), f64(n, ld), f64(n)
        self.st = torch.full((n,), -1, dtype=torch.int32, device=self.dev)
        self.info = torch.full((n, 8), -1, dtype=torch.int32, device=self.dev)

    def load(self, case):
        m, ms = case["m"].copy(), case["ms"].copy()
        m[case["usable"] <= 0] = np.nan                         # what an unusable row holds must never reach a sum
        ms[case["usable"] <= 0] = np.nan
        self.m.copy_(torch.from_numpy(m))
        self.ms.copy_(torch.from_numpy(ms))
        self.usable.copy_(torch.from_numpy(case["usable"]))
        return self

    def call(self, n_iter, smin=SMIN, outputs=True):
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        opt = (lambda t: p(t)) if outputs else (lambda t: None)
        return self.lib.vitvs_op_homography_law(self.n, self.ld, p(self.m), p(self.ms), p(self.usable), LAM, ZHAT, n_iter, smin,
                                                p(self.scratch), p(self.v), p(self.st), opt(self.H), opt(self.info),
                                                opt(self.weights), opt(self.sigma),
                                                C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream))

    def results(self):
        return dict(v=self.v.cpu().numpy(), status=self.st.cpu().numpy(), H=self.H.cpu().numpy().reshape(-1, 3, 3),
                    info=self.info.cpu().numpy(), weights=self.weights.cpu().numpy(), sigma=self.sigma.cpu().numpy())


def _compare(got, refs, tag):
    for b, ref in enumerate(refs):
        where = f"{tag} pair {b} (ratios {['%.2e' % g for g in ref['ratios']]})"
        assert got["status"][b] == ref["status"], where
        assert np.array_equal(got["info"][b], ref["info"]), (where, got["info"][b], ref["info"])
        for key in ("v", "H", "weights"):
            scale = max(1.0, float(np.abs(ref[key]).max()))
            err = float(np.abs(got[key][b] - ref[key]).max()) / scale
            assert err <= 1e-9, (where, key, err)
        # (an infinite scale, the median of mostly infinite residuals, must be the same infinity)
        assert got["sigma"][b] == ref["sigma"] or abs(got["sigma"][b] - ref["sigma"]) <= 1e-12, (where, got["sigma"][b], ref["sigma"])


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
            for key in ("v", "H", "weights", "sigma", "info", "status"):
                assert np.array_equal(got[key], first[key], equal_nan=True), (name, key)


@gpu
def test_twelve_calls_back_to_back():
    """The same buffers, no synchronisation between the calls: every call's workspace rows are rewritten by the next."""
    names = ["3x24", "1x24_collinear", "1x24_three_usable"] * 4
    ops = [_Op(3, 24) for _ in names]                          # outputs of their own, ONE scratch block and one set of inputs
    shared = ops[0]
    stage = []
    for k, name in enumerate(names):
        case = CASES[name]
        n = len(case["m"])
        full = dict(m=np.zeros((3, 24, 2)), ms=np.zeros((3, 24, 2)), usable=np.zeros((3, 24), np.int32))
        for key in full:
            full[key][:n] = case[key]
        stage.append((_Op(3, 24).load(full), n))
    for k, (name, (src, n)) in enumerate(zip(names, stage)):
        op = ops[k]
        shared.m.copy_(src.m)
        shared.ms.copy_(src.ms)
        shared.usable.copy_(src.usable)
        op.m, op.ms, op.usable, op.scratch, op.n = shared.m, shared.ms, shared.usable, shared.scratch, n
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
    other = _case(_pair(30, 24, outliers=3), _pair(31, 24), _pair(32, 24, outliers=2))
    op.load(other)
    graph.replay()
    torch.cuda.synchronize()
    refs = [hr.homography_law(other["m"][b], other["ms"][b], other["usable"][b], LAM, ZHAT, 4, SMIN) for b in range(3)]
    assert all(min(r["ratios"]) >= 1e-4 and r["edge"] >= 1e-6 for r in refs)
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
    assert torch.isnan(op.H).all() and (op.info == -1).all() and torch.isnan(op.weights).all() and torch.isnan(op.sigma).all()
    lib, p = op.lib, lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    args = lambda **kw: [kw.get("n", 3), kw.get("ld", 24), kw.get("m", p(op.m)), kw.get("ms", p(op.ms)), kw.get("u", p(op.usable)),   # noqa: E731
                         LAM, kw.get("z", ZHAT), kw.get("N", 4), SMIN, kw.get("s", p(op.scratch)), kw.get("v", p(op.v)),
                         kw.get("st", p(op.st)), None, None, None, None, None]
    for missing in ("m", "ms", "u", "s", "v", "st"):
        assert lib.vitvs_op_homography_law(*args(**{missing: None})) == -1, missing
    for bad in (dict(n=0), dict(ld=0), dict(N=-1), dict(N=17), dict(z=0.0), dict(z=-1.0), dict(z=float("inf")), dict(z=float("nan"))):
        assert lib.vitvs_op_homography_law(*args(**bad)) == -2, bad
    assert lib.vitvs_op_homography_law(*args(ld=20000, N=1)) == -3    # the plan's: rho and w of 20000 rows are past 160 KiB of LDS
