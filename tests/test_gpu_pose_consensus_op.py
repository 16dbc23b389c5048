"""The consensus start of the pose law at the kernel's seam (vitvs_op_pose_consensus_law: pose.hip on caller-given points, no handle,
no forward) against the fp64 numpy statement of tests/pose_consensus_ref.py.

Exact: the status, pose_info (with the winner's j + 1 in [6] and the start weights at 1 in [7]) and, with N = 0, the weights: they are
the start weights, 0 or 1.  Numeric, the bars of tests/test_gpu_pose_op.py: v_pose, R, t and the final weights <= 1e-9, sigma <=
1e-12.  Bit equality: no hypotheses (n_hyp = 0) is vitvs_op_pose_law on every case; ten runs; a captured graph's replay.

The cases and their references are tests/pose_consensus_cases.py's; tests/test_pose_consensus_host.py asserts on the CPU that in every
one the winner's cost is >= 1e-6 (relative) below that of any other row set, that no residual is within 1e-6 of the cut-off T or of
the rejection edge of a re-weighting, and that every solve keeps the eigen-gap margin of the law's own op test: neither a winner, a
start weight nor a status can flip, and no case is left out here."""
import ctypes as C

import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib

import pose_consensus_cases as cc
import pose_consensus_ref as cr

gpu = pytest.mark.gpu
KEYS = ("v", "R", "t", "weights", "sigma", "info", "status")


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

    def _args(self, n_iter, smin):
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        return [self.n, self.ld, p(self.P), p(self.Q), p(self.usable), cc.LAM, n_iter, smin, p(self.scratch), p(self.v), p(self.st),
                p(self.pose), p(self.info), p(self.weights), p(self.sigma), C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)]

    def call(self, n_hyp, n_iter, smin=cc.SMIN, seed=cc.SEED):
        return self.lib.vitvs_op_pose_consensus_law(*self._args(n_iter, smin), n_hyp, seed)

    def call_plain(self, n_iter, smin=cc.SMIN):
        return self.lib.vitvs_op_pose_law(*self._args(n_iter, smin))

    def clear(self):
        for t in (self.v, self.pose, self.weights, self.sigma):
            t.fill_(float("nan"))
        self.info.fill_(-1)

    def results(self):
        pose = self.pose.cpu().numpy()
        return dict(v=self.v.cpu().numpy(), status=self.st.cpu().numpy(), R=pose[:, :9].reshape(-1, 3, 3), t=pose[:, 9:],
                    info=self.info.cpu().numpy(), weights=self.weights.cpu().numpy(), sigma=self.sigma.cpu().numpy())


def _compare(got, refs, tag, n_iter):
    for b, ref in enumerate(refs):
        where = f"{tag} pair {b} (cost gap {ref['cgap']:.1e}, edge_T {ref['edge_T']:.1e}, gaps {['%.1e' % g for g in ref['gaps']]})"
        assert got["status"][b] == ref["status"], where
        assert np.array_equal(got["info"][b], ref["info"]), (where, got["info"][b], ref["info"])
        if n_iter == 0:                                         # (no re-weighting: the weights are the start weights)
            assert np.array_equal(ref["weights"], ref["start"]) and np.array_equal(got["weights"][b], ref["start"]), where
        for key in ("v", "R", "t", "weights"):
            err = float(np.abs(got[key][b] - ref[key]).max())
            assert err <= 1e-9, (where, key, err)
        assert got["sigma"][b] == ref["sigma"] or abs(got["sigma"][b] - ref["sigma"]) <= 1e-12, (where, got["sigma"][b], ref["sigma"])


@gpu
@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_kernel_equals_the_reference(name):
    case = cc.CASES[name]
    op = _Op(*case["usable"].shape).load(case)
    for n_hyp in cc.N_HYPS:
        for n_iter in cc.N_ITERS:
            op.clear()
            assert op.call(n_hyp, n_iter) == 0
            _compare(op.results(), cc.reference(name, n_hyp, n_iter), f"{name} M={n_hyp} N={n_iter}", n_iter)


@gpu
@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_no_hypotheses_is_the_law_without_consensus_bit_for_bit(name):
    case = cc.CASES[name]
    op = _Op(*case["usable"].shape).load(case)
    for n_iter in cc.N_ITERS:
        assert op.call_plain(n_iter) == 0
        want = op.results()
        op.clear()
        assert op.call(0, n_iter) == 0
        got = op.results()
        for key in KEYS:
            assert np.array_equal(got[key], want[key], equal_nan=True), (name, n_iter, key)
        assert not got["info"][:, 6:].any()
        # ... and the law without consensus behind a call with it: the plain form's start weights went over the workspace's flag row
        assert op.call(256, n_iter) == 0 and op.call_plain(n_iter) == 0
        again = op.results()
        for key in KEYS:
            assert np.array_equal(again[key], want[key], equal_nan=True), (name, n_iter, key, "behind a consensus call")


@gpu
def test_another_seed_draws_other_rows():
    case = cc.CASES["3x24"]
    op = _Op(3, 24).load(case)
    refs = [cr.pose_consensus_law(case["P"][b], case["Q"][b], case["usable"][b], cc.LAM, 4, cc.SMIN, 256, cc.SEED + 1) for b in range(3)]
    assert all(r["cgap"] >= 1e-6 and r["edge_T"] >= 1e-6 and r["edge"] >= 1e-6 and min(r["gaps"]) >= 1e-6 for r in refs)
    assert [int(r["info"][6]) for r in refs] != [int(r["info"][6]) for r in cc.reference("3x24", 256, 4)]
    assert op.call(256, 4, seed=cc.SEED + 1) == 0
    _compare(op.results(), refs, "seed + 1", 4)


@gpu
def test_ten_runs_have_equal_bits():
    for name, n_hyp in (("3x24", 257), ("3x300", 512)):
        case = cc.CASES[name]
        op = _Op(*case["usable"].shape).load(case)
        first = None
        for _ in range(10):
            assert op.call(n_hyp, 4) == 0
            got = op.results()
            first = first or got
            for key in KEYS:
                assert np.array_equal(got[key], first[key], equal_nan=True), (name, key)


@gpu
def test_captured_graph_replays():
    case = cc.CASES["3x24"]
    op = _Op(3, 24).load(case)
    assert op.call(256, 4) == 0                                 # (warm-up outside the capture)
    torch.cuda.synchronize()
    eager = op.results()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert op.call(256, 4) == 0
    for _ in range(2):
        op.v.fill_(float("nan"))
        op.info.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        got = op.results()
        for key in KEYS:
            assert np.array_equal(got[key], eager[key], equal_nan=True), key
    _compare(got, cc.reference("3x24", 256, 4), "replay", 4)


@gpu
def test_error_returns():
    case = cc.CASES["3x24"]
    op = _Op(3, 24).load(case)
    lib, p = op.lib, lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    args = lambda **kw: [kw.get("n", 3), kw.get("ld", 24), kw.get("P", p(op.P)), kw.get("Q", p(op.Q)), kw.get("u", p(op.usable)),   # noqa: E731
                         cc.LAM, kw.get("N", 4), kw.get("smin", cc.SMIN), kw.get("s", p(op.scratch)), kw.get("v", p(op.v)),
                         kw.get("st", p(op.st)), None, None, None, None, None, kw.get("M", 256), kw.get("seed", cc.SEED)]
    op.clear()
    assert lib.vitvs_op_pose_consensus_law(*args()) == 0                        # NULL optional outputs
    torch.cuda.synchronize()
    refs = cc.reference("3x24", 256, 4)
    assert list(op.st.cpu().numpy()) == [r["status"] for r in refs]
    assert np.abs(op.v.cpu().numpy() - np.stack([r["v"] for r in refs])).max() <= 1e-9
    assert torch.isnan(op.pose).all() and (op.info == -1).all() and torch.isnan(op.weights).all() and torch.isnan(op.sigma).all()
    for missing in ("P", "Q", "u", "s", "v", "st"):
        assert lib.vitvs_op_pose_consensus_law(*args(**{missing: None})) == -1, missing
    for bad in (dict(n=0), dict(ld=0), dict(N=-1), dict(N=17), dict(M=-1), dict(M=4097), dict(smin=0.0), dict(smin=-1.0),
                dict(smin=float("nan"))):
        assert lib.vitvs_op_pose_consensus_law(*args(**bad)) == -2, bad
    assert lib.vitvs_op_pose_consensus_law(*args(M=0, smin=0.0)) == 0           # without hypotheses the floor may be 0, as before
    assert lib.vitvs_op_pose_consensus_law(*args(M=4096, seed=0xFFFFFFFF)) == 0
    assert lib.vitvs_op_pose_consensus_law(*args(ld=20000, N=1)) == -3          # the plan's: past 160 KiB of LDS
    assert lib.vitvs_op_pose_consensus_law(*args(ld=20000, N=0)) == -3          # ... and without re-weightings: rho and the row list
    torch.cuda.synchronize()
