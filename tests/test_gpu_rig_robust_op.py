"""The robust rig law's kernel at its seam (vitvs_op_rig_robust_law: rig.hip's rig_robust_kernel on caller systems, no handle, no
forward) against the fp64 numpy statement of tests/rig_robust_ref.py.  Bars: v_rig <= 1e-9 relative L2 (the
project's bar for every law), weights <= 1e-9 absolute, sigma <= 1e-12 relative, rig_info exact (the Jacobi sweeps: in 0 .. 40),
normal <= 1e-12 of its largest entry; N = 1, 4, 16 re-weightings.

The shapes are the smallest at which each mechanism can go wrong: 1 x 4 rows (fewer than six: every solve is the Jacobi SVD's),
2 x 4 (the smallest stack of full rank), 3 x 32 with the planted case A of tests/test_rig_robust_host.py, 8 x 48 (the LDS tile's last fit), 8 x 50 (the
first shape past it: the stack's copy in the global work block), 9 x 260 with row counts that are no multiples of 8 or 32 and
padded pairs (non-zero rows, garbage e) in every camera, 2 x 2048 rows (the rank counting past 256 values), an odd and an even
number of live pairs with the scale above its floor, duplicated pairs (tied residuals), cameras without rows first / in the
middle / last, a camera without a live pair, nobody contributing (two ways), a rank-deficient stack, and a stack that loses
rank only once its outliers are rejected (LDL^T first, the Jacobi SVD of the sqrt(w)-scaled copy afterwards).  The first test
asserts on the CPU, for every case and N, that every solve of the reference sits >= 100 x away from the LDL^T pivot test on
either side and every weight >= 1e-6 away from the rejection edge t = 1: no case balances on a branch."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib

import rig_ref as rg
import rig_robust_ref as rr

gpu = pytest.mark.gpu
LAM = 0.35
ITERS = (1, 4, 16)


def _case(seed, rows, lives=None, ld=None, smin=0.03, out_share=0.125, Ws=None, noise=None):
    """A seeded rig: camera i has rows[i] rows (even), the first lives[i] pairs live and following one rig twist up to
    +-noise (0.3 smin unless given: the scale then sits on its floor), a share of them gross outliers; its other pairs are padding the law must not read into its sums (random rows,
    random e)."""
    rng = np.random.default_rng(seed)
    n = len(rows)
    noise = 0.3 * smin if noise is None else noise
    lives = [r // 2 for r in rows] if lives is None else lives
    Ws = [rg.twist_matrix(*rg.random_extrinsic(rng)) for _ in range(n)] if Ws is None else Ws
    Ls = [rg.camera_system(rng, r // 2) if r else np.zeros((0, 6)) for r in rows]
    v = rng.standard_normal(6) * 0.1
    es = []
    for L, W, r, lv in zip(Ls, Ws, rows, lives):
        e = rng.standard_normal(r)
        e[:2 * lv] = (L @ W @ v)[:2 * lv] + rng.uniform(-noise, noise, 2 * lv)
        for k in rng.choice(lv, int(round(out_share * lv)), replace=False) if lv else []:
            a, m = rng.uniform(0, 2 * np.pi), rng.uniform(0.3, 0.8)
            e[2 * k] += m * np.cos(a)
            e[2 * k + 1] += m * np.sin(a)
        es.append(e)
    return dict(Ls=Ls, es=es, Ws=Ws, lives=lives, ld=ld or max(max(rows), 2), smin=smin)


def _planted_a():
    Ls, es, Ws, _, _ = rr.planted(7000, [16, 16, 16], [6, 0, 0], smin=0.03)
    return dict(Ls=Ls, es=es, Ws=Ws, lives=None, ld=32, smin=0.03)


def _ties():
    """Eight points, each pair given twice with the same e: every residual has a twin (equal bits), the scale above its floor."""
    c = _case(21, [16], smin=1e-3, out_share=0.0, noise=0.005)
    return dict(c, Ls=[np.concatenate([c["Ls"][0]] * 2)], es=[np.concatenate([c["es"][0]] * 2)], lives=[16], ld=32)


def _rank_deficient():
    """3 cameras with equal extrinsics seeing the same two points: the stack repeats 4 rows (rank 4), e scattered."""
    rng = np.random.default_rng(83)
    W = rg.twist_matrix(*rg.random_extrinsic(rng))
    L = rg.camera_system(rng, 2)
    es = [0.05 * rng.standard_normal(4) for _ in range(3)]
    return dict(Ls=[L] * 3, es=es, Ws=[W] * 3, lives=None, ld=4, smin=0.03)


def _rank_lost_after_rejection(seed=31):
    """One camera: two points five times each (rank 4, e with small noise) and a third point twice, with gross errors in opposite
    directions.  The first solve has rank 6 (LDL^T); it leaves both copies of the third point half their difference as
    residual, they are rejected, and every later solve sees rank 4: the Jacobi SVD of the scaled copy."""
    rng = np.random.default_rng(seed)
    pts = [rg.camera_system(rng, 1) for _ in range(3)]
    v = rng.standard_normal(6) * 0.1
    L = np.concatenate([pts[0]] * 5 + [pts[1]] * 5 + [pts[2]] * 2)
    e = L @ v + rng.uniform(-0.005, 0.005, 24)
    e[20:22] += [0.4, -0.3]
    e[22:24] -= [0.4, -0.3]
    return dict(Ls=[L], es=[e], Ws=[np.eye(6)], lives=None, ld=24, smin=0.01)


def _cases():
    mixed = [258, 130, 52, 260, 6, 100, 34, 18, 202]
    return {
        "1x4": _case(1, [4], out_share=0.0),
        "2x4": _case(2, [4, 4], out_share=0.0),
        "3x32_planted_a": _planted_a(),
        "8x48": _case(3, [48] * 8, smin=0.002, noise=0.005),
        "8x50_past_the_tile": _case(4, [50] * 8, smin=0.002, noise=0.005),
        "9x260_padded": _case(5, mixed, lives=[r // 2 - 1 - (i % 3) for i, r in enumerate(mixed)], ld=260),
        "2x2048": _case(6, [2048, 2048], smin=0.002, noise=0.005),
        "odd_live": _case(7, [10, 10, 10], lives=[5, 4, 4], smin=1e-3, out_share=0.25, noise=0.005),
        "even_live": _case(8, [10, 10, 10], lives=[5, 5, 4], smin=1e-3, out_share=0.25, noise=0.005),
        "ties": _ties(),
        "empty_first": _case(9, [0, 48, 20, 6], ld=48),
        "empty_middle": _case(10, [20, 0, 0, 48], ld=50),
        "empty_last": _case(11, [48, 20, 0], ld=48),
        "live_zero": _case(12, [20, 20, 20], lives=[10, 0, 7], ld=20),
        "nobody": _case(13, [0, 0, 0], ld=16),
        "nobody_live": _case(14, [8, 8], lives=[0, 0], ld=8),
        "rank_deficient": _rank_deficient(),
        "rank_lost_after_rejection": _rank_lost_after_rejection(),
    }


CASES = _cases()
# the solver of each solve: "ldlt", "jacobi", "none", or "ldlt_then_jacobi"
SOLVER = {name: "ldlt" for name in CASES}
SOLVER.update({"1x4": "jacobi", "rank_deficient": "jacobi", "nobody": "none", "nobody_live": "none",
               "rank_lost_after_rejection": "ldlt_then_jacobi"})


@functools.lru_cache(maxsize=None)
def _reference(name, n_iter):
    """Computed once per (case, N) and shared; never modified."""
    case = CASES[name]
    st = rg.statuses(case)
    trace = []
    v, w, rho, sigma, n_zero, margin, M, e = rr.robust_rig_law(case["Ls"], case["es"], case["Ws"], st, case["lives"], LAM, n_iter,
                                                               case["smin"], trace=trace)
    con = rr.contributing(case["Ls"], st, case["lives"] or [None] * len(st))
    sw = trace[-1] if trace else np.zeros((0, 6))
    return dict(v=v, w=rr.camera_weights(w, case["Ls"], st, case["lives"], case["ld"] // 2), sigma=sigma, n_zero=n_zero, margin=margin,
                rows=M.shape[0], cameras=sum(1 for r, _ in con if r), worst=max(st), status=0 if M.shape[0] else max(max(st), 1),
                normal=rg.normal_packed(sw, np.sqrt(np.repeat(w, 2)) * e) if M.shape[0] else np.zeros(28),
                margins=[rg.ldlt_margin(x) for x in trace])


def _back_to_back_cases(n=9, ld=60):
    """12 systems for the same buffers: other rows and live pairs per camera each time, every third one rank-deficient."""
    rng = np.random.default_rng(90)
    cases = []
    for k in range(12):
        if k % 3 == 2:
            c = _rank_deficient()
            cases.append(dict(c, Ls=c["Ls"] * 3, es=c["es"] * 3, Ws=c["Ws"] * 3, ld=ld))
        else:
            rows = [int(r) for r in rng.choice([0, 4, 12, 48, 60], size=n)]
            cases.append(_case(900 + k, rows, lives=[max(r // 2 - int(rng.integers(0, 3)), 0) for r in rows], ld=ld, smin=0.01))
    return cases


def _ref_of(case, n_iter):
    st = rg.statuses(case)
    trace = []
    v, w, _, sigma, n_zero, margin, M, e = rr.robust_rig_law(case["Ls"], case["es"], case["Ws"], st, case["lives"], LAM, n_iter,
                                                             case["smin"], trace=trace)
    return dict(v=v, w=rr.camera_weights(w, case["Ls"], st, case["lives"], case["ld"] // 2), sigma=sigma, n_zero=n_zero, margin=margin,
                rows=M.shape[0], margins=[rg.ldlt_margin(x) for x in trace])


def _fair(margins, solver):
    if solver == "ldlt":
        return all(m >= 100 for m in margins)
    if solver == "jacobi":
        return all(m <= 0.01 for m in margins)
    if solver == "ldlt_then_jacobi":
        return margins[0] >= 100 and all(m <= 0.01 for m in margins[1:])
    return not margins


def test_every_case_is_a_fair_test_of_the_branches_it_takes():
    for name in CASES:
        for n_iter in ITERS:
            ref = _reference(name, n_iter)
            assert _fair(ref["margins"], SOLVER[name]), (name, n_iter, SOLVER[name], ref["margins"])
            assert len(ref["margins"]) == (n_iter + 1 if ref["rows"] else 0)
            assert ref["margin"] >= 1e-6, (name, n_iter, ref["margin"])
    for k, case in enumerate(_back_to_back_cases()):
        ref = _ref_of(case, 4)
        assert _fair(ref["margins"], "jacobi" if k % 3 == 2 else "ldlt") and ref["margin"] >= 1e-6, (k, ref["margins"], ref["margin"])
    # the cases do what their names say
    assert _reference("3x32_planted_a", 4)["n_zero"] == 6
    assert _reference("rank_lost_after_rejection", 4)["n_zero"] == 2
    for name in ("8x48", "8x50_past_the_tile", "odd_live", "even_live", "ties", "2x2048"):
        for n_iter in ITERS:
            # the median sets the scale, not the floor; and it is no cancellation product: residuals of 1e-2 of the errors they
            # are differences of or more, so that the reference's own sigma is good to ~100 ulp, well inside the 1e-12 bar
            sigma = _reference(name, n_iter)["sigma"]
            e_typ = np.median(np.abs(np.concatenate(CASES[name]["es"])))
            assert sigma > CASES[name]["smin"] and sigma >= 1e-2 * e_typ, (name, n_iter, sigma, e_typ)
    live = lambda name: sum(CASES[name]["lives"])  # noqa: E731
    assert live("odd_live") % 2 == 1 and live("even_live") % 2 == 0
    assert all(lv < r // 2 for lv, r in zip(CASES["9x260_padded"]["lives"], [L.shape[0] for L in CASES["9x260_padded"]["Ls"]]))


def _pack(case):
    """(rows int32 [n], live int32 [n], L float64 [n][7][ld] column-major, W float64 [n][36]) as the op takes them."""
    n, ld = len(case["Ls"]), case["ld"]
    rows = np.array([L.shape[0] for L in case["Ls"]], np.int32)
    lives = np.array(case["lives"] if case["lives"] is not None else rows // 2, np.int32)
    Lp = np.full((n, 7, ld), np.nan)                                # rows a camera does not have must never be read
    for i, (L, e) in enumerate(zip(case["Ls"], case["es"])):
        Lp[i, :6, :rows[i]] = L.T
        Lp[i, 6, :rows[i]] = e
    return rows, lives, Lp, np.stack([np.asarray(W).reshape(36) for W in case["Ws"]])


class Op:
    """Device buffers for one geometry (n_cams, ld) and the calls."""

    def __init__(self, n, ld, dev):
        self.lib, self.n, self.ld, self.dev = _lib.load(), n, ld, dev
        nbytes = self.lib.vitvs_op_rig_robust_scratch_bytes(n, ld)
        assert nbytes == 256 + 8 * (32 * n + 21 * n * ld)
        self.scratch = torch.zeros(nbytes, dtype=torch.uint8, device=dev)          # zeroed once, before the first call only
        self.rows = torch.zeros(n, dtype=torch.int32, device=dev)
        self.live = torch.zeros(n, dtype=torch.int32, device=dev)
        self.L = torch.zeros((n, 7, ld), dtype=torch.float64, device=dev)
        self.W = torch.zeros((n, 36), dtype=torch.float64, device=dev)
        self.v = torch.full((6,), np.nan, dtype=torch.float64, device=dev)
        self.st = torch.full((9,), -7, dtype=torch.int32, device=dev)             # rig_status | rig_info [8]
        self.normal = torch.full((28,), np.nan, dtype=torch.float64, device=dev)
        self.weights = torch.full((n, ld // 2), np.nan, dtype=torch.float64, device=dev)
        self.sigma = torch.full((1,), np.nan, dtype=torch.float64, device=dev)

    def load(self, rows, lives, Lp, W):
        self.rows.copy_(torch.as_tensor(rows))
        self.live.copy_(torch.as_tensor(lives))
        self.L.copy_(torch.as_tensor(Lp))
        self.W.copy_(torch.as_tensor(W))

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def call(self, n_iter, smin, live=True):
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        rc = self.lib.vitvs_op_rig_robust_law(self.n, p(self.rows), p(self.live) if live else None, p(self.L), self.ld, p(self.W), LAM,
                                              n_iter, smin, p(self.scratch), p(self.v), p(self.st), p(self.st[1:]), p(self.normal),
                                              p(self.weights), p(self.sigma), self._stream())
        assert rc == 0, rc

    def call_plain(self):
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        rc = self.lib.vitvs_op_rig_law(self.n, p(self.rows), p(self.L), self.ld, p(self.W), LAM, p(self.scratch), p(self.v), p(self.st),
                                       p(self.st[1:]), p(self.normal), self._stream())
        assert rc == 0, rc

    def tensors(self):
        return [self.v.clone(), self.st.clone(), self.normal.clone(), self.weights.clone(), self.sigma.clone()]

    @staticmethod
    def results(tensors):
        v, st, normal, weights, sigma = [t.cpu().numpy() for t in tensors]
        return dict(v=v, status=int(st[0]), info=st[1:], normal=normal, weights=weights, sigma=float(sigma[0]))


def _check(name, got, ref, solver, n_iter, n_cams):
    info = got["info"]
    assert got["status"] == ref.get("status", 0), (name, got["status"])
    if solver == "none":
        assert list(info) == [0, 0, 0, n_cams, ref["worst"], 0, 0, 0], (name, info)
        assert np.array_equal(got["v"], np.zeros(6)) and got["sigma"] == 0.0 and not got["normal"].any() and not got["weights"].any()
        return 0.0
    last = "jacobi" if solver == "ldlt_then_jacobi" else solver
    assert (int(info[2]) == -1) if last == "ldlt" else (0 <= int(info[2]) <= 40), (name, solver, info)
    want = [ref.get("cameras", info[0]), ref["rows"], info[2], n_cams, ref.get("worst", info[4]), n_iter, ref["n_zero"], 0]
    assert list(info) == want, (name, list(info), want)
    err_w = float(np.abs(got["weights"] - ref["w"]).max())
    assert err_w <= 1e-9, (name, err_w)
    assert abs(got["sigma"] - ref["sigma"]) <= 1e-12 * ref["sigma"], (name, got["sigma"], ref["sigma"])
    if "normal" in ref:
        err_n = float(np.abs(got["normal"] - ref["normal"]).max() / np.abs(ref["normal"][:27]).max())
        assert err_n <= 1e-12 and got["normal"][27] == ref["rows"], (name, err_n)
    err = float(np.linalg.norm(got["v"] - ref["v"]) / np.linalg.norm(ref["v"]))
    assert err <= 1e-9, (name, err, got["v"], ref["v"])
    return err


@gpu
@pytest.mark.parametrize("n_iter", ITERS)
@pytest.mark.parametrize("name", list(CASES))
def test_op_equals_the_reference(name, n_iter):
    case = CASES[name]
    dev = torch.device("cuda", 0)
    op = Op(len(case["Ls"]), case["ld"], dev)
    op.load(*_pack(case))
    op.call(n_iter, case["smin"])
    got = Op.results(op.tensors())
    err = _check(name, got, _reference(name, n_iter), SOLVER[name], n_iter, op.n)
    print(f"{name} N={n_iter}: {SOLVER[name]}, sweeps {int(got['info'][2])}, zero weights {int(got['info'][6])}, v_rig rel err {err:.2e}")


@gpu
def test_live_null_means_every_pair_is_live():
    case = dict(CASES["8x48"])
    dev = torch.device("cuda", 0)
    op = Op(8, 48, dev)
    op.load(*_pack(case))
    op.live.fill_(1)                                                               # (not read)
    op.call(4, case["smin"], live=False)
    _check("live NULL", Op.results(op.tensors()), _reference("8x48", 4), "ldlt", 4, 8)


@gpu
def test_optional_outputs_may_be_null_and_bad_arguments_are_refused():
    case = CASES["3x32_planted_a"]
    dev = torch.device("cuda", 0)
    op = Op(3, 32, dev)
    op.load(*_pack(case))
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    lib = op.lib
    f = lambda n=3, rows=p(op.rows), L=p(op.L), ld=32, W=p(op.W), it=4, scratch=p(op.scratch), v=p(op.v), st=p(op.st): \
        lib.vitvs_op_rig_robust_law(n, rows, None, L, ld, W, LAM, it, 0.03, scratch, v, st, None, None, None, None, None)  # noqa: E731
    assert f() == 0
    torch.cuda.synchronize()
    ref = _reference("3x32_planted_a", 4)
    assert np.linalg.norm(op.v.cpu().numpy() - ref["v"]) <= 1e-9 * np.linalg.norm(ref["v"])
    assert int(op.st[0]) == 0 and int(op.st[1]) == -7                              # rig_info untouched
    assert bool(torch.isnan(op.normal).all()) and bool(torch.isnan(op.weights).all()) and bool(torch.isnan(op.sigma).all())
    assert f(rows=None) == -1 and f(L=None) == -1 and f(W=None) == -1 and f(scratch=None) == -1 and f(v=None) == -1 and f(st=None) == -1
    assert f(n=0) == -2 and f(n=257) == -2 and f(ld=0) == -2 and f(it=0) == -2 and f(it=17) == -2
    assert lib.vitvs_op_rig_robust_scratch_bytes(0, 48) == -2


@gpu
def test_rows_beyond_ld_are_clamped_and_bad_counts_do_not_contribute():
    """Bounds: whatever rows and live say, no camera reads past its ld rows or writes past the stack, the weights or the LDS."""
    case = CASES["3x32_planted_a"]
    dev = torch.device("cuda", 0)
    op = Op(3, 32, dev)
    rows, lives, Lp, W = _pack(case)
    op.load(np.array([3200, -5, 32], np.int32), np.array([1 << 30, 9, -3], np.int32), Lp, W)
    op.call(4, 0.03)
    got = Op.results(op.tensors())
    keep = dict(case, Ls=[case["Ls"][0], np.zeros((0, 6)), np.zeros((0, 6))], lives=None)
    ref = _ref_of(keep, 4)
    assert list(got["info"][:2]) == [1, 32] and np.linalg.norm(got["v"] - ref["v"]) <= 1e-9 * np.linalg.norm(ref["v"])
    assert np.abs(got["weights"] - ref["w"]).max() <= 1e-9


@gpu
def test_the_same_buffers_with_new_contents_back_to_back():
    """The stale-line case of the hand-off: 12 calls on one stream into the same scratch, inputs and outputs, each with other rows
    and live pairs per camera and other contents, every third a rank-deficient stack.  No host synchronisation in between."""
    dev = torch.device("cuda", 0)
    n, ld = 9, 60
    cases = _back_to_back_cases()
    packed = [[torch.as_tensor(a).to(dev) for a in _pack(c)] for c in cases]
    refs = [_ref_of(c, 4) for c in cases]
    op = Op(n, ld, dev)
    outs = []
    torch.cuda.synchronize()
    for (rows, lives, Lp, W), c in zip(packed, cases):
        op.rows.copy_(rows)
        op.live.copy_(lives)
        op.L.copy_(Lp)
        op.W.copy_(W)
        op.call(4, c["smin"])
        outs.append(op.tensors())
    torch.cuda.synchronize()
    for k, (t, ref) in enumerate(zip(outs, refs)):
        _check(f"call {k}", Op.results(t), ref, "jacobi" if k % 3 == 2 else "ldlt", 4, n)
    assert int(op.scratch[:4].view(torch.int32)[0]) == 0             # the ticket is left zero


@gpu
@pytest.mark.parametrize("name", ["9x260_padded", "rank_lost_after_rejection"])
def test_bit_reproducible(name):
    case = CASES[name]
    dev = torch.device("cuda", 0)
    op = Op(len(case["Ls"]), case["ld"], dev)
    op.load(*_pack(case))
    outs = []
    for _ in range(10):
        op.call(4, case["smin"])
        outs.append(op.tensors())
    torch.cuda.synchronize()
    for t in outs[1:]:
        for a, b in zip(t, outs[0]):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@gpu
def test_a_captured_graph_of_two_launches_replays():
    """Two consecutive launches in one captured graph, replayed twice with new inputs: the ticket the first leaves is the second's."""
    dev = torch.device("cuda", 0)
    a, b = CASES["8x48"], CASES["8x50_past_the_tile"]
    ops = [Op(8, 48, dev), Op(8, 50, dev)]
    ops[1].scratch = ops[0].scratch = torch.zeros(max(o.scratch.numel() for o in ops), dtype=torch.uint8, device=dev)   # one ticket
    for op, c in zip(ops, (a, b)):
        op.load(*_pack(c))
        op.call(4, c["smin"])                                                     # (eager first: nothing is set up inside a capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops[0].call(4, a["smin"])
        ops[1].call(4, b["smin"])
    for op in ops:
        op.v.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    _check("replay 8x48", Op.results(ops[0].tensors()), _reference("8x48", 4), "ldlt", 4, 8)
    _check("replay 8x50", Op.results(ops[1].tensors()), _reference("8x50_past_the_tile", 4), "ldlt", 4, 8)
    c = _case(40, [48] * 8, smin=0.002, noise=0.005)
    ref = _ref_of(c, 4)
    assert min(ref["margins"]) >= 100 and ref["margin"] >= 1e-6
    ops[0].load(*_pack(c))
    graph.replay()
    torch.cuda.synchronize()
    _check("replay, new inputs", Op.results(ops[0].tensors()), ref, "ldlt", 4, 8)
    assert int(ops[0].scratch[:4].view(torch.int32)[0]) == 0


@gpu
def test_the_plain_op_is_untouched_by_a_robust_call_on_the_same_block():
    dev = torch.device("cuda", 0)
    case = CASES["9x260_padded"]
    op = Op(len(case["Ls"]), case["ld"], dev)
    op.load(*_pack(case))
    op.call_plain()
    before = op.tensors()[:3]
    op.call(4, case["smin"])
    op.call_plain()
    after = op.tensors()[:3]
    torch.cuda.synchronize()
    for x, y in zip(before, after):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    ref = rg.rig_law(case["Ls"], case["es"], case["Ws"], rg.statuses(case), LAM)
    assert np.linalg.norm(after[0].cpu().numpy() - ref["v_rig"]) <= 1e-9 * np.linalg.norm(ref["v_rig"])
