"""The operator hooks of include/vitvs_ops.h at both ends of the ranges the header states (GPU).

One parametrised test over the table of tests/contract_ends_cases.py; tests/test_contract_ends_host.py checks the table against
the header, derives every size that comes from a launch plan and asserts the conditioning of every reference on the CPU.  The
drivers are the neighbouring op tests' own (their buffers, packers, comparisons and bars); outputs start as NaN or sentinels with
guard words behind them that no launch may write; a refused call launches nothing and leaves every output at its sentinel; each
case records its worst error as a junit property (`--junitxml=FILE -o junit_family=legacy`).

The ends (here: a case of this module; otherwise the test that already sits on the end) and the worst error over the hook's cases
of this module, every figure read from the junit properties of one run on an MI355X.  The module's 87 cases take 7.5 s there.

  hook                       smallest                    largest                              first refused             worst error
  rig_law                    1 camera x 1 row (here)     256 cameras, ld 1 / 2 / 4 / 48,      257 cameras, -2 (here)    v_rig 3.9e-15 rel
                                                         both solvers, equal bits, two
                                                         launches, one block (here)
  rig_robust_law             1 camera x 1 pair, and 256  256 cameras, ld 2 / 4 / 48, both     ld 80 at 256 cameras, -3  v_rig 1.8e-15 rel
                             x ld 1: no pair (here)      solvers, equal bits, and the plan's  (here); 257 cameras, -2
                                                         ld 79: 158 KiB of LDS (here)         (test_gpu_rig_robust_op)
  pose_rig_law               1 x 1 and 256 x 1 (here)    256 cameras, ld 2 and the plan's     ld 40 at 256 cameras, -3  1.9e-14 abs
                                                         ld 39 (here)                         (here); n_cams 0
                                                                                              (test_gpu_pose_rig_op)
  pose_law                   ld 1 (here), ld 3           ld 10080, 64 pairs (here)            ld 10081, -3 (here)       3.0e-14 abs
                             (test_gpu_pose_op)
  pose_consensus_law         ld 1, ld 3, n_hyp 1 (here), ld 8060, 64 pairs, n_hyp 4096        ld 8061, -3 (here);       6.7e-16 abs
                             n_hyp 0 (..._consensus_op)  (here)                               n_hyp 4097 (..._consensus_op)
  homography_law             ld 1 (here), ld 4           ld 9864, 64 pairs (here)             ld 9865, -3 (here)        2.4e-14 abs
                             (test_gpu_homography_op)
  homography_consensus_law   ld 1, ld 4, n_hyp 1 (here), ld 7888, 64 pairs, n_hyp 4096        ld 7889, -3 (here);       2.6e-14 abs
                             n_hyp 0 (..._consensus_op)  (here)                               n_hyp 4097 (..._consensus_op)
  best_order_dev             T 1, 4, 9 (here)            T 16384, all equal (here), random    129 x 129, -3             0 (equality)
                                                         (test_gpu_select_op)                 (test_gpu_select_op)
  gram_stencil               grids 1, 2, 3, 5; ties,     any grid: 30 x 30                    -                         sim_1 2.4e-7
                             signs, zeros, norms (here)  (test_gpu_correspond_cover)
  gram_argmax                T 1, 2, 31, 33 (here)       T 2100 (test_gpu_correspond_cover)   -                         sim_1 2.2e-7
  quarter_turns              S 1, 2, 31, 33 (here)       S 224 (test_gpu_roll_op)             -                         0 (equality)
  normalize_rows             Dp 1 (test_gpu_ends_cover)  Dp 4097 (here)                       -                         1.1e-7 rel
  saliency                   1 head (here)               16 heads; T 8191 / 8189 (here)       T 8192 / 8190, -3 (here); 2.0e-6 abs
                                                                                              head H (test_gpu_ends_cover)
  embed_ln, residual_ln,     1 slice, one image of one   8 slices, the same (here)            0 and 9 slices            0.33 of the bars
  residual_desc              token (here)                                                     (test_gpu_ends_cover)
  attention                  N = 1 (test_gpu_attention_keys)

The rig law's hooks take no camera status (a camera without rows is the one that does not contribute); the pose rig law's cases
carry cameras whose status is not OK.  With the references written in the kernels' order of arithmetic, several homography cases
agree bit for bit (worst error 0).
"""
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib
from op_support import gpu_lib as lib  # noqa: F401
from op_support import mk, nan_like, ptr, rel_max, stream, values

import contract_ends_cases as ce

pytestmark = pytest.mark.gpu

GUARD = 64                # words behind every output that no launch may write
KEY_SENTINEL = 0x5A5A5A5A5A5A5A5A
IDX_SENTINEL = -7


def _sentinel(dtype):
    return float("nan") if dtype.is_floating_point else (0x5A if dtype == torch.uint8 else IDX_SENTINEL)


def _untouched(t):
    return bool(torch.isnan(t).all()) if t.dtype.is_floating_point else bool((t == _sentinel(t.dtype)).all())


def _guard(op, names):
    """Moves the named tensors of an op test's buffer object in front of GUARD sentinel words each; -> a check of those words."""
    wholes = []
    for name in names:
        t = getattr(op, name)
        n = t.numel()
        whole = torch.full((n + GUARD,), _sentinel(t.dtype), dtype=t.dtype, device=t.device)
        whole[:n] = t.reshape(-1)
        setattr(op, name, whole[:n].view(t.shape))
        wholes.append((name, whole[n:]))

    def check():
        torch.cuda.synchronize()
        for name, tail in wholes:
            assert _untouched(tail), f"the words behind {name} were written"
    return check


def _all_untouched(op, names):
    torch.cuda.synchronize()
    for name in names:
        assert _untouched(getattr(op, name)), f"a refused call wrote {name}"


def _p(t):
    return C.c_void_p(t.data_ptr())


# ============================================================================================================== the rig law
RIG_OUT = ("v", "st", "normal")


def _rig_op(ro, n, ld):
    op = ro.Op(n, ld, torch.device("cuda", 0))
    op.st.fill_(IDX_SENTINEL)
    return op, _guard(op, RIG_OUT + ("scratch",))


def _rig(case, a, d, rec):
    import test_gpu_rig_op as ro
    n, ld = a["n"], a["ld"]
    if case.rc != 0:                   # one camera too many: the block, systems and outputs of 256 cameras are more than it may touch
        op, tails = _rig_op(ro, 256, ld)
        rows = torch.full((n,), ld, dtype=torch.int32, device="cuda")
        L = torch.zeros((n, 7, ld), dtype=torch.float64, device="cuda")
        W = torch.zeros((n, 36), dtype=torch.float64, device="cuda")
        rc = op.lib.vitvs_op_rig_law(n, _p(rows), _p(L), ld, _p(W), ce.LAM, _p(op.scratch), _p(op.v), _p(op.st), _p(op.st[1:]),
                                     _p(op.normal), stream())
        assert rc == case.rc, rc
        _all_untouched(op, RIG_OUT)
        assert not op.scratch.any(), "a refused call wrote its scratch block"
        tails()
        return 0.0
    op, tails = _rig_op(ro, n, ld)
    op.load(*ro._pack(d["case"]))
    op.call()
    worst = ro._check(case.id, op.results(), d["ref"], d["solver"])
    if a.get("bits"):                  # ten launches, then the two-launch form: equal bits
        outs = []
        for _ in range(10):
            op.call()
            outs.append((op.v.clone(), op.normal.clone(), op.st.clone()))
        assert op.lib.vitvs_op_rig_two_launches(1) == 0
        try:
            op.call()
        finally:
            assert op.lib.vitvs_op_rig_two_launches(0) == 1
        outs.append((op.v.clone(), op.normal.clone(), op.st.clone()))
        torch.cuda.synchronize()
        for k, (v, normal, st) in enumerate(outs[1:]):
            assert torch.equal(v.view(torch.int64), outs[0][0].view(torch.int64)), ("v", k)
            assert torch.equal(normal.view(torch.int64), outs[0][1].view(torch.int64)), ("normal", k)
            assert torch.equal(st, outs[0][2]), ("status and info", k)
    if a.get("block"):                 # the block, zeroed once, then serves 3 cameras and 256 again
        small, _ = _rig_op(ro, 3, 48)
        small.scratch = op.scratch
        small.load(*ro._pack(d["small"]))
        small.call()
        worst = max(worst, ro._check(case.id + " (3 cameras)", small.results(), d["small_ref"], "ldlt"))
        op.v.fill_(float("nan"))
        op.call()
        worst = max(worst, ro._check(case.id + " (256 again)", op.results(), d["ref"], d["solver"]))
    assert int(op.scratch[:4].view(torch.int32)[0]) == 0             # the ticket is left zero
    tails()
    rec("v_rig", worst)
    return worst


# ======================================================================================================= the robust rig law
ROBUST_OUT = ("v", "st", "normal", "weights", "sigma")


def _robust(case, a, d, rec):
    import test_gpu_rig_robust_op as rro
    n, ld = a["n"], a["ld"]
    op = rro.Op(n, ld, torch.device("cuda", 0))
    op.st.fill_(IDX_SENTINEL)
    tails = _guard(op, ROBUST_OUT + ("scratch",))
    if case.rc != 0:
        op.rows.fill_(ld & ~1)
        rc = op.lib.vitvs_op_rig_robust_law(n, _p(op.rows), None, _p(op.L), ld, _p(op.W), ce.LAM, 4, 0.01, _p(op.scratch), _p(op.v),
                                            _p(op.st), _p(op.st[1:]), _p(op.normal), _p(op.weights), _p(op.sigma), stream())
        assert rc == case.rc, rc
        _all_untouched(op, ROBUST_OUT)
        assert not op.scratch.any(), "a refused call wrote its scratch block"
        tails()
        return 0.0
    c = d["case"]
    op.load(*rro._pack(c))
    if "rows_given" in c:              # one row per camera and live = NULL (every pair live): only the dropped odd row leaves
        op.rows.copy_(torch.as_tensor(np.array(c["rows_given"], np.int32)))              # nobody to contribute
    op.call(d["n_iter"], c["smin"], live="rows_given" not in c)
    got = rro.Op.results(op.tensors())
    worst = rro._check(case.id, got, d["ref"], d["solver"], d["n_iter"], n)
    if a.get("bits"):                  # ten launches with equal bits
        outs = []
        for _ in range(10):
            op.call(d["n_iter"], c["smin"])
            outs.append(op.tensors())
        torch.cuda.synchronize()
        for k, t in enumerate(outs):
            for x, y in zip(t, outs[0]):
                assert torch.equal(x.view(torch.int32), y.view(torch.int32)), k
        assert np.array_equal(rro.Op.results(outs[0])["v"].view(np.int64), got["v"].view(np.int64))
    assert int(op.scratch[:4].view(torch.int32)[0]) == 0
    tails()
    rec("v_rig", worst)
    return worst


# ========================================================================================================= the pose rig law
POSE_RIG_OUT = ("v", "pose", "moments", "weights", "sigma", "st", "info")


def _worst_of(got, ref, keys):
    return max(float(np.abs(np.asarray(got[k]) - np.asarray(ref[k])).max()) for k in keys if np.size(ref[k]))


def _pose_rig(case, a, d, rec):
    import test_gpu_pose_rig_op as pro
    n, ld = a["n"], a["ld"]
    op = pro._Op(n, ld)
    op.st.fill_(IDX_SENTINEL)
    op.info.fill_(IDX_SENTINEL)
    tails = _guard(op, POSE_RIG_OUT + ("scratch",))
    if case.rc != 0:
        op.usable.fill_(1)
        assert op.call(a["n_iter"]) == case.rc
        _all_untouched(op, POSE_RIG_OUT)
        assert not op.scratch.any(), "a refused call wrote its scratch block"
        tails()
        return 0.0
    op.load(d["case"])
    worst = 0.0
    for n_iter, ref in d["refs"].items():
        assert op.call(n_iter) == 0
        got = op.results()
        pro._compare(got, ref, f"{case.id} N={n_iter}")
        worst = max(worst, _worst_of(got, ref, ("v", "R", "t", "weights")))
    tails()
    rec("v_R_t_weights", worst)
    return worst


# ============================================================================== the pose and homography laws, consensus starts
def _pairs_law(case, a, d, rec):
    pose, consensus = "pose" in case.hook, "consensus" in case.hook
    if pose:
        import test_gpu_pose_consensus_op as cons
        import test_gpu_pose_op as plain
        outs, keys = ("v", "pose", "weights", "sigma", "st", "info"), ("v", "R", "t", "weights")
    else:
        import test_gpu_homography_consensus_op as cons
        import test_gpu_homography_op as plain
        outs, keys = ("v", "H", "weights", "sigma", "st", "info"), ("v", "H", "weights")
    op = (cons if consensus else plain)._Op(a["pairs"], a["ld"])
    op.st.fill_(IDX_SENTINEL)
    op.info.fill_(IDX_SENTINEL)
    tails = _guard(op, outs + ("scratch",))

    def call(n_hyp, n_iter, smin):
        return op.call(n_hyp, n_iter, smin, 1) if consensus else op.call(n_iter, smin)
    if case.rc != 0:
        op.usable.fill_(1)
        assert call(a.get("n_hyp", (0,))[0], a["n_iter"][0], 0.019) == case.rc
        _all_untouched(op, outs)
        assert not op.scratch.any(), "a refused call wrote its scratch block"
        tails()
        return 0.0
    op.load(d["case"])
    worst = 0.0
    for (n_hyp, n_iter), refs in d["refs"].items():
        for name in outs[:4]:
            getattr(op, name).fill_(float("nan"))
        assert call(n_hyp, n_iter, d["smin"]) == 0
        got = op.results()
        tag = f"{case.id} M={n_hyp} N={n_iter}"
        if consensus:
            cons._compare(got, refs, tag, n_iter)
        else:
            plain._compare(got, refs, tag)
        for b, ref in enumerate(refs):
            worst = max(worst, _worst_of({k: got[k][b] for k in keys}, ref, keys))
    tails()
    rec("v_pose_weights", worst)
    return worst


# =========================================================================================================== the best order
def _best(case, a, d, rec):
    T = a["T"]
    nn1, nn2, sim = (torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).cuda()
                     for x, dt in zip(d["tables"], (np.int32, np.int32, np.float32)))
    for cells, want in d["want"].items():
        out = torch.full((T + GUARD,), IDX_SENTINEL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert _lib.load().vitvs_op_best_order_dev(T, cells, 1, _p(nn1), _p(nn2), _p(sim), _p(out), None) == 0
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert (got[T:] == IDX_SENTINEL).all(), "the words behind the order were written"
        assert np.array_equal(got[:T], want), (case.id, cells, int(np.argmax(got[:T] != want)))
    rec("order", 0.0)                  # equality held
    return 0.0


# ================================================================================================ the stencil and fused arg-max
CoverCase = namedtuple("CoverCase", "id T special")


def _check_tables(case_id, S, n1, n2, s1, argmax_tol, sim_tol, special=""):
    """test_gpu_correspond_cover._check_tables where it applies (T >= 2), and on top of it: EVERY index is fp64's (the host test
    asserted a clear maximum, or a planted exact tie with numpy's first index, in every row and column).  -> worst |sim_1 - max|."""
    import test_gpu_correspond_cover as cc
    T = S.shape[0]
    assert n1.min() >= 0 and n1.max() < T and n2.min() >= 0 and n2.max() < T, case_id
    if T >= 2 and (argmax_tol, sim_tol) == (cc.ARGMAX_TOL, cc.SIM_TOL):
        cc._check_tables(CoverCase(case_id, T, special), S, n1, n2, s1, 0)
    rmax, cmax = S.max(1), S.max(0)
    assert float((rmax - S[np.arange(T), n1]).max()) <= argmax_tol, (case_id, "nn_1 is not a row maximum")
    assert float((cmax - S[n2, np.arange(T)]).max()) <= argmax_tol, (case_id, "nn_2 is not a column maximum")
    err = float(np.abs(s1.astype(np.float64) - rmax).max())
    assert err <= sim_tol, (case_id, "sim_1", err)
    assert np.array_equal(n1, S.argmax(1)), (case_id, "nn_1 differs from fp64", np.nonzero(n1 != S.argmax(1))[0])
    assert np.array_equal(n2, S.argmax(0)), (case_id, "nn_2 differs from fp64", np.nonzero(n2 != S.argmax(0))[0])
    return err


def _tables(n, T):
    """keys and tables of n pairs and one guard pair behind them"""
    keys_r = torch.full(((n + 1) * T,), KEY_SENTINEL, dtype=torch.int64, device="cuda")
    nn1 = torch.full(((n + 1) * T,), IDX_SENTINEL, dtype=torch.int32, device="cuda")
    sim1 = torch.full(((n + 1) * T,), float("nan"), dtype=torch.float32, device="cuda")
    return keys_r, keys_r.clone(), nn1, nn1.clone(), sim1


def _check_guard_pair(case_id, n, T, keys_r, keys_c, nn1, nn2, sim1):
    tail = slice(n * T, None)
    assert bool((keys_r[tail] == KEY_SENTINEL).all()) and bool((keys_c[tail] == KEY_SENTINEL).all()), (case_id, "guard keys")
    assert bool((nn1[tail] == IDX_SENTINEL).all()) and bool((nn2[tail] == IDX_SENTINEL).all()), (case_id, "guard tables")
    assert bool(sim1[tail].isnan().all()), (case_id, "guard sim_1")


def _stencil(case, a, d, rec, lib):
    import test_gpu_correspond_cover as cc
    g, D = a["grid"], a["D"]
    T = g * g
    rc, plan = cc.gram_plan(lib, _lib.F32, 1, T, D, 1, 1)
    assert rc == 0 and plan[0] == cc.GRAM_STENCIL, plan
    argmax_tol, sim_tol = ce.stencil_norm_bars() if a["kind"] == "norm" else (cc.ARGMAX_TOL, cc.SIM_TOL)
    worst = 0.0
    for P, e in d.items():
        keys_r, keys_c, nn1, nn2, sim1 = _tables(1, T)
        G = torch.full((2 * T * T,), float("nan"), dtype=torch.float32, device="cuda")
        sq = torch.full((3 * T,), float("nan"), dtype=torch.float32, device="cuda")
        x = e["x"].cuda()
        rc = lib.vitvs_op_gram_stencil(ptr(x), T, P, D, g, 1, 0, ptr(G), ptr(sq), ptr(keys_r), ptr(keys_c), ptr(nn1), ptr(nn2),
                                       ptr(sim1), stream())
        assert rc == 0, (case.id, P, rc)
        torch.cuda.synchronize()
        _check_guard_pair(case.id, 1, T, keys_r, keys_c, nn1, nn2, sim1)
        assert bool(G[T * T:].isnan().all()) and bool(sq[2 * T:].isnan().all()), (case.id, "guard Gram / norms")
        assert bool(torch.isfinite(G[:T * T]).all()) and bool(torch.isfinite(sq[:2 * T]).all()), (case.id, P, "a prefix row leaked")
        s1 = sim1.cpu().numpy()[:T]
        assert np.isfinite(s1).all(), (case.id, P)
        worst = max(worst, _check_tables(f"{case.id} P={P}", e["S"], nn1.cpu().numpy()[:T].astype(np.int64),
                                         nn2.cpu().numpy()[:T].astype(np.int64), s1, argmax_tol, sim_tol,
                                         "neg" if a["kind"] == "neg" else ""))
    rec("sim_1", worst)
    return worst


def _argmax(case, a, d, rec, lib):
    import test_gpu_correspond_cover as cc
    T = a["T"]
    worst = 0.0
    for (Dp, pairs, shared), e in d.items():
        rc, plan = cc.gram_plan(lib, _lib.F32, 0, T, Dp, pairs, pairs)
        assert rc == 0 and plan[0] == cc.GRAM_F32 and not plan[6], plan
        keys_r, keys_c, nn1, nn2, sim1 = _tables(pairs, T)
        dn = e["dn"].cuda()
        rc = lib.vitvs_op_gram_argmax(_lib.F32, ptr(dn), T, Dp, pairs, int(shared), None, ptr(keys_r), ptr(keys_c), ptr(nn1), ptr(nn2),
                                      ptr(sim1), stream())
        assert rc == 0, (case.id, Dp, pairs, shared, rc)
        torch.cuda.synchronize()
        _check_guard_pair(case.id, pairs, T, keys_r, keys_c, nn1, nn2, sim1)
        n1, n2, s1 = nn1.cpu().numpy().astype(np.int64), nn2.cpu().numpy().astype(np.int64), sim1.cpu().numpy()
        for b in range(pairs):
            o = slice(b * T, (b + 1) * T)
            worst = max(worst, _check_tables(f"{case.id} Dp={Dp} pairs={pairs} shared={shared} pair {b}", e["S"][b], n1[o], n2[o], s1[o],
                                             cc.ARGMAX_TOL, cc.SIM_TOL))
    rec("sim_1", worst)
    return worst


# ========================================================================================================= the elementwise ends
def _turns(case, a, d, rec, lib):
    S, n = a["S"], 2
    rng = np.random.default_rng(ce._seed(case))
    frames = rng.integers(0, 256, size=(n, S, S, 3), dtype=np.uint8)
    f = torch.from_numpy(frames).cuda()
    size = n * 4 * S * S * 3
    out = torch.full((size + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    assert lib.vitvs_op_quarter_turns(ptr(f), n, S, ptr(out), stream()) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[size:] == 0x5A).all(), "the bytes behind the last copy were written"
    got = got[:size].reshape(n, 4, S, S, 3)
    for i in range(n):
        for k in range(4):
            assert np.array_equal(got[i, k], np.rot90(frames[i], k)), (S, i, k)
    assert np.array_equal(f.cpu().numpy(), frames)
    rec("rot90", 0.0)
    return 0.0


def _normalize(case, a, d, rec, lib):
    import test_gpu_ends_cover as ec
    Dp, rows = a["Dp"], ce.NORMALIZE_ROWS
    src = ec.normalize_inputs(rows, Dp, True)
    dst = torch.full((rows * Dp + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    srcd = src.cuda()
    assert lib.vitvs_op_normalize_rows(ptr(srcd), ptr(dst), rows, Dp, stream()) == 0
    torch.cuda.synchronize()
    got = dst.cpu()
    assert bool(torch.isnan(got[rows * Dp:]).all()), "the words behind the last row were written"
    got = got[:rows * Dp].view(rows, Dp)
    assert torch.isfinite(got).all() and not got[rows // 2].any(), "the all-zero row does not give zeros"
    err = rel_max(got, ec.dn_ref(src))
    rec("normalize", err)
    assert err <= ce.normalize_bar(), err
    return err


def _saliency(case, a, d, rec, lib):
    T, P, H, heads = a["T"], a["P"], a["H"], list(a["heads"])
    idx = (C.c_int32 * len(heads))(*heads)
    out = torch.full((2 * T + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    if case.rc != 0:
        qkv = torch.zeros((2 * (P + T), 3 * 64 * H), device="cuda")
        assert lib.vitvs_op_saliency(_lib.F32, ptr(qkv), ptr(out), 2, T, P, H, idx, len(heads), 0, stream()) == case.rc
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()), "a refused call wrote its output"
        return 0.0
    qd = d["qkv"].cuda()
    rc = lib.vitvs_op_saliency(_lib.F32, ptr(qd), ptr(out), 2, T, P, H, idx, len(heads), 0, stream())
    assert rc == 0, (rc, _lib.last_error(None))
    torch.cuda.synchronize()
    got = out.cpu()
    assert bool(torch.isnan(got[2 * T:]).all()), "the words behind the last image were written"
    got = got[:2 * T].view(2, T)
    for img in range(2):
        assert float(got[img].min()) == 0.0 and float(got[img].max()) == 1.0, f"image {img} is not min-max normalised"
        assert int(got[img].argmax()) == int(d["ref"][img].argmax()), f"image {img} peaks elsewhere"
    err = float((got.double() - d["ref"]).abs().max())
    rec("saliency", err)
    assert err <= ce.saliency_bar(), err
    return err


ONE_TOKEN_PRECS = ((_lib.F32, "fp32"), (_lib.BF16, "bf16"), (_lib.F16, "fp16"), (_lib.F16X2, "f16x2"))
ONE_TOKEN_SHAPES = ((128, 1), (384, 5), (1024, 1))          # D, P


def _embed(case, a, d, rec, lib):
    """one image of one token: M = P + 1 rows"""
    import test_gpu_ends_cover as ec
    slices, worst = a["slices"], 0.0
    for prec, name in ONE_TOKEN_PRECS:
        for D, P in ONE_TOKEN_SHAPES:
            t = ec.embed_inputs(D, P, slices, 1, 1)
            M = P + 1
            dv = {k: v.cuda() for k, v in t.items() if k not in ("part", "x_ref")}
            x, out = ec._nan32(M + ec.GUARD, D), nan_like(prec, M + ec.GUARD, D)
            rc = lib.vitvs_op_embed_ln(prec, ptr(x), ptr(dv["buf"]), slices, ptr(dv["bias"]), ptr(dv["pos"]), ptr(dv["cls"]),
                                       ptr(dv["reg"]) if P > 1 else None, ptr(dv["gamma"]), ptr(dv["beta"]), ptr(out), 1, 1, P, D, 1e-6,
                                       stream())
            assert rc == 0, (name, D, P, rc)
            torch.cuda.synchronize()
            x, out = x.cpu(), out.cpu()
            assert ec._all_nan(x[M:]) and ec._all_nan(out[M:]), "rows beyond M were written"
            got = values(prec, out[:M])
            assert torch.isfinite(x[:M]).all() and torch.isfinite(got).all()
            ex, eln = rel_max(x[:M], t["x_ref"]), rel_max(got, ec.layer_norm64(t["x_ref"], t["gamma"], t["beta"]))
            assert ex <= ec.BAR_X[prec] and eln <= ec.BAR_LN[prec], (name, D, P, ex, eln)
            worst = max(worst, ex / ec.BAR_X[prec], eln / ec.BAR_LN[prec])
    rec("worst_share_of_bar", worst)
    return worst


def _one_row_parts(D, slices, P=0):
    import test_gpu_ends_cover as ec
    g = ec._gen(D, slices, P, 4711)
    M = P + 1
    return dict(x0=mk((M, D), g), part=mk((slices, M, D), g, 0.5), bias=mk((D,), g, 0.3), ls=0.5 + torch.rand(D, generator=g),
                gamma=1.0 + 0.1 * mk((D,), g), beta=0.1 * mk((D,), g))


def _residual_ln(case, a, d, rec, lib):
    """M = 1 row"""
    import test_gpu_ends_cover as ec
    slices, worst = a["slices"], 0.0
    for prec, name in ONE_TOKEN_PRECS:
        for D, _ in ONE_TOKEN_SHAPES:
            t = _one_row_parts(D, slices)
            x_ref = t["x0"].double() + t["ls"].double() * (t["part"].double().sum(0) + t["bias"].double())
            x = torch.cat([t["x0"], torch.full((ec.GUARD, D), float("nan"))]).cuda()
            dv = {k: v.cuda() for k, v in t.items()}
            out = nan_like(prec, 1 + ec.GUARD, D)
            rc = lib.vitvs_op_residual_ln(prec, ptr(x), ptr(dv["part"]), slices, ptr(dv["bias"]), ptr(dv["ls"]), ptr(dv["gamma"]),
                                          ptr(dv["beta"]), ptr(out), 1, D, 1e-6, stream())
            assert rc == 0, (name, D, rc)
            torch.cuda.synchronize()
            x, out = x.cpu(), out.cpu()
            assert ec._all_nan(x[1:]) and ec._all_nan(out[1:]), "rows beyond the one row were written"
            ex = rel_max(x[:1], x_ref)
            eln = rel_max(values(prec, out[:1]), ec.layer_norm64(x[:1], t["gamma"], t["beta"]))
            assert ex <= ec.BAR_X[prec] and eln <= ec.BAR_LN[prec], (name, D, ex, eln)
            worst = max(worst, ex / ec.BAR_X[prec], eln / ec.BAR_LN[prec])
    rec("worst_share_of_bar", worst)
    return worst


def _residual_desc(case, a, d, rec, lib):
    """one image of one token: M = P + 1 rows, one patch row"""
    import test_gpu_ends_cover as ec
    slices, worst = a["slices"], 0.0
    for prec, name in ONE_TOKEN_PRECS:
        for D, P in ONE_TOKEN_SHAPES:
            M = P + 1
            t = _one_row_parts(D, slices, P)
            x_ref = t["x0"].double() + t["ls"].double() * (t["part"].double().sum(0) + t["bias"].double())
            x = torch.cat([t["x0"], torch.full((ec.GUARD, D), float("nan"))]).cuda()
            dv = {k: v.cuda() for k, v in t.items()}
            dn, sq = ec._nan32(ec.GUARD + 1 + ec.GUARD, D), ec._nan32(1, ec.GUARD + 1 + ec.GUARD)[0]
            za, zb = ec._keys(M * 64), ec._keys(M * 64)
            rc = lib.vitvs_op_residual_desc(prec, ptr(x), ptr(dv["part"]), slices, ptr(dv["bias"]), ptr(dv["ls"]), ptr(dn[ec.GUARD:]),
                                            ptr(sq[ec.GUARD:]), ptr(za), ptr(zb), M * 64, 1, P, M, D, stream())
            assert rc == 0, (name, D, P, rc)
            torch.cuda.synchronize()
            ec._check_keys(za, zb, M * 64, case.id)
            xc, dc, sc = x.cpu(), dn.cpu(), sq.cpu()
            assert ec._all_nan(xc[M:]), "rows of x beyond M were written"
            assert ec._all_nan(dc[:ec.GUARD]) and ec._all_nan(dc[ec.GUARD + 1:]), "dn was written outside its one patch row"
            assert ec._all_nan(sc[:ec.GUARD]) and ec._all_nan(sc[ec.GUARD + 1:]), "sq was written outside its one word"
            row = xc[P:M]
            ex = rel_max(xc[:M], x_ref)
            edn, esq = rel_max(dc[ec.GUARD:ec.GUARD + 1], ec.dn_ref(row)), rel_max(sc[ec.GUARD:ec.GUARD + 1], ec.sq_ref(row))
            assert ex <= ec.BAR_X[prec] and edn <= ec.BAR["epilogue_dn"] and esq <= ec.BAR["epilogue_sq"], (name, D, P, ex, edn, esq)
            worst = max(worst, ex / ec.BAR_X[prec], edn / ec.BAR["epilogue_dn"], esq / ec.BAR["epilogue_sq"])
    rec("worst_share_of_bar", worst)
    return worst


DRIVERS = {
    "vitvs_op_rig_law": _rig, "vitvs_op_rig_robust_law": _robust, "vitvs_op_pose_rig_law": _pose_rig, "vitvs_op_pose_law": _pairs_law,
    "vitvs_op_pose_consensus_law": _pairs_law, "vitvs_op_homography_law": _pairs_law, "vitvs_op_homography_consensus_law": _pairs_law,
    "vitvs_op_best_order_dev": _best,
}
LIB_DRIVERS = {
    "vitvs_op_gram_stencil": _stencil, "vitvs_op_gram_argmax": _argmax, "vitvs_op_quarter_turns": _turns,
    "vitvs_op_normalize_rows": _normalize, "vitvs_op_saliency": _saliency, "vitvs_op_embed_ln": _embed,
    "vitvs_op_residual_ln": _residual_ln, "vitvs_op_residual_desc": _residual_desc,
}


@pytest.mark.parametrize("case", ce.CASES, ids=[c.id for c in ce.CASES])
def test_the_hook_keeps_the_headers_word_at_this_end(lib, record_property, case):
    a, d = ce.resolve(case.args), ce.build(case.id)

    def rec(what, err):
        record_property(what, f"{err:.3e}")
    if case.hook in DRIVERS:
        err = DRIVERS[case.hook](case, a, d, rec)
    else:
        err = LIB_DRIVERS[case.hook](case, a, d, rec, lib)
    print(f"{case.id}: {case.end} of {case.hook}, worst error {err:.3e}")
