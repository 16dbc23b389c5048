"""The table of contract ends (tests/contract_ends_cases.py) against include/vitvs_ops.h, without a GPU.

Every quoted sentence is in the header; every plan's largest admitted size and first refused one is found by bisecting the plan
hook and equals the header's formula; every case's reference is conditioned well enough that the device test tests the kernel
and not the input; every hook that states a range has both of its ends in the table, run or cited; every cited test exists."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import contract_ends_cases as ce
import rig_ref as rg
import select_ref as sref
from op_support import ROOT
from op_support import host_lib as lib  # noqa: F401

KIB160 = 160 * 1024


def _header():
    with open(os.path.join(ROOT, "include", "vitvs_ops.h")) as f:
        text = f.read()
    return " ".join(re.sub(r"^\s*(/\*|\*/|\*)", " ", line) for line in text.splitlines()).replace("*/", " ")


def _norm(s):
    return " ".join(s.split())


def test_every_quoted_sentence_is_in_the_header():
    header = _norm(_header())
    for entry in ce.CASES + ce.CITED:
        assert _norm(entry.sentence) in header, (entry, "is not a sentence of include/vitvs_ops.h")
    assert len({c.id for c in ce.CASES}) == len(ce.CASES)
    assert {c.end for c in ce.CASES} <= {"smallest", "largest", "first_refused"}


def test_every_hook_that_states_a_range_has_its_ends_in_the_table():
    header = _header()
    for hook, ends in ce.ENDS.items():
        assert re.search(r"\b%s\(" % hook, header), hook
        have = {c.end for c in ce.CASES if c.hook == hook} | {c.end for c in ce.CITED if c.hook == hook}
        assert set(ends) <= have, (hook, "ends without a case or a citation:", set(ends) - have)
    assert {c.hook for c in ce.CASES} | {c.hook for c in ce.CITED} <= set(ce.ENDS)
    # every hook the header declares is in ENDS or, with the test that covers it (None: no device launch of its own), in EXCLUDED
    declared = set(re.findall(r"\bVITVS_API\s+int\s+(vitvs_op_\w+)\(", header))
    assert declared == set(ce.ENDS) | set(ce.EXCLUDED), declared ^ (set(ce.ENDS) | set(ce.EXCLUDED))
    assert not set(ce.ENDS) & set(ce.EXCLUDED)
    for hook, test in ce.EXCLUDED.items():
        if test is not None:
            path, name = test.split("::")
            with open(os.path.join(ROOT, path)) as f:
                assert re.search(r"^def %s\(" % name, f.read(), re.M), (hook, test)
    for c in ce.CASES:
        assert (c.rc == 0) == (c.end != "first_refused"), c.id


def test_every_cited_test_exists():
    for c in ce.CITED:
        path, name = c.test.split("::")
        with open(os.path.join(ROOT, path)) as f:
            assert re.search(r"^def %s\(" % name, f.read(), re.M), c.test


def test_plan_ends_equal_the_headers_formulas(lib):
    b = ce.bounds()

    def last(bytes_of):
        r = 1
        while bytes_of(r + 1) <= KIB160:
            r += 1
        return (r, r + 1)
    # "8 (320 + (n_iter > 0 ? 2 max_rows : 0))" and its kin, within 160 KiB
    assert b["pose"] == last(lambda r: 8 * (320 + 2 * r)) == (10080, 10081)
    assert b["pose_consensus"] == last(lambda r: 8 * (320 + 2 * r + 8 + (r + 1) // 2))
    assert b["homography"] == last(lambda r: 8 * (752 + 2 * r))
    assert b["homography_consensus"] == last(lambda r: 8 * (752 + 2 * r + 8 + (r + 1) // 2))
    assert b["pose_rig"] == last(lambda ld: 8 * (320 + 2 * 256 * ld))
    assert b["rig_robust"] == last(lambda ld: 8 * (260 + 2 * 256 * (ld // 2)) if 256 * ld > 384 else 0)
    out = (C.c_int32 * 8)()
    for name, args in (("pose", (1,)), ("pose_consensus", (1, 64)), ("homography", (1,)), ("homography_consensus", (1, 64))):
        fn = getattr(lib, f"vitvs_op_{name}_plan")
        assert fn(b[name][0], *args, out) == 0 and out[0] <= KIB160 and out[2] == 1          # the opt-in beyond 64 KiB
        assert fn(b[name][1], *args, out) == -3 and out[0] > KIB160
    # the servo plan states no formula: its own out[3] is on either side of 160 KiB
    assert lib.vitvs_op_servo_plan(196, b["servo"][0], 4, 0, 0, out) == 0 and out[3] <= KIB160
    assert lib.vitvs_op_servo_plan(196, b["servo"][1], 4, 0, 0, out) == -3 and out[3] > KIB160
    # the best order has no plan hook: T keys on the next power of two; the refusal comes before any device call
    assert b["best_order"] == (128 * 128, 129 * 129)
    assert ce.best_order_lds(b["best_order"][0]) <= KIB160 < ce.best_order_lds(b["best_order"][1])
    buf = (C.c_int32 * 4)()
    p = C.cast(buf, C.c_void_p)
    assert lib.vitvs_op_best_order_dev(b["best_order"][1], 16, 1, p, p, p, p, None) == -3
    # "2 T + P floats pass 64 KiB"
    for P in (1, 5):
        T, T1 = b[f"saliency_p{P}"]
        assert (2 * T + P) * 4 <= 65536 < (2 * T1 + P) * 4 and T1 == T + 1
    # every size of a device case at a plan's end is looked up, not typed
    for c in ce.CASES:
        if c.sentence in (ce.S_ROBUST_PLAN, ce.S_POSE_PLAN, ce.S_POSE_CONS_PLAN, ce.S_HOMOGRAPHY_PLAN, ce.S_HOMOGRAPHY_CONS_PLAN,
                          ce.S_POSE_RIG_PLAN, ce.S_SALIENCY_LDS, ce.S_BEST):
            assert any(isinstance(v, str) and v.startswith("@") for v in c.args.values()), c.id
            assert all(isinstance(v, (int, tuple)) for v in ce.resolve(c.args).values() if not isinstance(v, str)), c.id


@pytest.mark.parametrize("T", [1, 4, 9, 16, 196, 289, 484])
def test_the_sort_based_rank_is_the_definition(T):
    rng = np.random.default_rng(T)
    for cells in (1, 2, 4, 16):
        nn1, nn2 = rng.integers(-1, T + 1, T), rng.integers(0, T, T)
        nn2[nn1[: T // 2].clip(0, T - 1)] = np.arange(T // 2)
        sim = rng.uniform(0.1, 0.9, T).astype(np.float32)
        sim[rng.integers(0, T, T // 3)] = np.float32(0.625)          # exact ties
        sim[rng.integers(0, T, 3)] = 0.0
        sim[rng.integers(0, T, 3)] = -0.0
        for a, b in zip(ce.sorted_ranks(nn1, nn2, sim, cells), sref.ranks(nn1, nn2, sim, cells)):
            assert np.array_equal(a, b), (T, cells)
        assert np.array_equal(ce.sorted_best_order(nn1, nn2, sim, cells), sref.best_order(nn1, nn2, sim, cells))


_BUILT = [c for c in ce.CASES if c.rc == 0 and c.hook in ce._BUILDERS]


@pytest.mark.parametrize("case", _BUILT, ids=[c.id for c in _BUILT])
def test_the_reference_alone_is_well_conditioned(case):
    d = ce.build(case.id)
    a = ce.resolve(case.args)
    if case.hook == "vitvs_op_rig_law":
        for ref, solver in [(d["ref"], d["solver"])] + ([(d["small_ref"], "ldlt")] if "small" in d else []):
            margin = rg.ldlt_margin(ref["M"])
            assert (margin >= 100) if solver == "ldlt" else (margin <= 0.01), (solver, margin)
            if solver == "jacobi":     # numpy's pinv cuts at 1e-15 of the largest singular value: none may sit near the cut
                sv = np.linalg.svd(ref["M"], compute_uv=False)
                assert ((sv >= 1e-6 * sv[0]) | (sv <= 1e-16 * sv[0])).all(), sv / sv[0]
        rows = [L.shape[0] for L in d["case"]["Ls"]]
        if a["n"] > 2 and a["kind"] == "mixed":
            assert rows[0] == 0 and rows[a["n"] // 2] == 0 and rows[-1] == 0 and len(set(rows)) > 1 or a["ld"] == 1
    elif case.hook == "vitvs_op_rig_robust_law":
        import test_gpu_rig_robust_op as rro
        if a.get("kind") == "turning":
            M, _ = rg.stacked(d["case"]["Ls"], d["case"]["es"], d["case"]["Ws"], rg.statuses(d["case"]))
            sv = np.linalg.svd(M, compute_uv=False)
            assert ((sv >= 1e-6 * sv[0]) | (sv <= 1e-16 * sv[0])).all() and (sv >= 1e-6 * sv[0]).sum() == 3, sv / sv[0]
        if d["solver"] != "none":
            assert rro._fair(d["ref"]["margins"], d["solver"]), (d["solver"], d["ref"]["margins"])
            assert d["ref"]["margin"] >= 1e-6, d["ref"]["margin"]
    elif case.hook == "vitvs_op_pose_rig_law":
        for n_iter, ref in d["refs"].items():
            degenerate = ref["info"][1] < 3
            for g in ref["gaps"]:
                assert g >= 1e-6 or (degenerate and g <= 1e-10), (n_iter, ref["gaps"])
            assert ref["edge"] >= 1e-6, (n_iter, ref["edge"])
            if not degenerate:
                assert ref["status"] == 0 and ref["info"][3] == n_iter
        if a["n"] > 4:
            assert d["refs"][0]["info"][0] < a["n"] and (d["refs"][0]["info"][6] > 0 or a["ld"] <= 8)   # cameras left out, holes met
    elif case.hook in ("vitvs_op_pose_law", "vitvs_op_pose_consensus_law", "vitvs_op_homography_law",
                       "vitvs_op_homography_consensus_law"):
        assert ce.pairs_law_conditioned(case.hook, a, d["refs"]) is None, (d["salt"], ce.pairs_law_conditioned(case.hook, a, d["refs"]))
        for (n_hyp, n_iter), refs in d["refs"].items():
            if a["ld"] >= 1000 and n_iter:                      # the median and the re-weighting do work at the large size
                assert refs[0]["info"][3] >= a["ld"] // 40 and refs[0]["info"][0] < a["ld"]
        if a["pairs"] > 1:                                      # each pair has its own answer, and its own unusable rows
            assert a["ld"] < 24 or len({tuple(u) for u in d["case"]["usable"]}) >= min(a["pairs"], 20)
            vs = np.stack([r["v"] for r in next(iter(d["refs"].values()))])
            assert len(np.unique(vs.round(6), axis=0)) == a["pairs"]
    elif case.hook == "vitvs_op_best_order_dev":
        for cells, want in d["want"].items():
            assert sorted(want) == list(range(a["T"]))
            if a["T"] <= 484:
                assert np.array_equal(want, sref.best_order(*d["tables"], cells))
        if a["kind"] == "flat":
            assert not sref.mutual_mask(*d["tables"][:2]).any() and np.array_equal(d["want"][1], np.arange(a["T"]))
    elif case.hook == "vitvs_op_gram_stencil":
        from test_gpu_correspond_cover import MARGIN
        assert MARGIN == ce.MARGIN
        for P, e in d.items():
            assert ce.clear_everywhere(e["S"], MARGIN, e["ties_r"], e["ties_c"]), (P, e["salt"])
            for i, j in e["ties_r"].items():
                assert e["S"][i].argmax() == j and (e["S"][i] == e["S"][i].max()).sum() >= 2
            for j, i in e["ties_c"].items():
                assert e["S"][:, j].argmax() == i and (e["S"][:, j] == e["S"][:, j].max()).sum() >= 2
            if a["kind"] == "neg":
                assert e["S"].max() < 0
            if a["kind"] == "ties":
                for i in (11, 15, 58):          # one tile (10, 14) and the next (57); likewise the rows
                    assert sorted(np.nonzero(e["S"][i] == e["S"][i].max())[0]) == [10, 14, 57]
                for j in (10, 14, 57):
                    assert sorted(np.nonzero(e["S"][:, j] == e["S"][:, j].max())[0]) == [11, 15, 58]
            assert np.isfinite(e["S"]).all() and torch.isnan(e["x"][:, :P]).all()
    elif case.hook == "vitvs_op_gram_argmax":
        for key, e in d.items():
            assert all(ce.clear_everywhere(S, ce.MARGIN) for S in e["S"]), (key, e["salt"])
    elif case.hook == "vitvs_op_saliency":
        top = torch.sort(d["ref"], dim=1).values
        assert float((top[:, -1] - top[:, -2]).min()) >= 10 * ce.saliency_bar(), "the peak could move within the bar"
        assert float((top[:, 1] - top[:, 0]).min()) > 0.0


def test_measured_errors_are_not_understated():
    """The bar table's figures (contract_ends_cases.MEASURED), re-measured: the plain torch fp32 statement against fp64."""
    worst = 0.0
    for case in ce.CASES:
        if case.hook == "vitvs_op_saliency" and case.rc == 0:
            d = ce.build(case.id)
            worst = max(worst, float((d["f32"].double() - d["ref"]).abs().max()))
    assert worst <= ce.MEASURED["saliency"], worst
    assert ce.MEASURED["saliency"] <= 2 * worst, "overstated"
    sim, arg = ce.stencil_f32_errors()
    assert sim <= ce.MEASURED["stencil_norm_sim"] <= 2 * sim, sim
    assert arg <= ce.MEASURED["stencil_norm_argmax"] <= 2 * arg, arg
    err = ce.normalize_f32_error()
    assert err <= ce.MEASURED["normalize"] <= 2 * err, err
    import test_gpu_correspond_cover as cc
    import test_gpu_ends_cover as ec
    assert (ce.ARGMAX_TOL, ce.SIM_TOL, ce.MARGIN) == (cc.ARGMAX_TOL, cc.SIM_TOL, cc.MARGIN)
    assert (ce.SALIENCY_CAP, ce.NORMALIZE_CAP) == (ec.CAP["saliency"], ec.CAP["normalize"])
