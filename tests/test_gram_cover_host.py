"""CPU-side coverage check of tests/test_gpu_correspond_cover.py: every Gram plan the product can reach has a GPU case.

vitvs_op_gram_plan is host arithmetic (correspond.hip plan_gram): no device calls here.  The walk is tools/plan_cover.py's
domain (every model, 224/308/448/518 inputs at stride patch and patch/2, the four precisions) with binned descriptors on and
off, every pair count whose forward fits its 1 .. 16 frames with and without a shared goal, and handles of max_pairs = n_pairs
and 16.  A plan key is the form, tile and k-groups, and whether the call has one pair, several with their own goals or several
sharing one goal; the 9 D-wide form of binned descriptors shares the keys of the fused arg-max it launches."""
import importlib.util
import os

import pytest

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib
from op_support import host_lib as lib  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _module(name, path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def cover():
    return _module("plan_cover", os.path.join("tools", "plan_cover.py"))


@pytest.fixture(scope="module")
def gpu_cases():
    return _module("gpu_correspond_cover", os.path.join("tests", "test_gpu_correspond_cover.py"))


def reachable_keys(lib, cover, cases):
    """{gram key: the first product shape that reaches it}."""
    keys = {}
    for prec in cover.PRECISIONS:
        for model, size, stride, cfg in cover.geometries():
            for binned in (0, 1):
                for shared in (False, True):
                    for n in range(1, 16):
                        if (1 if shared else n) + n > max(cover.FRAMES):
                            break
                        for max_pairs in sorted({n, 16}):
                            rc, plan = cases.gram_plan(lib, prec, binned, cfg.tokens, cfg.dim, n, max_pairs)
                            assert rc == 0, (model, size, stride, prec, binned, n, max_pairs, plan)
                            key = cases.gram_key(plan, n, shared)
                            keys.setdefault(key, f"{cover.PREC_NAMES[prec]} {model} {size}/{stride} binned={binned} "
                                                 f"pairs={n} shared={shared} max_pairs={max_pairs}")
    return keys


def test_every_reachable_gram_plan_has_a_gpu_case(lib, cover, gpu_cases):
    reach = reachable_keys(lib, cover, gpu_cases)
    covered = {}
    for case in gpu_cases.CASES:
        rc, plan = gpu_cases.gram_plan(lib, *gpu_cases.plan_args(case))
        covered.setdefault(gpu_cases.gram_key(plan, case.pairs, case.shared), case.id)
    missing = [f"{gpu_cases.key_id(k)} (reached by {where})" for k, where in sorted(reach.items()) if k not in covered]
    assert not missing, "Gram plans without a case in tests/test_gpu_correspond_cover.py: " + "; ".join(missing)
    # the walk reaches the three forms, each with both of its tiles
    assert {(k[0], k[1]) for k in reach} == {(1, 32), (1, 64), (2, 64), (2, 128), (3, 32), (3, 64)}


def test_every_gpu_case_plans_its_family(lib, gpu_cases):
    for case in gpu_cases.CASES:
        rc, plan = gpu_cases.gram_plan(lib, *gpu_cases.plan_args(case))
        assert rc == 0 and tuple(plan[:4]) == case.family, (case.id, plan)
        assert plan[6] == (case.family[0] == gpu_cases.GRAM_SPLIT), case.id
        if case.op == "stencil":
            assert case.T == round(case.T ** 0.5) ** 2 and case.P >= 1, case.id


def test_gram_plan_switch_points(lib, gpu_cases):
    plan = lambda *a: gpu_cases.gram_plan(lib, *a)[1]  # noqa: E731
    # fp32 fused arg-max: 32 x 32 tiles with two k-groups up to 512 tokens when Dp / 32 is even
    assert plan(_lib.F32, 0, 512, 64, 1, 1)[:4] == [1, 32, 32, 2] and plan(_lib.F32, 0, 513, 64, 1, 1)[:4] == [1, 64, 64, 1]
    assert plan(_lib.F32, 0, 200, 96, 1, 1)[:4] == [1, 64, 64, 1]
    # 16-bit modes split from 1024 tokens; 128 x 128 tiles from ceil(T / 128)^2 * n_pairs = 256 on
    assert plan(_lib.BF16, 0, 1023, 64, 1, 1)[0] == 1 and plan(_lib.F16, 0, 1024, 64, 1, 1)[0] == 2
    assert plan(_lib.BF16, 0, 1024, 64, 3, 3)[:4] == [2, 64, 64, 1] and plan(_lib.BF16, 0, 1024, 64, 4, 4)[:4] == [2, 128, 128, 1]
    assert plan(_lib.BF16, 0, 1024, 96, 1, 1)[:4] == [1, 64, 64, 1]      # the split needs Dp % 64 == 0
    assert plan(_lib.F16X2, 0, 3136, 768, 1, 1)[0] == 1 and plan(_lib.F32, 0, 3136, 768, 1, 1)[0] == 1
    # binned: the stencil up to 8 GiB of raw Gram over the handle's pairs, the 9 D-wide descriptors beyond (whose split would
    # pass the 4 GiB of 32-bit operand offsets wherever the stencil does not fit)
    assert plan(_lib.BF16, 1, 3136, 768, 1, 218)[:4] == [3, 64, 64, 1]
    assert plan(_lib.BF16, 1, 3136, 768, 1, 219) == [4, 64, 64, 1, 17, 301, 0]
    assert plan(_lib.F32, 1, 3136, 768, 1, 219)[:4] == [4, 64, 64, 1]
    # band rows and workgroups per XCD (correspond.hip gram_band_rows): 3136 tokens, 625 tiles of 128 x 128
    assert plan(_lib.BF16, 0, 3136, 768, 1, 1)[4:6] == [9, 79]


def test_gram_plan_hook_refuses_what_it_cannot_plan(lib, gpu_cases):
    assert gpu_cases.gram_plan(lib, _lib.F32, 0, 0, 64, 1, 1)[0] == -2
    assert gpu_cases.gram_plan(lib, _lib.F32, 0, 196, 64, 0, 1)[0] == -2
    assert gpu_cases.gram_plan(lib, _lib.F32, 0, 196, 64, 2, 1)[0] == -2          # more pairs than the handle holds
    assert gpu_cases.gram_plan(lib, _lib.F32, 0, 196, 48, 1, 1)[0] == -2          # Dp not a multiple of 32
