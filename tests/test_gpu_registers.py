"""DINOv2 with register tokens (dinov2_vit{s,b,l}14_reg) on the device, against the CPU restatement of the register forward
(tests/registers_ref.py, itself pinned to HF Dinov2WithRegistersModel in tests/test_registers_host.py).  The bars and the
acceptance rule are tests/test_gpu_path.py's: tokens to 2e-5 of their largest magnitude in fp32 / f16x2 (2e-2 in bf16),
arg-max tables bit-exact on a pair whose top-1 / top-2 margins are >= 1e-4 (4 <= mutual < T, mean(sim_1) <= 0.99), v_c to 1e-9
relative L2 (the law runs in fp64 on both sides)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib, config, synth, weights
from vitvs_amd.engine import Engine
from oracle import servo_ref as sr

import registers_ref as rr
from robust_ref import rel_l2

pytestmark = pytest.mark.gpu

EXACT = ["fp32", "f16x2"]
TOKEN_BARS = {"fp32": 2e-5, "f16x2": 2e-5, "bf16": 2e-2}
FRAME_SEED = 20250738        # synth.ACCEPTED_FRAME_SEEDS["vits14_308"]: meets the acceptance rule with the registers too (asserted)
REG = "dinov2_vits14_reg"


def _rel_max(got, ref):
    return float((got - ref).abs().max() / ref.abs().max())


_MEMO = {}


def _default_case():
    """The reference default plus registers: ViT-S/14 at 308², 12 blocks, synthetic weights (seed 0), the accepted frame pair,
    and the restatement's tokens of that pair (computed once)."""
    if "case" not in _MEMO:
        cfg = config.vit_config(REG, 308)
        sd = weights.synthetic_state_dict(cfg, 0)
        des, cur = synth.frame_pair(cfg.img_size, FRAME_SEED)
        toks = rr.tokens(cfg, sd, np.stack([des, cur]))
        _MEMO["case"] = cfg, sd, des, cur, toks
    return _MEMO["case"]


@pytest.mark.parametrize("precision", ["fp32", "f16x2", "bf16"])
def test_forward_tokens_of_the_register_model(precision):
    cfg, sd, des, cur, ref = _default_case()
    eng = Engine(cfg, precision=precision, max_pairs=1).load_state_dict(sd)
    got = eng.forward_tokens(np.stack([des, cur])).cpu()
    assert got.shape == ref.shape == (2, 489, 384)
    err = _rel_max(got, ref)
    print(f"{REG} 308 {precision}: tokens max abs err / max abs = {err:.2e}")
    assert err <= TOKEN_BARS[precision]
    if precision in EXACT:   # the registers move the patch tokens by far more than the bar (measured 7.6e-3 of the largest)
        plain = {k: v for k, v in sd.items() if k != "register_tokens"}
        if "plain" not in _MEMO:
            _MEMO["plain"] = rr.tokens(dataclasses.replace(cfg, registers=0), plain, np.stack([des, cur]))
        assert _rel_max(got[:, 5:], _MEMO["plain"][:, 1:]) > 100 * TOKEN_BARS[precision]
    eng.close()


@pytest.mark.parametrize("precision", ["fp32", "f16x2", "bf16"])
def test_forward_tokens_long_sequence(precision):
    """ViT-L/14 with registers at 518²: 1 + 4 + 1369 = 1374 rows, the long-sequence attention (key-range split and its workspace
    in the 16-bit modes) at a row count no plain configuration has; two blocks."""
    cfg = config.vit_config("dinov2_vitl14_reg", 518, layer=1)
    assert cfg.seq == 1374
    sd = weights.synthetic_state_dict(cfg, 1)
    frames = np.stack(synth.frame_pair(cfg.img_size, 5))
    if "l14" not in _MEMO:
        _MEMO["l14"] = rr.tokens(cfg, sd, frames)
    ref = _MEMO["l14"]
    eng = Engine(cfg, config.ServoParams(dino_input_size=518, use_feature_binning=False), precision=precision,
                  max_pairs=1).load_state_dict(sd)
    got = eng.forward_tokens(frames).cpu()
    assert got.shape == ref.shape == (2, 1374, 1024)
    err = _rel_max(got, ref)
    print(f"dinov2_vitl14_reg 518 {precision}: tokens max abs err / max abs = {err:.2e}")
    assert err <= TOKEN_BARS[precision]
    eng.close()


def test_zero_registers_through_create_ex_is_bit_identical(monkeypatch):
    """vitvs_create_ex(cfg, 0, ...) is vitvs_create: the same tokens and twist, bit for bit (ViT-S/16 at 224²)."""
    cfg = config.baseline_config("vits16_224")
    sd = weights.synthetic_state_dict(cfg, 0)
    params = config.ServoParams(dino_input_size=cfg.img_size, use_feature_binning=False)
    des, cur = synth.frame_pair(cfg.img_size, synth.ACCEPTED_FRAME_SEEDS["vits16_224"])
    depth = synth.depth_pattern()
    outs = []
    for via_ex in (False, True):
        lib = _lib.load()
        if via_ex:
            monkeypatch.setattr(lib, "vitvs_create", lambda c, out: lib.vitvs_create_ex(c, 0, out))
        eng = Engine(cfg, params, precision="fp32", max_pairs=1, max_rows=cfg.tokens).load_state_dict(sd)
        assert lib.vitvs_register_tokens(eng.handle) == 0
        toks = eng.forward_tokens(np.stack([des, cur])).cpu()
        v, st = eng.compute_velocity(cur, des, depth, params.intrinsics(), mode=_lib.SELECT_DENSE)
        outs.append((toks, v.cpu(), st.cpu(), eng.last_details(1)))
        eng.close()
        monkeypatch.undo()
    (t0, v0, s0, d0), (t1, v1, s1, d1) = outs
    assert torch.equal(t0, t1) and torch.equal(v0, v1) and torch.equal(s0, s1)
    assert np.array_equal(d0["nn_1"], d1["nn_1"]) and np.array_equal(d0["nn_2"], d1["nn_2"])


@pytest.mark.parametrize("precision", EXACT)
def test_descriptors_and_facets_skip_the_registers(precision):
    """The velocity path's own descriptors (plain and binned), and every facet plain, with the cls row and binned: patch rows
    only, the registers never appear (include_cls: [cls, patches])."""
    cfg = config.vit_config(REG, 308, layer=3)
    sd = weights.synthetic_state_dict(cfg, 11)
    frames = np.stack(synth.frame_pair(cfg.img_size, 4242))
    tol = TOKEN_BARS[precision]
    toks = rr.tokens(cfg, sd, frames)
    engines = {}
    for binned in (False, True):
        eng = Engine(cfg, config.ServoParams(dino_input_size=cfg.img_size, use_feature_binning=binned), precision=precision,
                      max_pairs=1).load_state_dict(sd)
        engines[binned] = eng
        got = eng.extract_descriptors(frames).cpu()[:, 0]
        want = rr.descriptors(cfg, sd, frames, bin=binned, toks=toks)
        assert got.shape == want.shape == (2, cfg.tokens, cfg.dim * (9 if binned else 1))
        assert _rel_max(got, want) <= tol, binned
    engines[True].close()
    eng = engines[False]
    for facet in ("query", "key", "value", "token"):
        for bin_, cls in ((False, False), (False, True), (True, False)):
            want = rr.facet(cfg, sd, frames, facet, bin=bin_, include_cls=cls)
            got = eng.extract_descriptors(frames, facet=facet, bin=bin_, include_cls=cls).cpu()[:, 0]
            assert got.shape == want.shape == (2, cfg.tokens + int(cls), cfg.dim * (9 if bin_ else 1))
            assert _rel_max(got, want) <= tol, (facet, bin_, cls)
    eng.close()


def _accepted_reference(cfg, sd, des, cur, toks, params, depth, seed):
    d = rr.descriptors(cfg, sd, None, bin=True, toks=toks)
    S = sr.cosine_matrix(d[0], d[1], exact_order=False)
    mr, mc = sr.argmax_margins(S)
    ref = sr.servo_update(d[0], d[1], depth, num_pairs=params.num_pairs, input_size=cfg.img_size, u_max=params.u_max,
                          v_max=params.v_max, fx=params.f_x, fy=params.f_y, lam=params.lambda_,
                          generator=torch.Generator().manual_seed(seed))
    corr = ref["corr"]
    nn1, nn2 = corr["nn_1"].numpy(), corr["nn_2"].numpy()
    mutual = int((nn2[nn1] == np.arange(cfg.tokens)).sum())
    assert min(mr, mc) >= 1e-4 and 4 <= mutual < cfg.tokens and float(corr["sim_1"].mean()) <= 0.99   # the acceptance rule
    assert ref["status"] == "ok" and not corr["same_image"]
    # the reference's draw as a visiting order: its selected candidates first, then every other token
    sel = corr["selected"].numpy().astype(np.int32)
    order = np.concatenate([sel, np.setdiff1d(np.arange(cfg.tokens), sel)]).astype(np.int32)
    return ref, order


@pytest.mark.parametrize("precision", EXACT)
def test_reference_default_with_registers_end_to_end(precision):
    """ViT-S/14 308² binned (the reference's shipped configuration) on the register checkpoint: bit-exact arg-max tables, the
    reference's twist under the reference's draw, the same through the host-pointer seam, and a cached goal equal to the
    recomputing call."""
    cfg, sd, des, cur, toks = _default_case()
    params = config.ServoParams(dino_input_size=cfg.img_size, use_feature_binning=True)
    depth = synth.depth_pattern()
    ref, order = _accepted_reference(cfg, sd, des, cur, toks, params, depth, seed=7)
    eng = Engine(cfg, params, precision=precision, max_pairs=1).load_state_dict(sd)
    v, st = eng.compute_velocity(cur, des, depth, params.intrinsics(), mode=_lib.SELECT_ORDER, selection=order[None])
    det = eng.last_details(1)
    assert int(st[0]) == 0
    assert np.array_equal(det["nn_1"][0], ref["corr"]["nn_1"].numpy())
    assert np.array_equal(det["nn_2"][0], ref["corr"]["nn_2"].numpy())
    k = params.num_pairs
    assert np.array_equal(det["selected"][0, :k], ref["corr"]["selected"].numpy())
    v = v.cpu().numpy()[0].copy()
    assert rel_l2(v, ref["v_c"]) <= 1e-9
    # the host-pointer entry point: the same bits
    v_h, st_h = eng.compute_velocity_host(cur, des, depth, np.array(params.intrinsics()), mode=_lib.SELECT_ORDER,
                                          selection=order[None])
    assert int(st_h[0]) == 0 and np.array_equal(v_h[0], v)
    # a cached goal: the current frame alone goes through the network
    eng.set_goal(des)
    v_g, st_g = eng.compute_velocity(cur, None, depth, params.intrinsics(), mode=_lib.SELECT_ORDER, selection=order[None])
    det_g = eng.last_details(1)
    assert int(st_g[0]) == 0
    assert np.array_equal(det_g["nn_1"], det["nn_1"]) and np.array_equal(det_g["nn_2"], det["nn_2"])
    assert rel_l2(v_g.cpu().numpy()[0], v) <= 1e-9
    eng.close()


def test_saliency_attends_over_the_registers():
    """The class token's softmax runs over all 1 + R + T keys; the patch columns are kept (trained-like weights: peaked rows)."""
    cfg = config.vit_config(REG, 308, layer=3)
    sd = weights.trained_like_state_dict(cfg, 5)
    frames = np.stack(synth.frame_pair(cfg.img_size, 99))
    want = rr.saliency_maps(cfg, sd, frames)
    eng = Engine(cfg, config.ServoParams(dino_input_size=cfg.img_size, use_feature_binning=False), precision="fp32",
                  max_pairs=1).load_state_dict(sd)
    fr = torch.from_numpy(frames).to(eng.device)
    heads = (C.c_int32 * 4)(0, 2, 4, 5)
    got = torch.empty((2, cfg.tokens), dtype=torch.float32, device=eng.device)
    rc = eng.lib.vitvs_extract_saliency_dev(eng.handle, 2, C.c_void_p(fr.data_ptr()), 4, heads, C.c_void_p(got.data_ptr()),
                                            C.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream))
    assert rc == 0, _lib.last_error(eng.handle)
    got = got.cpu()
    assert float(got.min()) == 0.0 and float(got.max()) == 1.0
    assert float((got - want).abs().max()) <= 2e-4                           # tests/test_gpu_path.py SALIENCY_BARS["fp32"]
    eng.close()


def test_pipeline_with_borrowed_weights_equals_a_lone_engine():
    from vitvs_amd.engine import VitvsError
    from vitvs_amd.pipeline import UpdatePipeline
    cfg, sd, des, cur, _ = _default_case()
    params = config.ServoParams(dino_input_size=cfg.img_size, use_feature_binning=True)
    dev = torch.device("cuda", torch.cuda.current_device())
    Ic, Id = torch.from_numpy(cur[None]).to(dev), torch.from_numpy(des[None]).to(dev)
    Z = torch.from_numpy(synth.depth_pattern()[None]).to(dev)
    K = torch.tensor([params.intrinsics()], dtype=torch.float64, device=dev)
    lone = Engine(cfg, params, precision="f16x2", max_pairs=1, max_rows=cfg.tokens).load_state_dict(sd)
    lone.set_option("in_flight", 4)                                          # the tile plan the pipeline's slots run
    v_ref, st_ref = lone.compute_velocity(cur, des, synth.depth_pattern(), params.intrinsics(), mode=_lib.SELECT_DENSE)
    pipe = UpdatePipeline(cfg, params, sd, precision="f16x2", depth=4, max_rows=cfg.tokens, device=dev)
    assert all(e.lib.vitvs_register_tokens(e.handle) == 4 for e in pipe.engines)
    tickets = [pipe.submit(Ic, Id, Z, K, _lib.SELECT_DENSE) for _ in range(4)]
    for t in tickets:
        v, st = pipe.result(t)
        assert torch.equal(v.cpu(), v_ref.cpu()) and torch.equal(st.cpu(), st_ref.cpu())
    pipe.close()
    # borrowing across different register counts is refused: the same geometry, another network
    plain = config.vit_config("dinov2_vits14", 308)
    other = Engine(plain, params, precision="f16x2", max_pairs=1).load_state_dict(weights.synthetic_state_dict(plain, 0))
    borrower = Engine(cfg, params, precision="f16x2", max_pairs=1)
    with pytest.raises(VitvsError, match="register"):
        borrower.share_weights(other)
    with pytest.raises(VitvsError):
        Engine(plain, params, precision="f16x2", max_pairs=1).share_weights(lone)
    for e in (lone, other, borrower):
        e.close()


def test_register_tokens_upload_is_checked():
    cfg, sd, _, _, _ = _default_case()
    eng = Engine(cfg, precision="fp32", max_pairs=1)
    lib, h = eng.lib, eng.handle
    for name, t in sd.items():
        if name == "register_tokens":
            continue
        if name == "pos_embed":
            t = weights.resample_pos_embed(t, cfg.grid)
        elif name.startswith("blocks.") and int(name.split(".")[1]) >= cfg.blocks_run:
            continue
        a = np.ascontiguousarray(t.numpy())
        assert lib.vitvs_set_tensor(h, name.encode(), a.ctypes.data_as(C.c_void_p), a.size) == 0, name
    assert lib.vitvs_weights_ready(h) == -4 and "register_tokens" in _lib.last_error(h)
    reg = np.ascontiguousarray(sd["register_tokens"].numpy())
    assert lib.vitvs_set_tensor(h, b"register_tokens", reg.ctypes.data_as(C.c_void_p), reg.size - 1) == -5
    assert lib.vitvs_weights_ready(h) == -4
    assert lib.vitvs_set_tensor(h, b"register_tokens", reg.ctypes.data_as(C.c_void_p), reg.size) == 0
    assert lib.vitvs_weights_ready(h) == 0
    eng.close()
    plain = config.vit_config("dinov2_vits14", 308)
    eng0 = Engine(plain, precision="fp32", max_pairs=1)
    assert eng0.lib.vitvs_set_tensor(eng0.handle, b"register_tokens", reg.ctypes.data_as(C.c_void_p), reg.size) == -5
    eng0.close()
    # the engine refuses a register checkpoint under the plain name before anything reaches the device
    with pytest.raises(ValueError, match="_reg"):
        Engine(plain, precision="fp32", max_pairs=1).load_state_dict(sd)


def test_register_counts_through_the_engine():
    cfg = dataclasses.replace(config.vit_config(REG, 56), dim=128, heads=2, depth=1, layer=0, native_grid=4, registers=16)
    sd = weights.synthetic_state_dict(cfg, 3)
    frames = np.random.default_rng(0).integers(0, 256, size=(2, 56, 56, 3), dtype=np.uint8)
    eng = Engine(cfg, config.ServoParams(dino_input_size=56, use_feature_binning=False), precision="fp32",
                  max_pairs=1).load_state_dict(sd)
    got = eng.forward_tokens(frames).cpu()
    ref = rr.tokens(cfg, sd, frames)
    assert got.shape == ref.shape == (2, 1 + 16 + 16, 128)
    assert _rel_max(got, ref) <= 2e-5
    eng.close()
