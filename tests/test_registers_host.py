"""DINOv2 with register tokens (dinov2_vit{s,b,l}14_reg) on the host side: configuration geometry, state-dict layout and
its guard, the C ABI's validation of the register count (no GPU), and the CPU restatement of the register forward
(tests/registers_ref.py) against an independent implementation, HF transformers' Dinov2WithRegistersModel."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib, config, weights
from oracle import vit_ref

import registers_ref as rr

REG_MODELS = {"dinov2_vits14_reg": (384, 6, 12), "dinov2_vitb14_reg": (768, 12, 12), "dinov2_vitl14_reg": (1024, 16, 24)}


@pytest.mark.parametrize("name", sorted(REG_MODELS))
def test_register_model_geometry_at_308(name):
    cfg = config.vit_config(name, 308)
    plain = config.vit_config(name[:-len("_reg")], 308)
    dim, heads, depth = REG_MODELS[name]
    assert (cfg.dim, cfg.heads, cfg.depth, cfg.patch, cfg.native_grid) == (dim, heads, depth, 14, 37)
    assert cfg.registers == 4 and cfg.prefix == 5
    assert cfg.tokens == 484 and cfg.seq == 489
    assert plain.registers == 0 and plain.prefix == 1 and plain.seq == 485
    assert cfg.mean == plain.mean and cfg.std == plain.std                 # DINOv2's ImageNet normalisation
    assert cfg.flops_per_image() > plain.flops_per_image()                 # 489 rows through every block, not 485
    # the baseline table stays BASELINE.json's configs plus the reference default: no register model in it
    assert not [k for k, (m, _) in config.BASELINE_CONFIGS.items() if m.endswith("_reg")]


def test_vit_config_accepts_the_register_names_and_keeps_the_plain_ones():
    for name in REG_MODELS:
        assert config.vit_config(name, 518).registers == 4
    for name in ("dinov2_vits14", "dinov2_vitb14", "dinov2_vitl14", "dino_vits16", "vit_base_patch16_224"):
        assert config.vit_config(name, 224 if "16" in name else 518).registers == 0
    with pytest.raises(ValueError):
        config.vit_config("dinov2_vitg14_reg", 518)                        # SwiGLU MLP: not in this family


def test_state_dict_keys_of_a_register_model():
    cfg = config.vit_config("dinov2_vits14_reg", 308)
    want = weights.expected_tensors(cfg)
    plain = weights.expected_tensors(config.vit_config("dinov2_vits14", 308))
    assert set(want) - set(plain) == {"register_tokens"}
    assert want["register_tokens"] == (1, 4, 384)
    assert want["pos_embed"] == plain["pos_embed"] == (1, 1 + 37 * 37, 384)   # registers carry no position embedding
    for make in (weights.synthetic_state_dict, weights.trained_like_state_dict):
        sd = make(cfg, 3)
        weights.check_state_dict(cfg, sd)
        assert tuple(sd["register_tokens"].shape) == (1, 4, 384) and float(sd["register_tokens"].abs().max()) > 0
    # register_tokens is drawn last: the plain model's tensors are the same draws
    sd, sd0 = weights.synthetic_state_dict(cfg, 3), weights.synthetic_state_dict(config.vit_config("dinov2_vits14", 308), 3)
    assert all(torch.equal(sd[k], sd0[k]) for k in sd0)


def test_check_state_dict_refuses_a_register_checkpoint_under_the_plain_name():
    reg = config.vit_config("dinov2_vits14_reg", 308)
    plain = config.vit_config("dinov2_vits14", 308)
    sd = weights.synthetic_state_dict(reg, 0)
    with pytest.raises(ValueError, match="dinov2_vits14_reg"):
        weights.check_state_dict(plain, sd)
    bad = dict(sd, register_tokens=torch.zeros(1, 3, 384))
    with pytest.raises(ValueError, match="register_tokens"):
        weights.check_state_dict(reg, bad)
    missing = {k: v for k, v in sd.items() if k != "register_tokens"}
    with pytest.raises(KeyError):
        weights.check_state_dict(reg, missing)
    weights.check_state_dict(plain, missing)                               # the plain checkpoint still loads


def _cabi_config(cfg):
    c = _lib.VitvsConfig()
    c.abi_version = _lib.ABI_VERSION
    c.img_size, c.patch, c.stride, c.dim = cfg.img_size, cfg.patch, cfg.stride, cfg.dim
    c.heads, c.blocks, c.layerscale = cfg.heads, cfg.blocks_run, int(cfg.layerscale)
    for i in range(3):
        c.mean[i], c.std[i] = cfg.mean[i], cfg.std[i]
    c.ln_eps = cfg.ln_eps
    c.precision, c.binned, c.num_pairs, c.u_max, c.v_max, c.lambda_ = _lib.F32, 1, 24, 640, 480, 0.03
    c.max_pairs, c.max_rows = 1, 48
    return c


@pytest.mark.parametrize("count", [-1, 17])
def test_create_ex_rejects_a_bad_register_count_without_touching_a_gpu(count):
    if not __import__("os").path.isfile(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    c = _cabi_config(config.vit_config("dinov2_vits14_reg", 308))
    h = ctypes.c_void_p()
    assert lib.vitvs_create_ex(ctypes.byref(c), count, ctypes.byref(h)) < 0
    assert not h.value
    assert b"register" in lib.vitvs_last_error(None)
    assert lib.vitvs_register_tokens(None) == -1


def _frames(cfg, n=2, seed=0):
    return np.random.default_rng(seed).integers(0, 256, size=(n, cfg.img_size, cfg.img_size, 3), dtype=np.uint8)


def _check_against_hf(cfg, sd, frames):
    hs = rr.hf_hidden_states(cfg, sd, frames)
    mine = rr.tokens(cfg, sd, frames, return_all=True)
    assert len(hs) == len(mine) == cfg.blocks_run + 1
    for a, b in zip(hs, mine):
        assert a.shape == b.shape == (frames.shape[0], cfg.seq, cfg.dim)
        assert float((a - b).abs().max()) < 2e-5 * max(1.0, float(b.abs().max()))
    return mine


def test_restatement_matches_hf_dinov2_with_registers_tiny_layerscale():
    pytest.importorskip("transformers")
    base = config.vit_config("dinov2_vits14_reg", 56)
    cfg = dataclasses.replace(base, dim=128, depth=3, heads=2, layer=2, native_grid=base.grid)
    sd = weights.synthetic_state_dict(cfg, 2)
    frames = _frames(cfg)
    mine = _check_against_hf(cfg, sd, frames)
    # the embedding rows: cls + pos[0], the registers as they are, patches + pos[1 + t]
    x0 = mine[0]
    pos = vit_ref.resample_pos_embed(sd["pos_embed"], cfg.grid)[0]
    assert torch.equal(x0[:, 1:5], sd["register_tokens"].expand(2, -1, -1))
    assert torch.allclose(x0[:, 0], sd["cls_token"][0, 0] + pos[0])
    # and without registers the restatement is the oracle's forward
    plain = {k: v for k, v in sd.items() if k != "register_tokens"}
    cfg0 = dataclasses.replace(cfg, registers=0)
    assert torch.equal(rr.tokens(cfg0, plain, frames), vit_ref.block_tokens(plain, frames, patch=cfg.patch, stride=cfg.stride,
                                                                            heads=cfg.heads, layer=cfg.layer, mean=cfg.mean,
                                                                            std=cfg.std))


def test_restatement_matches_hf_dinov2_with_registers_at_vits14_width():
    """ViT-S/14 width (384, 6 heads, LayerScale gains != 1), the stored 37 x 37 grid resampled to 22 x 22, two blocks: 489 rows."""
    pytest.importorskip("transformers")
    cfg = dataclasses.replace(config.vit_config("dinov2_vits14_reg", 308), depth=2, layer=1)
    sd = weights.synthetic_state_dict(cfg, 6)
    frames = _frames(cfg, seed=5)
    _check_against_hf(cfg, sd, frames)


def test_restatement_slices_descriptors_facets_and_attention():
    base = config.vit_config("dinov2_vits14_reg", 56)
    cfg = dataclasses.replace(base, dim=128, depth=2, heads=2, layer=1, native_grid=base.grid)
    sd = weights.synthetic_state_dict(cfg, 4)
    frames = _frames(cfg, seed=3)
    toks = rr.tokens(cfg, sd, frames)
    assert torch.equal(rr.descriptors(cfg, sd, frames), toks[:, 5:])
    assert torch.equal(rr.descriptors(cfg, sd, frames, bin=True), vit_ref.log_bin(toks[:, 5:], cfg.grid))
    with_cls = rr.facet(cfg, sd, frames, "token", include_cls=True)
    assert with_cls.shape == (2, 1 + cfg.tokens, cfg.dim)
    assert torch.equal(with_cls[:, 0], toks[:, 0]) and torch.equal(with_cls[:, 1:], toks[:, 5:])
    q = rr.facet(cfg, sd, frames, "query")
    assert q.shape == (2, cfg.tokens, cfg.dim)
    a = rr.cls_attention(cfg, sd, frames)
    assert a.shape == (2, cfg.heads, cfg.tokens)
    assert float(a.sum(-1).max()) < 1.0                                   # the cls and register columns hold the rest
    s = rr.saliency_maps(cfg, sd, frames, head_idxs=(0, 1))
    assert float(s.min()) == 0.0 and float(s.max()) == 1.0
