"""CPU restatement of the forward of a ViT with register tokens (DINOv2 "_reg" checkpoints), built from the oracle's pieces
(oracle/vit_ref.py, oracle/servo_ref.py) plus the three things registers change:

  * token order  x = [cls + pos[0], reg_0 .. reg_{R-1}, patch_t + pos[1 + t]]: the registers are inserted AFTER the position
    embedding and carry none (DINOv2 prepare_tokens_with_masks; HF Dinov2WithRegistersEmbeddings.forward), and every block
    attends over all N = 1 + R + T rows;
  * descriptors and facets take the patch rows x[:, 1 + R:] (include_cls: [cls, patches], registers dropped);
  * the class token's attention is a softmax over all N keys, of which the patch columns are kept.

A helper module for tests/test_registers_host.py and tests/test_gpu_registers.py, not a test file itself.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import vit_ref


def _kw(cfg):
    return dict(patch=cfg.patch, stride=cfg.stride, heads=cfg.heads, layer=cfg.layer, mean=cfg.mean, std=cfg.std,
                eps=cfg.ln_eps)


@torch.no_grad()
def block_tokens(sd, frames_u8: np.ndarray, *, patch: int, stride: int, heads: int, layer: int, mean, std,
                 eps: float = 1e-6, return_all: bool = False):
    """Residual stream after ``blocks[layer]``: float32 [B, 1 + R + T, D] (R = 0 without ``register_tokens``)."""
    x = vit_ref.preprocess_u8(frames_u8, mean, std)
    x = F.conv2d(x, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=stride)
    b, d, gh, gw = x.shape
    assert gh == gw, "square grids only"
    x = x.flatten(2).transpose(1, 2)
    x = torch.cat((sd["cls_token"].expand(b, -1, -1), x), dim=1)
    x = x + vit_ref.resample_pos_embed(sd["pos_embed"], gh)
    if "register_tokens" in sd:
        x = torch.cat((x[:, :1], sd["register_tokens"].expand(b, -1, -1), x[:, 1:]), dim=1)
    stages = [x]
    for i in range(layer + 1):
        x = vit_ref.block(x, sd, i, heads, eps)
        stages.append(x)
    return stages if return_all else x


def prefix(sd) -> int:
    """P: rows in front of the patch tokens (cls + registers)."""
    return 1 + (int(sd["register_tokens"].shape[1]) if "register_tokens" in sd else 0)


def tokens(cfg, sd, frames_u8, return_all: bool = False):
    return block_tokens(sd, frames_u8, return_all=return_all, **_kw(cfg))


def descriptors(cfg, sd, frames_u8, bin: bool = False, toks=None) -> torch.Tensor:
    """The token facet's descriptors [B, T, D] (or [B, T, 9 D] binned): patch rows only."""
    x = (tokens(cfg, sd, frames_u8) if toks is None else toks)[:, prefix(sd):]
    return vit_ref.log_bin(x, int(math.sqrt(x.shape[1]))) if bin else x


def _qkv_of_layer(cfg, sd, frames_u8):
    stages = tokens(cfg, sd, frames_u8, return_all=True)
    x = stages[cfg.layer]                                    # input of blocks[layer]
    p = f"blocks.{cfg.layer}."
    y = F.layer_norm(x, (x.shape[-1],), sd[p + "norm1.weight"], sd[p + "norm1.bias"], cfg.ln_eps)
    b, n, c = y.shape
    qkv = F.linear(y, sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"]).reshape(b, n, 3, cfg.heads, c // cfg.heads)
    return stages[-1], qkv.permute(2, 0, 3, 1, 4)           # 3 x B x H x N x hd


@torch.no_grad()
def facet(cfg, sd, frames_u8, which: str, bin: bool = False, include_cls: bool = False) -> torch.Tensor:
    """extract_descriptors(facet, bin, include_cls) of a register model: [B, T, D], [B, 1 + T, D] or [B, T, 9 D]."""
    assert not (bin and include_cls)
    P = prefix(sd)
    if which == "token":
        f = tokens(cfg, sd, frames_u8)
    else:
        f = _qkv_of_layer(cfg, sd, frames_u8)[1][{"query": 0, "key": 1, "value": 2}[which]]   # B x H x N x hd
        f = f.permute(0, 2, 3, 1).flatten(start_dim=-2)      # B x N x (d x h): index d * H + h
    f = torch.cat((f[:, :1], f[:, P:]), dim=1) if include_cls else f[:, P:]
    return vit_ref.log_bin(f, int(math.sqrt(f.shape[1]))) if bin else f


@torch.no_grad()
def cls_attention(cfg, sd, frames_u8) -> torch.Tensor:
    """The class token's attention probabilities in ``blocks[layer]``, softmax over all N keys, patch columns: [B, H, T]."""
    qkv = _qkv_of_layer(cfg, sd, frames_u8)[1]
    q, k = qkv[0], qkv[1]
    attn = ((q @ k.transpose(-2, -1)) * (cfg.dim // cfg.heads) ** -0.5).softmax(dim=-1)
    return attn[:, :, 0, prefix(sd):]


def saliency_maps(cfg, sd, frames_u8, head_idxs=(0, 2, 4, 5)) -> torch.Tensor:
    m = cls_attention(cfg, sd, frames_u8)[:, list(head_idxs)].mean(dim=1)
    lo, hi = m.min(dim=1)[0], m.max(dim=1)[0]
    return (m - lo[:, None]) / (hi - lo)[:, None]


def hf_hidden_states(cfg, sd, frames_u8):
    """HF transformers Dinov2WithRegistersModel (built from a local config, no download) with these weights: its hidden states.
    It is handed the already-resampled position embedding, so it interpolates nothing and witnesses everything else."""
    import transformers
    hf_cfg = transformers.Dinov2WithRegistersConfig(
        hidden_size=cfg.dim, num_hidden_layers=cfg.blocks_run, num_attention_heads=cfg.heads, mlp_ratio=4,
        image_size=cfg.img_size, patch_size=cfg.patch, layer_norm_eps=cfg.ln_eps, hidden_act="gelu", qkv_bias=True,
        layerscale_value=1.0, use_swiglu_ffn=False, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
        drop_path_rate=0.0, num_register_tokens=cfg.registers)
    model = transformers.Dinov2WithRegistersModel(hf_cfg).eval()
    own = model.state_dict()
    m = {"embeddings.cls_token": sd["cls_token"], "embeddings.register_tokens": sd["register_tokens"],
         "embeddings.position_embeddings": vit_ref.resample_pos_embed(sd["pos_embed"], cfg.grid),
         "embeddings.patch_embeddings.projection.weight": sd["patch_embed.proj.weight"],
         "embeddings.patch_embeddings.projection.bias": sd["patch_embed.proj.bias"],
         "embeddings.mask_token": own["embeddings.mask_token"]}
    d = cfg.dim
    for i in range(cfg.blocks_run):
        s, t = f"blocks.{i}.", f"encoder.layer.{i}."
        qw, qb = sd[s + "attn.qkv.weight"], sd[s + "attn.qkv.bias"]
        for j, nm in enumerate(("query", "key", "value")):
            m[t + f"attention.attention.{nm}.weight"] = qw[j * d:(j + 1) * d]
            m[t + f"attention.attention.{nm}.bias"] = qb[j * d:(j + 1) * d]
        m[t + "attention.output.dense.weight"] = sd[s + "attn.proj.weight"]
        m[t + "attention.output.dense.bias"] = sd[s + "attn.proj.bias"]
        for a, b in (("norm1", "norm1"), ("norm2", "norm2")):
            m[t + f"{b}.weight"] = sd[s + f"{a}.weight"]
            m[t + f"{b}.bias"] = sd[s + f"{a}.bias"]
        m[t + "layer_scale1.lambda1"] = sd[s + "ls1.gamma"]
        m[t + "layer_scale2.lambda1"] = sd[s + "ls2.gamma"]
        for nm in ("fc1", "fc2"):
            m[t + f"mlp.{nm}.weight"] = sd[s + f"mlp.{nm}.weight"]
            m[t + f"mlp.{nm}.bias"] = sd[s + f"mlp.{nm}.bias"]
    missing, unexpected = model.load_state_dict(m, strict=False)
    assert not [k for k in missing if not k.startswith("layernorm.")], missing
    assert not unexpected, unexpected
    x = vit_ref.preprocess_u8(frames_u8, cfg.mean, cfg.std)
    with torch.no_grad():
        return model(pixel_values=x, output_hidden_states=True).hidden_states
