"""Attention maps and CLS attention rollout of the fervit models.

The reference builds its encoders from nn.MultiheadAttention (`image_vit.py:101`,
`latent_vit.py:24`) and timm Attention (`hybrid_latent_vit.py:227-233`), where a user reads the
attention weights with `need_weights=True` or a forward hook. The fused layer functions here go
from qkv straight to the attention output, so this module taps qkv (fervit.layers.ATTN_TAP) and
lets fer_attention_probs produce the weights: head-averaged and row-selected inside the kernel,
the per-head [B, H, N, N] tensor is only written when asked for.

    maps = attention_maps(model, x)              # [L, B, N, N], mean over heads
    r    = attention_rollout(model, x)           # [B, N], CLS row of the rollout
    sal  = cls_saliency(model, x)                # [B, gh, gw] (patch models) / [B, tokens] (w+ models)
    t    = final_tokens(model, x)                # [B, N, D], what the head's LayerNorm reads
    cls_sim, tok_sim = token_similarity(model, x)  # [B, N-1], [B, N-1, N-1]

Maps are an eval / no-grad feature: a tapped forward that records gradients, has attention
dropout on or runs under graph capture raises RuntimeError. The tap sits in the layer functions,
so every model built from them (ImageViT, LatentViT, LatentViTv2, HybridLatentViT with or
without adapters, ExpressionAwareViT) is covered by the same code.

The reference's `eval/evaluate_model.py:231-296` (visualize_attention) re-runs the model's parts by hand to
reach the encoder output, then takes the cosine similarity of the final CLS token with every other token
and of those tokens with each other. The fused models go from tokens straight to logits (HeadFn), so
fervit.layers.TOKEN_TAP hands the final tokens out, under the same eval / no-grad / no-capture rule, and
fer_token_cosine computes both similarities in one launch.
"""
from __future__ import annotations

import contextlib
import math
from typing import Iterable, List, Optional

import torch

from . import layers as _layers
from . import ops


@contextlib.contextmanager
def capture_attention(average_heads: bool = True, queries: str = "all", layers: Optional[Iterable[int]] = None):
    """Collect one fp32 tensor per transformer layer, in forward order, from every forward run
    inside the block: [B, nq, N] (mean over heads) or [B, H, nq, N]; queries="all" keeps every
    query row (nq = N), "cls" only row 0 (nq = 1). `layers`: optional set of layer indices
    (position in forward order) to keep. Yields the list that fills up. The previous tap is
    restored on exit, also when the block raises."""
    if queries not in ("all", "cls"):
        raise ValueError('capture_attention: queries must be "all" or "cls"')
    keep = None if layers is None else {int(i) for i in layers}
    maps: List[torch.Tensor] = []
    seen = [0]

    def tap(qkv, cfg):
        i = seen[0]
        seen[0] += 1
        if keep is not None and i not in keep:
            return
        dh = qkv.shape[1] // (3 * cfg.H)
        maps.append(ops.attention_probs(qkv, cfg.B, cfg.N, cfg.H, dh, average_heads=average_heads,
                                        q_start=0, q_count=1 if queries == "cls" else None))

    prev = _layers.ATTN_TAP
    _layers.ATTN_TAP = tap
    try:
        yield maps
    finally:
        _layers.ATTN_TAP = prev


def attention_maps(model, x, average_heads: bool = True, queries: str = "all", layers=None) -> torch.Tensor:
    """Attention weights of every transformer layer for one eval forward of `model` on `x`:
    [L, B, nq, N], or [L, B, H, nq, N] with average_heads=False. Runs model.eval() under
    torch.no_grad() and restores the model's previous train / eval mode."""
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad(), capture_attention(average_heads, queries, layers=layers) as maps:
            model(x)
    finally:
        model.train(was_training)
    if not maps:
        raise RuntimeError("fervit: the model ran no fused attention layer (or `layers` kept none)")
    return torch.stack(maps)


def attention_rollout(model, x, residual: float = 0.5) -> torch.Tensor:
    """[B, N]: the CLS row of the attention rollout (Abnar & Zuidema 2020) over the model's layers,
    from the head-averaged maps (definition: rollout_reference)."""
    return ops.attention_rollout_cls(attention_maps(model, x), residual)


def cls_saliency(model, x, residual: float = 0.5) -> torch.Tensor:
    """How much the CLS token draws on each input token: the rollout without its CLS column,
    renormalised to sum 1. Image input [B, C, H, W]: [B, gh, gw] over the patch grid; w+ latent
    input [B, L, D]: [B, tokens] (18, or 36 behind a `concat` decomposer)."""
    r = attention_rollout(model, x, residual)[:, 1:]
    r = r / r.sum(dim=1, keepdim=True)
    if x.dim() == 4:
        tokens = r.shape[1]
        p = getattr(model, "patch_size", None)
        if p and (x.shape[2] // p) * (x.shape[3] // p) == tokens:
            gh, gw = x.shape[2] // p, x.shape[3] // p
        else:
            gh = gw = math.isqrt(tokens)
            if gh * gw != tokens:
                return r
        return r.reshape(r.shape[0], gh, gw)
    return r


def final_tokens(model, x) -> torch.Tensor:
    """[B, N, D]: the encoder output the model's head reads (row 0 of each batch element is the CLS token),
    in the model's compute dtype, from one eval forward under torch.no_grad(). The model's train / eval
    mode and the previous tap are restored."""
    got: List[torch.Tensor] = []

    def tap(t, cfg):
        got.append(t.view(cfg.B, cfg.N, t.shape[1]))

    was_training = model.training
    prev = _layers.TOKEN_TAP
    model.eval()
    _layers.TOKEN_TAP = tap
    try:
        with torch.no_grad():
            model(x)
    finally:
        _layers.TOKEN_TAP = prev
        model.train(was_training)
    if len(got) != 1:
        raise RuntimeError(f"fervit: the model ran {len(got)} fused heads (HeadFn), expected 1")
    return got[0]


def token_similarity(model, x, eps: float = 1e-8):
    """(cls_sim [B, N-1], tok_sim [B, N-1, N-1]), fp32: cosine similarity of the final CLS token with every
    other final token, and of those tokens with each other (torch.cosine_similarity's definition)."""
    return ops.token_cosine(final_tokens(model, x), eps)


def rollout_reference(maps: torch.Tensor, residual: float = 0.5) -> torch.Tensor:
    """The definition fer_attention_rollout_cls is tested against, in fp64 torch: with
    A'_l = residual * I + (1 - residual) * maps[l], row 0 of the full product A'_L ... A'_1.
    maps [L, B, N, N] -> [B, N] (float64, on maps' device)."""
    if maps.dim() != 4 or maps.shape[2] != maps.shape[3]:
        raise ValueError("rollout_reference: maps must be [L, B, N, N]")
    if not 0.0 <= float(residual) < 1.0:
        raise ValueError("rollout_reference: residual must be in [0, 1)")
    A = maps.double()
    L, B, N, _ = A.shape
    eye = torch.eye(N, dtype=torch.float64, device=A.device)
    R = eye.expand(B, N, N)
    for l in range(L):
        R = (residual * eye + (1.0 - residual) * A[l]) @ R
    return R[:, 0, :].contiguous()
