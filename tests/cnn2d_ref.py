"""Reference arithmetic for LatentCNN2D (reference `models_fer_vit/latent_cnn.py:333-409`), restated in
plain torch on top of tests/cnn_ref.py (test infrastructure; CPU, float64 or float32). Pixel-major rows
[M = B*H*W][C], as csrc/conv2d.hip.

  conv2d_cols / conv2d_cols_bwd   im2col of nn.Conv2d(3x3, padding 1) in (cin, kh, kw) column order and its
                                  adjoint (`:358,364`)
  conv2d_c1 / conv2d_c1_bwd       the first layer Conv2d(1, Cout, 3, padding 1) with bias (`:353`) and its
                                  hand-written backward (dw, dbias, dx)
  pool2_chdrop / pool2_chdrop_bwd MaxPool2d((2, 2)) then Dropout2d with an explicit [B, C] keep mask
                                  (`:356,361-362,367-368`); the argmax is the window's first maximum in (kh, kw)
                                  scan order under a strict >, PyTorch's rule
  forward_2d                      the model from a state dict, differentiable by torch autograd; `rnd` rounds
                                  where the native bf16 path stores bf16
"""
from __future__ import annotations

from typing import Callable, Dict, Optional

import torch

import cnn_ref as R

KIND = "2d"
# (conv, bn, pool?, index of the Dropout2d whose keep mask follows) of LatentCNN2D.features
STAGES = (("features.0", "features.1", False), ("features.4", "features.5", True), ("features.9", "features.10", True))


def fixture_inputs(fx):
    """(state dict, x, labels) the '2d' fixture was recorded with, rebuilt from the key names alone."""
    return R.fixture_inputs(KIND, fx)


# ------------------------------------------------------------------ operators
def _padded(x: torch.Tensor, B: int, H: int, W: int) -> torch.Tensor:
    """[B, H + 2, W + 2, C] with a zero border."""
    C = x.shape[1]
    xp = x.new_zeros(B, H + 2, W + 2, C)
    xp[:, 1:H + 1, 1:W + 1] = x.reshape(B, H, W, C)
    return xp


def conv2d_cols(x: torch.Tensor, B: int, H: int, W: int) -> torch.Tensor:
    """cols[(b*H + h)*W + w][c*9 + kh*3 + kw] = x[(b*H + h+kh-1)*W + (w+kw-1)][c] inside the image, else 0."""
    C = x.shape[1]
    xp = _padded(x, B, H, W)
    taps = [xp[:, kh:kh + H, kw:kw + W] for kh in range(3) for kw in range(3)]
    return torch.stack(taps, dim=-1).reshape(B * H * W, 9 * C)


def conv2d_cols_bwd(dcols: torch.Tensor, B: int, H: int, W: int) -> torch.Tensor:
    """dx[m][c] = sum over (kh, kw) in scan order of dcols[m - (kh-1)*W - (kw-1)][c*9 + kh*3 + kw] inside the image."""
    C = dcols.shape[1] // 9
    d = dcols.reshape(B, H, W, C, 9)
    dx = d.new_zeros(B, H + 2, W + 2, C)
    for k in range(9):
        kh, kw = divmod(k, 3)
        dx[:, kh:kh + H, kw:kw + W] += d[..., k]
    return dx[:, 1:H + 1, 1:W + 1].reshape(B * H * W, C)


def conv2d_c1(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], B: int, H: int, W: int) -> torch.Tensor:
    """y[m][co] = bias[co] + sum_k x9[m][k] w[co][k]: x with B*H*W elements, w [Cout, 1, 3, 3] (or [Cout, 9])."""
    y = conv2d_cols(x.reshape(-1, 1), B, H, W) @ w.reshape(w.shape[0], 9).t()
    return y if bias is None else y + bias


def conv2d_c1_bwd(dy: torch.Tensor, x: torch.Tensor, w: torch.Tensor, B: int, H: int, W: int):
    """(dw [Cout, 9], dbias [Cout], dx [B*H*W]) of conv2d_c1, from the formulas."""
    x9 = conv2d_cols(x.reshape(-1, 1), B, H, W)
    dw = dy.t() @ x9
    dx = conv2d_cols_bwd(dy @ w.reshape(w.shape[0], 9), B, H, W).reshape(-1)
    return dw, dy.sum(0), dx


def pool_argmax(x: torch.Tensor, B: int, H: int, W: int):
    """(max [B, Ho, Wo, C], position 0..3 of the first maximum in (kh, kw) scan order)."""
    C = x.shape[1]
    Ho, Wo = H // 2, W // 2
    win = x.reshape(B, H, W, C)[:, :2 * Ho, :2 * Wo].reshape(B, Ho, 2, Wo, 2, C).permute(0, 1, 3, 5, 2, 4)
    win = win.reshape(B, Ho, Wo, C, 4)
    best, pos = win[..., 0], torch.zeros(win.shape[:-1], dtype=torch.long)
    for q in range(1, 4):
        better = win[..., q] > best
        best = torch.where(better, win[..., q], best)
        pos = torch.where(better, torch.full_like(pos, q), pos)
    return best, pos


def pool2_chdrop(x: torch.Tensor, B: int, H: int, W: int, pool: bool, keep: Optional[torch.Tensor] = None,
                 scale: float = 1.0) -> torch.Tensor:
    """x [B*H*W, C] -> [B*Ho*Wo, C]; keep: bool [B, C] (None: no dropout)."""
    C = x.shape[1]
    if pool:
        best, pos = pool_argmax(x.detach(), B, H, W)
        Ho, Wo = H // 2, W // 2
        # gather (differentiable) the chosen pixel instead of returning `best`, so autograd follows the rule
        win = x.reshape(B, H, W, C)[:, :2 * Ho, :2 * Wo].reshape(B, Ho, 2, Wo, 2, C).permute(0, 1, 3, 5, 2, 4)
        y = win.reshape(B, Ho, Wo, C, 4).gather(-1, pos[..., None]).squeeze(-1)
    else:
        y = x.reshape(B, H, W, C)
    if keep is not None:
        y = torch.where(keep[:, None, None, :], y * scale, torch.zeros_like(y))
    return y.reshape(-1, C)


def pool2_chdrop_bwd(dy: torch.Tensor, x: torch.Tensor, B: int, H: int, W: int, pool: bool,
                     keep: Optional[torch.Tensor] = None, scale: float = 1.0) -> torch.Tensor:
    """dx [B*H*W, C]: dy * keep * scale at each window's argmax pixel, exactly 0 elsewhere."""
    C = x.shape[1]
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    g = dy.reshape(B, Ho, Wo, C)
    if keep is not None:
        g = torch.where(keep[:, None, None, :], g * scale, torch.zeros_like(g))
    if not pool:
        return g.reshape(-1, C)
    _, pos = pool_argmax(x, B, H, W)
    dx = dy.new_zeros(B, H, W, C)
    for q in range(4):
        kh, kw = divmod(q, 2)
        dx[:, kh:2 * Ho:2, kw:2 * Wo:2] = torch.where(pos == q, g, torch.zeros_like(g))
    return dx.reshape(-1, C)


# ------------------------------------------------------------------ model
def forward_2d(sd: Dict[str, torch.Tensor], x: torch.Tensor, train: bool, keeps=None,
               rnd: Optional[Callable[[torch.Tensor], torch.Tensor]] = None):
    """(logits, buffers after the call) of LatentCNN2D with state `sd` on x (B, H, W).
    keeps: None, or [(keep [B, C] bool, scale)] for the three Dropout2d sites and the classifier's Dropout
    (keep [B, 256]), in forward order; an entry may be None.
    `rnd` (default: identity) is applied wherever the native bf16 path stores bf16: the input image, the GEMM
    weight operands of the second and third convolution and of the classifier's first Linear, every
    convolution / BatchNorm / pool / mean output. The first convolution's weight, BatchNorm parameters, biases,
    statistics and the final Linear stay in full precision, as they do natively."""
    rnd = rnd or (lambda t: t)
    keeps = keeps or [None] * 4
    B, H, W = x.shape
    buf = {}

    def bn_relu(h, bn, keep=None):
        y, _, _, rm, rv = R.batchnorm(h, sd[bn + ".weight"], sd[bn + ".bias"], sd[bn + ".running_mean"],
                                      sd[bn + ".running_var"], train, relu=True,
                                      keep=None if keep is None else keep[0], scale=1.0 if keep is None else keep[1])
        buf[bn + ".running_mean"], buf[bn + ".running_var"] = rm, rv
        buf[bn + ".num_batches_tracked"] = sd[bn + ".num_batches_tracked"] + (1 if train else 0)
        return rnd(y)

    t = rnd(x.reshape(-1))
    for i, (conv, bn, pool) in enumerate(STAGES):
        w, b = sd[conv + ".weight"], sd[conv + ".bias"]
        if i == 0:
            h = conv2d_c1(t, w, b, B, H, W)
        else:
            h = conv2d_cols(t, B, H, W) @ rnd(w).reshape(w.shape[0], -1).t() + b
        r = bn_relu(rnd(h), bn)
        k = keeps[i]
        if pool or k is not None:
            r = rnd(pool2_chdrop(r, B, H, W, pool, None if k is None else k[0], 1.0 if k is None else k[1]))
        t = r
        if pool:
            H, W = H // 2, W // 2
    pooled = rnd(R.seq_mean(t, B, H * W))
    h = rnd(pooled @ rnd(sd["classifier.1.weight"]).t() + sd["classifier.1.bias"])
    h = bn_relu(h, "classifier.2", keeps[3])
    return R.logits(h, sd["classifier.5.weight"], sd["classifier.5.bias"]), buf


def pool_nonfirst(sd: Dict[str, torch.Tensor], x: torch.Tensor):
    """For the two MaxPool2d of a train-mode forward without dropout: the fraction of windows whose argmax is
    not the top-left pixel."""
    out = []
    B, H, W = x.shape
    t = x.reshape(-1)
    for i, (conv, bn, pool) in enumerate(STAGES):
        w, b = sd[conv + ".weight"], sd[conv + ".bias"]
        h = conv2d_c1(t, w, b, B, H, W) if i == 0 else conv2d_cols(t, B, H, W) @ w.reshape(w.shape[0], -1).t() + b
        r = R.batchnorm(h, sd[bn + ".weight"], sd[bn + ".bias"], None, None, True, relu=True)[0]
        if pool:
            out.append((pool_argmax(r, B, H, W)[1] != 0).double().mean().item())
            r = pool2_chdrop(r, B, H, W, True)
            H, W = H // 2, W // 2
        t = r
    return out
