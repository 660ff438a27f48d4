"""Autograd functions of the LatentCNN baseline (reference `models_fer_vit/latent_cnn.py`), on the
same rules as layers.py: each forward / backward is a fixed sequence of libfervit launches (ops.py),
parameter gradients go straight into the model's flat gradient buffer (`_targets` / `_finish`),
dropout seeds come from `next_seed()` and masks are regenerated in the backward.

Activations are token-major [M = B*L][C] in the compute dtype, so the reference's `x.transpose(1, 2)`
costs nothing. BatchNorm's running statistics stay ordinary torch buffers of the nn.BatchNorm1d
modules (outside the flat store); the kernels update them in place on the device.

  ConvBNFn     [Conv1d(k=3) | Linear] -> BatchNorm1d -> (+ residual) -> ReLU -> Dropout
               (`latent_cnn.py:28-38` LatentConv1D, `:116-119` classifier, `:282-294` Light encoder)
  ResBlockFn   LatentResBlock1D (`latent_cnn.py:55-63`): both conv + BN stages, the gradient arriving
               over the skip connection added inside the first stage's im2col adjoint
  SeqMeanFn    AdaptiveAvgPool1d(1) + Flatten (`latent_cnn.py:157,115`)
  LogitsFn     the final Linear(D, num_classes) (`latent_cnn.py:120`)
  MlpLogitsFn  Linear -> ReLU -> Dropout -> Linear(., num_classes) (`latent_cnn.py:301-304`)
  ProjLNFn     Linear -> LayerNorm -> ReLU -> Dropout, LatentCNNDeep's input_proj (`latent_cnn.py:183-188`)
  AttnPoolFn   Conv1d(C, 1, 1) -> Softmax over the sequence -> weighted sum (`latent_cnn.py:207-211,256-257`)
  Conv2dBNFn   LatentCNN2D's stages (`latent_cnn.py:351-369`) on pixel-major rows [B*H*W][C]:
               Conv2d(3x3, padding 1) -> BatchNorm2d -> ReLU -> (MaxPool2d((2, 2))) -> Dropout2d; the convolution
               is im2col + GEMM, or the direct first-layer kernel when Cin = 1
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from . import ops
from .layers import _deferred_reductions, _dgrad, _finish, _targets, _weight, _wgrad
from .runtime import FlatParams, next_seed


@dataclass
class CnnCfg:
    B: int
    L: int
    k3: bool = True        # Conv1d(k=3, padding=1) (im2col + GEMM) or a plain Linear
    relu: bool = True
    dropout: float = 0.0   # applied after the ReLU; 0 outside training
    save: bool = True


@dataclass
class BNState:
    """Buffers and hyper-parameters of one nn.BatchNorm1d, read at call time."""
    running_mean: Optional[torch.Tensor]
    running_var: Optional[torch.Tensor]
    num_batches_tracked: Optional[torch.Tensor]
    momentum: float
    eps: float
    train: bool


def bn_state(bn: torch.nn.BatchNorm1d) -> BNState:
    if bn.momentum is None:
        raise NotImplementedError("fervit: BatchNorm1d(momentum=None) (cumulative moving average) has no kernel")
    if not bn.affine:
        raise NotImplementedError("fervit: BatchNorm1d(affine=False) has no kernel")
    train = bn.training or bn.running_mean is None
    return BNState(bn.running_mean, bn.running_var, bn.num_batches_tracked, float(bn.momentum), float(bn.eps), train)


def _stage_fwd(x, res, cfg: CnnCfg, flat: FlatParams, bn: BNState, w, b, gam, beta):
    """One conv / linear + BatchNorm stage. Returns (y, state for _stage_bwd)."""
    dt = x.dtype
    if cfg.k3:
        a = ops.conv1d_cols(x, cfg.B, cfg.L)
        Wm = _weight(flat, w, dt).reshape(w.shape[0], -1)
    else:
        a = x
        Wm = _weight(flat, w, dt)
    h = ops.linear_fwd(a, Wm, None if b is None else b.data)
    seed = next_seed() if cfg.dropout > 0 else 0
    y, mean, rstd = ops.batchnorm_fwd(h, gam.data, beta.data, bn.running_mean, bn.running_var,
                                      bn.num_batches_tracked, bn.train, bn.momentum, bn.eps, res=res, relu=cfg.relu,
                                      dropout=cfg.dropout, seed=seed)
    return y, (a, h, mean, rstd, seed, bn.train)


def _stage_bwd(dy, state, res, cfg: CnnCfg, flat: FlatParams, w, b, gam, beta, G, acc, want_dx=True,
               want_dres=False, dx_add=None):
    """Backward of _stage_fwd. G = gradient targets of (w, b, gamma, beta) (None: not wanted).
    Returns (dx, dres); dx_add (k3 only) is added to dx inside the im2col adjoint."""
    a, h, mean, rstd, seed, train = state
    gw, gb, ggam, gbeta = G
    dres = torch.empty_like(dy) if want_dres else None
    dh, dres = ops.batchnorm_bwd(dy, h, mean, rstd, gam.data, beta.data, train, res=res, relu=cfg.relu,
                                 dropout=cfg.dropout, seed=seed, dres=dres, dgamma=ggam, dbeta=gbeta, accumulate=acc)
    if gb is not None:
        ops.colsum(dh, gb, accumulate=acc)
    if gw is not None:
        _wgrad(dh, a, gw.view(gw.shape[0], -1), accumulate=acc)
    dx = None
    if want_dx:
        if cfg.k3:
            # conv weights are 3-D: no transposed shadow in the flat store, the dgrad reads W as an MN operand
            da = ops.linear_dgrad(dh, _weight(flat, w, dh.dtype).reshape(w.shape[0], -1))
            dx = ops.conv1d_cols_bwd(da, cfg.B, cfg.L, res=dx_add)
        else:
            dx = _dgrad(flat, dh, w, dh.dtype)
    return dx, dres


class ConvBNFn(torch.autograd.Function):
    # params: w ([Cout,Cin,3] or [Cout,Cin]), b (or None), bn gamma, bn beta
    @staticmethod
    def forward(ctx, x, res, cfg: CnnCfg, flat: FlatParams, bn: BNState, *P):
        y, state = _stage_fwd(x, res, cfg, flat, bn, *P)
        if cfg.save:
            ctx.cfg, ctx.flat, ctx.P = cfg, flat, P
            ctx.saved = (state, res)
        return y

    @staticmethod
    @_deferred_reductions
    def backward(ctx, dy):
        cfg, flat, P = ctx.cfg, ctx.flat, ctx.P
        state, res = ctx.saved
        needs = ctx.needs_input_grad[5:]
        G, acc = _targets(flat, P, needs)
        dx, dres = _stage_bwd(dy.contiguous(), state, res, cfg, flat, *P, G, acc, want_dx=ctx.needs_input_grad[0],
                              want_dres=res is not None and ctx.needs_input_grad[1])
        _finish(flat, P, needs)
        ctx.saved = None
        return (dx, dres, None, None, None) + (None,) * len(P)


class ResBlockFn(torch.autograd.Function):
    # params: conv1_w, bn1 gamma, bn1 beta, conv2_w, bn2 gamma, bn2 beta
    @staticmethod
    def forward(ctx, x, cfg: CnnCfg, flat: FlatParams, bn1: BNState, bn2: BNState, *P):
        w1, g1, b1, w2, g2, b2 = P
        cfg2 = CnnCfg(cfg.B, cfg.L, True, True, 0.0, cfg.save)
        o1, s1 = _stage_fwd(x, None, cfg, flat, bn1, w1, None, g1, b1)
        o2, s2 = _stage_fwd(o1, x, cfg2, flat, bn2, w2, None, g2, b2)
        if cfg.save:
            ctx.cfg, ctx.cfg2, ctx.flat, ctx.P = cfg, cfg2, flat, P
            ctx.saved = (x, s1, s2)
        return o2

    @staticmethod
    @_deferred_reductions
    def backward(ctx, dy):
        cfg, cfg2, flat, P = ctx.cfg, ctx.cfg2, ctx.flat, ctx.P
        w1, g1, b1, w2, g2, b2 = P
        x, s1, s2 = ctx.saved
        needs = ctx.needs_input_grad[5:]
        G, acc = _targets(flat, P, needs)
        want_dx = ctx.needs_input_grad[0]
        d1, dskip = _stage_bwd(dy.contiguous(), s2, x, cfg2, flat, w2, None, g2, b2, (G[3], None, G[4], G[5]), acc,
                               want_dres=want_dx)
        dx, _ = _stage_bwd(d1, s1, None, cfg, flat, w1, None, g1, b1, (G[0], None, G[1], G[2]), acc, want_dx=want_dx,
                           dx_add=dskip)
        _finish(flat, P, needs)
        ctx.saved = None
        return (dx, None, None, None, None) + (None,) * len(P)


class SeqMeanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, B: int, L: int):
        ctx.BL = (B, L)
        return ops.seq_mean_fwd(x, B, L)

    @staticmethod
    def backward(ctx, dy):
        B, L = ctx.BL
        return ops.seq_mean_bwd(dy.contiguous(), B, L), None, None


class LogitsFn(torch.autograd.Function):
    # params: W [C,D], b [C]
    @staticmethod
    def forward(ctx, x, save: bool, flat: FlatParams, *P):
        W, b = P
        logits = ops.logits_fwd(x, W.data, b.data)
        if save:
            ctx.flat, ctx.P = flat, P
            ctx.saved = (x,)
        return logits

    @staticmethod
    @_deferred_reductions
    def backward(ctx, dlogits):
        flat, P = ctx.flat, ctx.P
        W, b = P
        (x,) = ctx.saved
        needs = ctx.needs_input_grad[3:]
        G, acc = _targets(flat, P, needs)
        dx = ops.logits_bwd(x, W.data, dlogits.contiguous().float(), dW=G[0], dbias=G[1], accumulate=acc,
                            want_dx=ctx.needs_input_grad[0])
        _finish(flat, P, needs)
        ctx.saved = None
        return (dx, None, None) + (None,) * len(P)


class MlpLogitsFn(torch.autograd.Function):
    # params: W1 [H,D], b1 [H], W2 [C,H], b2 [C]
    @staticmethod
    def forward(ctx, x, dropout: float, save: bool, flat: FlatParams, *P):
        W1, b1, W2, b2 = P
        dt = x.dtype
        H = W1.shape[0]
        seed = next_seed() if dropout > 0 else 0
        f = torch.empty(x.shape[0], H, dtype=dt, device=x.device) if save else None
        # f = ReLU'(pre) * keep / (1 - p): logits_bwd multiplies the hidden gradient by it
        g = ops.linear_fwd(x, _weight(flat, W1, dt), b1.data, pre=f, pre_gate=True, act="relu", dropout=dropout,
                           seed=seed, drop_ld=H)
        logits = ops.logits_fwd(g, W2.data, b2.data)
        if save:
            ctx.flat, ctx.P = flat, P
            ctx.saved = (x, f, g)
        return logits

    @staticmethod
    @_deferred_reductions
    def backward(ctx, dlogits):
        flat, P = ctx.flat, ctx.P
        W1, b1, W2, b2 = P
        x, f, g = ctx.saved
        needs = ctx.needs_input_grad[4:]
        G, acc = _targets(flat, P, needs)
        gW1, gb1, gW2, gb2 = G
        du = ops.logits_bwd(g, W2.data, dlogits.contiguous().float(), gate=f, dW=gW2, dbias=gb2, accumulate=acc)
        if gb1 is not None:
            ops.colsum(du, gb1, accumulate=acc)
        if gW1 is not None:
            _wgrad(du, x, gW1, accumulate=acc)
        dx = _dgrad(flat, du, W1, du.dtype) if ctx.needs_input_grad[0] else None
        _finish(flat, P, needs)
        ctx.saved = None
        return (dx, None, None, None) + (None,) * len(P)


class ProjLNFn(torch.autograd.Function):
    # params: W [H,D], b [H], LayerNorm gamma [H], beta [H]
    @staticmethod
    def forward(ctx, x, eps: float, dropout: float, save: bool, flat: FlatParams, *P):
        W, b, gam, beta = P
        dt = x.dtype
        h = ops.linear_fwd(x, _weight(flat, W, dt), None if b is None else b.data)
        mean = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        n = ops.layernorm_fwd(h, gam.data, beta.data, eps, mean=mean, rstd=rstd)
        seed = next_seed() if dropout > 0 else 0
        y = ops.relu_dropout_fwd(n, dropout=dropout, seed=seed)
        if save:
            ctx.flat, ctx.P, ctx.dropout, ctx.seed = flat, P, dropout, seed
            ctx.saved = (x, h, mean, rstd, n)
        return y

    @staticmethod
    @_deferred_reductions
    def backward(ctx, dy):
        flat, P = ctx.flat, ctx.P
        W, b, gam, beta = P
        x, h, mean, rstd, n = ctx.saved
        needs = ctx.needs_input_grad[5:]
        G, acc = _targets(flat, P, needs)
        gW, gb, ggam, gbeta = G
        dn = ops.relu_dropout_bwd(dy.contiguous(), n, dropout=ctx.dropout, seed=ctx.seed)
        dh = ops.layernorm_bwd(dn, h, mean, rstd, gam.data, dgamma=ggam, dbeta=gbeta, accumulate=acc)
        if gb is not None:
            ops.colsum(dh, gb, accumulate=acc)
        if gW is not None:
            _wgrad(dh, x, gW, accumulate=acc)
        dx = _dgrad(flat, dh, W, dh.dtype) if ctx.needs_input_grad[0] else None
        _finish(flat, P, needs)
        ctx.saved = None
        return (dx, None, None, None, None) + (None,) * len(P)


class AttnPoolFn(torch.autograd.Function):
    # params: attention Conv1d weight [1,C,1], bias [1] (both read as fp32 parameters)
    @staticmethod
    def forward(ctx, x, B: int, L: int, save: bool, flat: FlatParams, *P):
        w, b = P
        y, probs = ops.attnpool_fwd(x, w.data, None if b is None else b.data, B, L, want_probs=save)
        if save:
            ctx.flat, ctx.P, ctx.BL = flat, P, (B, L)
            ctx.saved = (x, probs)
        return y

    @staticmethod
    @_deferred_reductions
    def backward(ctx, dy):
        flat, P = ctx.flat, ctx.P
        w, b = P
        B, L = ctx.BL
        x, probs = ctx.saved
        needs = ctx.needs_input_grad[5:]
        G, acc = _targets(flat, P, needs)
        dx = ops.attnpool_bwd(dy.contiguous(), x, w.data, probs, B, L, dw=G[0], dbias=G[1], accumulate=acc,
                              want_dx=ctx.needs_input_grad[0])
        _finish(flat, P, needs)
        ctx.saved = None
        return (dx, None, None, None, None) + (None,) * len(P)


# ---------------------------------------------------------------- LatentCNN2D
# The im2col matrix of a 3x3 convolution is nine times its input (B*9216 x 576 bf16 = 680 MB for
# Conv2d(64, 128) at batch 64). It is built per group of whole samples of at most this many bytes (fer_gemm
# takes operands below 2 GiB), consumed by the GEMM and dropped; the backward rebuilds it from the saved
# input for the weight gradient instead of keeping it. The groups depend on the shape alone.
COLS_CHUNK_BYTES = 1 << 30


@dataclass
class Cnn2dCfg:
    B: int
    H: int
    W: int
    pool: bool = False     # MaxPool2d((2, 2)) behind the ReLU
    dropout: float = 0.0   # Dropout2d (per sample and channel), behind the pool; 0 outside training
    save: bool = True


def _sample_groups(B: int, rows_per_sample: int, row_bytes: int):
    """[(first sample, samples)] with rows_per_sample * row_bytes * samples <= COLS_CHUNK_BYTES (at least 1)."""
    nb = max(1, min(B, COLS_CHUNK_BYTES // max(1, rows_per_sample * row_bytes)))
    return [(b0, min(nb, B - b0)) for b0 in range(0, B, nb)]


class Conv2dBNFn(torch.autograd.Function):
    # params: conv w [Cout,Cin,3,3], conv b (or None), bn gamma, bn beta. x: [B*H*W, Cin], or for Cin = 1 the
    # image itself, any contiguous shape with B*H*W elements
    @staticmethod
    def forward(ctx, x, cfg: Cnn2dCfg, flat: FlatParams, bn: BNState, *P):
        w, b, gam, beta = P
        B, H, W = cfg.B, cfg.H, cfg.W
        dt = x.dtype
        Cout, Cin = w.shape[0], w.shape[1]
        bias = None if b is None else b.data
        if Cin == 1:
            h = ops.conv2d_c1_fwd(x, w.data, bias, B, H, W)
        else:
            Wm = _weight(flat, w, dt).reshape(Cout, -1)
            h = torch.empty(B * H * W, Cout, dtype=dt, device=x.device)
            for b0, nb in _sample_groups(B, H * W, 9 * Cin * x.element_size()):
                r0, r1 = b0 * H * W, (b0 + nb) * H * W
                ops.linear_fwd(ops.conv2d_cols(x[r0:r1], nb, H, W), Wm, bias, out=h[r0:r1])
        r, mean, rstd = ops.batchnorm_fwd(h, gam.data, beta.data, bn.running_mean, bn.running_var,
                                          bn.num_batches_tracked, bn.train, bn.momentum, bn.eps, relu=True)
        tail = cfg.pool or cfg.dropout > 0
        seed = next_seed() if cfg.dropout > 0 else 0
        y = ops.pool2_chdrop_fwd(r, B, H, W, cfg.pool, dropout=cfg.dropout, seed=seed) if tail else r
        if cfg.save:
            ctx.cfg, ctx.flat, ctx.P = cfg, flat, P
            ctx.saved = (x, h, mean, rstd, r if cfg.pool else None, seed, bn.train, tail)
        return y

    @staticmethod
    @_deferred_reductions
    def backward(ctx, dy):
        cfg, flat, P = ctx.cfg, ctx.flat, ctx.P
        w, b, gam, beta = P
        x, h, mean, rstd, r, seed, train, tail = ctx.saved
        B, H, W = cfg.B, cfg.H, cfg.W
        Cout, Cin = w.shape[0], w.shape[1]
        needs = ctx.needs_input_grad[4:]
        G, acc = _targets(flat, P, needs)
        gw, gb, ggam, gbeta = G
        want_dx = ctx.needs_input_grad[0]
        dy = dy.contiguous()
        if tail:
            # pool = 0 reads no x: the keep bits alone
            dy = ops.pool2_chdrop_bwd(dy, r if cfg.pool else h, B, H, W, cfg.pool, dropout=cfg.dropout, seed=seed)
        dh, _ = ops.batchnorm_bwd(dy, h, mean, rstd, gam.data, beta.data, train, relu=True, dgamma=ggam, dbeta=gbeta,
                                  accumulate=acc)
        if gb is not None:
            ops.colsum(dh, gb, accumulate=acc)
        dx = None
        if Cin == 1:
            dx = ops.conv2d_c1_bwd(dh, x, w.data, B, H, W, dw=gw, accumulate=acc, want_dx=want_dx)
        elif gw is not None or want_dx:
            Wm = _weight(flat, w, dh.dtype).reshape(Cout, -1)
            if want_dx:
                dx = torch.empty_like(x)
            for i, (b0, nb) in enumerate(_sample_groups(B, H * W, 9 * Cin * x.element_size())):
                r0, r1 = b0 * H * W, (b0 + nb) * H * W
                if gw is not None:
                    # K = pixels: the split count must not hang on the shared workspace's size (ops.gemm ws_exact)
                    _wgrad(dh[r0:r1], ops.conv2d_cols(x[r0:r1], nb, H, W), gw.view(Cout, -1), accumulate=acc or i > 0,
                           ws_exact=True)
                if want_dx:
                    # conv weights are 4-D: no transposed shadow in the flat store, the dgrad reads W as an MN operand
                    ops.conv2d_cols_bwd(ops.linear_dgrad(dh[r0:r1], Wm), nb, H, W, out=dx[r0:r1])
        _finish(flat, P, needs)
        ctx.saved = None
        return (dx, None, None, None) + (None,) * len(P)
