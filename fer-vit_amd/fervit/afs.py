"""Autograd function of the AFS style extractor (reference `afs/style_extractor.py`), on the rules of
cnn.py: a fixed sequence of libfervit launches (ops.py, csrc/grouped.hip), parameter gradients straight
into the model's flat gradient buffer (`_targets` / `_finish`).

G structurally identical blocks run as ONE launch per stage: their parameters sit at a constant stride
in the flat store (checked by `block_stride`), so block g's weight is `block 0's + g * stride` in the
fp32 master, its bf16 shadow and the gradient buffer alike. The [B, G, D] input is read in place and the
last stage writes [B, G, D] in place.

  forward   (down GEMM) -> per highway layer: one 3-set GEMM + one highway launch -> (up GEMM)
  backward  (up wgrad, up dgrad) -> per highway layer: highway bwd, 3-set wgrad, 3-set dgrad ->
            (down wgrad, down dgrad)

The same module may run several forwards before one backward (the AFS trainer calls h three times per
step): every call keeps its own saved tensors on its ctx, and the backward passes meet in `_targets`,
which returns accumulate = False for the first to arrive and True for the later ones.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence

import torch

from . import ops
from .layers import _deferred_reductions, _finish, _targets
from .runtime import FlatParams

PER_HIGHWAY = 8  # nonlinear.0.weight, .bias, nonlinear.1.weight, .bias, linear.weight, .bias, gate.weight, .bias


@dataclass
class HwStats:
    """BatchNorm buffers of one highway layer over the G blocks ([G, C] / [G] views) and its constants."""
    running_mean: torch.Tensor
    running_var: torch.Tensor
    num_batches_tracked: torch.Tensor
    momentum: float
    eps: float


@dataclass
class AfsCfg:
    G: int
    n_hw: int
    ends: bool     # Linear(in, mid) in front and Linear(mid, in) behind the highway layers (a StyleBlock)
    act: str       # 'lrelu' | 'relu'
    train: bool
    stride: int    # elements between consecutive blocks' parameters in the flat store
    save: bool = True


def block_stride(flat: FlatParams, blocks: Sequence[Sequence[torch.nn.Parameter]]) -> int:
    """The constant distance between the blocks' parameters in the flat store (0 for one block)."""
    if len(blocks) == 1:
        return 0
    offs = [[flat.offsets[id(p)] for p in ps] for ps in blocks]
    s = offs[1][0] - offs[0][0]
    for g, row in enumerate(offs):
        if len(row) != len(offs[0]) or any(o != o0 + g * s for o, o0 in zip(row, offs[0])):
            raise NotImplementedError("fervit: the style blocks' parameters are not at a constant stride in the flat "
                                      "parameter store; the grouped kernels have no pointer-table path")
    return s


def _gview(buf: torch.Tensor, flat: FlatParams, p: torch.nn.Parameter, cfg: AfsCfg) -> torch.Tensor:
    """[G, *p.shape] view of a flat buffer: block 0's parameter p and its G - 1 counterparts."""
    return torch.as_strided(buf, (cfg.G,) + tuple(p.shape), (cfg.stride,) + tuple(p.stride()), flat.offsets[id(p)])


class StyleBlocksFn(torch.autograd.Function):
    # x [B, G, K]; P: the G blocks' parameters, block after block, each in state_dict order
    @staticmethod
    def forward(ctx, x, cfg: AfsCfg, flat: FlatParams, stats: List[HwStats], *P):
        dt = x.dtype
        B = x.shape[0]
        wbuf = flat.bf16() if dt == torch.bfloat16 else flat.data
        W = lambda p: _gview(wbuf, flat, p, cfg)
        F = lambda p: _gview(flat.data, flat, p, cfg)
        xg = x.transpose(0, 1)
        k = 0
        h = xg
        if cfg.ends:
            h = ops.grouped_linear_fwd(xg, [W(P[0])], [F(P[1])])[0]
            k = 2
        saved = []
        for j in range(cfg.n_hw):
            nw, nb, bw, bb, lw, lb, gw, gb = P[k:k + PER_HIGHWAY]
            k += PER_HIGHWAY
            pn, pl, pg = ops.grouped_linear_fwd(h, [W(nw), W(lw), W(gw)], [F(nb), F(lb), F(gb)])
            st = stats[j]
            out = None
            if not cfg.ends and j == cfg.n_hw - 1:
                out = torch.empty(B, cfg.G, pn.shape[2], dtype=dt, device=x.device).transpose(0, 1)
            y, mean, rstd = ops.highway_fwd(pn, pl, pg, F(bw), F(bb), st.running_mean, st.running_var,
                                            st.num_batches_tracked, cfg.train, st.momentum, st.eps, cfg.act, out=out,
                                            want_stats=cfg.save)
            saved.append((h, pn, pl, pg, mean, rstd))
            h = y
        if cfg.ends:
            y = torch.empty(B, cfg.G, P[k].shape[0], dtype=dt, device=x.device)
            ops.grouped_linear_fwd(h, [W(P[k])], [F(P[k + 1])], outs=[y.transpose(0, 1)])
        else:
            y = h.transpose(0, 1)
        if cfg.save:
            ctx.cfg, ctx.flat, ctx.P = cfg, flat, P
            ctx.saved = (xg, saved, h)
        return y

    @staticmethod
    @_deferred_reductions
    def backward(ctx, dy):
        cfg, flat, P = ctx.cfg, ctx.flat, ctx.P
        xg, saved, h_last = ctx.saved
        G = cfg.G
        per = len(P) // G
        needs = ctx.needs_input_grad[4:]
        # frozen blocks are skipped inside the launches; within the live blocks a parameter is wanted in all or none
        live = [g for g in range(G) if any(needs[g * per:(g + 1) * per])]
        skip = sum(1 << g for g in range(G) if g not in live)
        want = []
        for k in range(per):
            v = {needs[g * per + k] for g in live}
            if len(v) > 1:
                raise NotImplementedError("fervit: freeze whole style blocks, or the same parameter in every block")
            want.append(bool(v and v.pop()))
        _, acc = _targets(flat, P, needs)
        dt = dy.dtype
        wbuf = flat.bf16() if dt == torch.bfloat16 else flat.data
        W = lambda p: _gview(wbuf, flat, p, cfg)
        F = lambda p: _gview(flat.data, flat, p, cfg)
        D = lambda k: _gview(flat.grad, flat, P[k], cfg) if want[k] else None
        want_dx = ctx.needs_input_grad[0]
        B = dy.shape[0]

        def wgrad(dys, x, ks_w, ks_b):
            dws, dbs = [D(k) for k in ks_w], [D(k) for k in ks_b]
            if any(t is not None for t in dws + dbs):
                ops.grouped_linear_wgrad(dys, x, dws, dbs, accumulate=acc, skip_mask=skip)

        dh = dy.contiguous().transpose(0, 1)
        k = per
        if cfg.ends:
            k -= 2
            wgrad([dh], h_last, [k], [k + 1])
            dh = ops.grouped_linear_dgrad([dh], [W(P[k])])
        dx = None
        for j in reversed(range(cfg.n_hw)):
            k -= PER_HIGHWAY
            nw, nb, bw, bb, lw, lb, gw, gb = P[k:k + PER_HIGHWAY]
            hin, pn, pl, pg, mean, rstd = saved[j]
            dps = ops.highway_bwd(dh, pn, pl, pg, mean, rstd, F(bw), F(bb), cfg.train, cfg.act, dgamma=D(k + 2),
                                  dbeta=D(k + 3), accumulate=acc, skip_mask=skip)
            wgrad(dps, hin, [k, k + 4, k + 6], [k + 1, k + 5, k + 7])
            first = j == 0 and not cfg.ends
            if not first or want_dx:
                out = None
                if first:
                    dx = torch.empty(B, G, hin.shape[2], dtype=dt, device=dy.device)
                    out = dx.transpose(0, 1)
                dh = ops.grouped_linear_dgrad(dps, [W(nw), W(lw), W(gw)], out=out)
        if cfg.ends:
            wgrad([dh], xg, [0], [1])
            if want_dx:
                dx = torch.empty(B, G, xg.shape[2], dtype=dt, device=dy.device)
                ops.grouped_linear_dgrad([dh], [W(P[0])], out=dx.transpose(0, 1))
        _finish(flat, P, needs)
        ctx.saved = None
        return (dx, None, None, None) + (None,) * len(P)
