"""Reference arithmetic of the AFS style extractor (reference `afs/style_extractor.py`), restated in plain
torch from the formulas (test infrastructure; CPU, float64 or float32).

Stages, grouped over G independent blocks ([G, rows, cols] operands, as csrc/grouped.hip):
  linear / linear_dgrad / linear_wgrad     y = x W^T + b and its adjoints
  highway / highway_bwd                    y = s n + (1 - s) l, n = act(BatchNorm(pn)), s = sigmoid(pg), with the
                                           hand-written backward the kernel implements
Model: `forward(sd, w, train, ...)` from a state dict, differentiable by torch autograd, returning the
buffers after the call; `train_step` is the trainer's three-call pattern the fixture records.
"""
from __future__ import annotations

import os
from typing import Callable, Dict, Optional

import numpy as np
import torch

from cnn_ref import det_state, sample_idx  # noqa: F401  (re-exported for the tests)
from detparams import det_input

B_FIX, G_FIX, D_FIX = 4, 18, 512


# ------------------------------------------------------------------ stages
def linear(x, W, b=None):
    """x [G, M, K], W [G, N, K], b [G, N] -> [G, M, N]."""
    y = torch.einsum("gmk,gnk->gmn", x, W)
    return y if b is None else y + b[:, None, :]


def linear_dgrad(dys, Ws):
    return sum(torch.einsum("gmn,gnk->gmk", dy, W) for dy, W in zip(dys, Ws))


def linear_wgrad(dy, x):
    """(dW [G, N, K], db [G, N])."""
    return torch.einsum("gmn,gmk->gnk", dy, x), dy.sum(1)


def act_fn(v, act: str):
    if act == "lrelu":
        return torch.where(v > 0, v, 0.2 * v)
    if act == "relu":
        return torch.where(v > 0, v, torch.zeros_like(v))
    raise ValueError(act)


def act_grad(v, act: str):
    return torch.where(v > 0, torch.ones_like(v), torch.full_like(v, 0.2 if act == "lrelu" else 0.0))


def highway(pn, pl, pg, gamma, beta, running_mean, running_var, train: bool, momentum=0.1, eps=1e-5, act="lrelu"):
    """pn, pl, pg [G, B, C]; gamma, beta, running_* [G, C]. Returns (y, mean, rstd, new running_mean, new
    running_var): train normalises by the biased batch variance and moves the running variance towards the
    unbiased one."""
    Bn = pn.shape[1]
    if train:
        mean = pn.mean(1)
        var = ((pn - mean[:, None]) ** 2).mean(1)
        new_rm = new_rv = None
        if running_mean is not None:
            new_rm = (1 - momentum) * running_mean + momentum * mean.detach()
            new_rv = (1 - momentum) * running_var + momentum * var.detach() * (Bn / (Bn - 1))
    else:
        mean, var, new_rm, new_rv = running_mean, running_var, running_mean, running_var
    rstd = 1.0 / torch.sqrt(var + eps)
    v = (pn - mean[:, None]) * rstd[:, None] * gamma[:, None] + beta[:, None]
    s = torch.sigmoid(pg)
    y = s * act_fn(v, act) + torch.sigmoid(-pg) * pl
    return y, mean, rstd, new_rm, new_rv


def highway_bwd(dy, pn, pl, pg, mean, rstd, gamma, beta, train: bool, act="lrelu"):
    """(dpn, dpl, dpg, dgamma, dbeta) from the formulas: dg = dy (n - l) s (1 - s), dl = dy (1 - s),
    dn = dy s through the activation and the BatchNorm adjoint."""
    Bn = pn.shape[1]
    xh = (pn - mean[:, None]) * rstd[:, None]
    v = xh * gamma[:, None] + beta[:, None]
    s, sc = torch.sigmoid(pg), torch.sigmoid(-pg)
    dpg = dy * (act_fn(v, act) - pl) * (s * sc)
    dpl = dy * sc
    dv = dy * s * act_grad(v, act)
    dbeta = dv.sum(1)
    dgamma = (dv * xh).sum(1)
    if train:
        dpn = (gamma * rstd)[:, None] * (dv - dbeta[:, None] / Bn - xh * (dgamma[:, None] / Bn))
    else:
        dpn = (gamma * rstd)[:, None] * dv
    return dpn, dpl, dpg, dgamma, dbeta


# ------------------------------------------------------------------ model
def _stack(sd, G, name):
    return torch.stack([sd[f"blocks.{g}.{name}"] for g in range(G)])


def forward(sd: Dict[str, torch.Tensor], w: torch.Tensor, train: bool, n_hw: int = 2, act: str = "lrelu",
            momentum: float = 0.1, eps: float = 1e-5, rnd: Optional[Callable] = None, buf: Optional[dict] = None):
    """h(w) for w [B, G, D] with state `sd` (keys of StyleExtractor.state_dict()); `buf` (a dict of the
    BatchNorm buffers, default: sd's) is read and, in train mode, replaced entry by entry with the
    updated statistics. `rnd` is applied wherever the native bf16 path stores bf16."""
    rnd = rnd or (lambda t: t)
    G = w.shape[1]
    buf = sd if buf is None else buf
    h = rnd(w).transpose(0, 1)
    h = rnd(linear(h, rnd(_stack(sd, G, "down.weight")), _stack(sd, G, "down.bias")))
    for j in range(n_hw):
        pre = f"highways.{j}."
        pn, pl, pg = (rnd(linear(h, rnd(_stack(sd, G, pre + n + ".weight")), _stack(sd, G, pre + n + ".bias")))
                      for n in ("nonlinear.0", "linear", "gate"))
        bn = pre + "nonlinear.1."
        y, _, _, rm, rv = highway(pn, pl, pg, _stack(sd, G, bn + "weight"), _stack(sd, G, bn + "bias"),
                                  _stack(buf, G, bn + "running_mean"), _stack(buf, G, bn + "running_var"), train,
                                  momentum, eps, act)
        if train:
            for g in range(G):
                k = f"blocks.{g}.{bn}"
                buf[k + "running_mean"], buf[k + "running_var"] = rm[g], rv[g]
                buf[k + "num_batches_tracked"] = buf[k + "num_batches_tracked"] + 1
        h = rnd(y)
    y = rnd(linear(h, rnd(_stack(sd, G, "up.weight")), _stack(sd, G, "up.bias")))
    return y.transpose(0, 1)


def probe(shape) -> torch.Tensor:
    """The fixed linear probe of w_new in the fixture's loss."""
    return det_input("afs_probe", tuple(shape)) / float(np.prod(shape))


def train_step(h: Callable, w_src, w_tgt):
    """The trainer's pattern: s = h(w_src), t = h(w_tgt), w_new = (w_src - s) + t, n = h(w_new);
    loss = l1(n, t.detach()) + <probe, w_new>. Returns (s, t, n, loss)."""
    s = h(w_src)
    t = h(w_tgt)
    w_new = (w_src - s) + t
    n = h(w_new)
    loss = (n - t.detach()).abs().mean() + (w_new * probe(w_new.shape).to(w_new)).sum()
    return s, t, n, loss


# ------------------------------------------------------------------ fixture
def load_fixture():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "afs_style_extractor.npz"))


def fixture_inputs(fx):
    """(state dict, w_src, w_tgt) the fixture was recorded with, rebuilt from the key names alone."""
    shapes = [(k, tuple(int(d) for d in s.split(",")) if s else ()) for k, s in zip(fx["sd_keys"], fx["sd_shapes"])]
    shape = tuple(fx["out_src"].shape)
    return det_state(shapes), det_input("afs_src", shape), det_input("afs_tgt", shape)
