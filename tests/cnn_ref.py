"""Reference arithmetic for the LatentCNN operators and models, restated in plain torch from the
formulas (test infrastructure; runs on the CPU in float64 or float32).

Operators (token-major [M = B*L][C], as csrc/convbn.hip):
  conv1d_cols / conv1d_cols_bwd   im2col of nn.Conv1d(k=3, padding=1) in (cin, k) column order and its
                                  adjoint (reference `models_fer_vit/latent_cnn.py:22-23,49,51,282-292`)
  batchnorm / batchnorm_bwd       nn.BatchNorm1d (`:24,50,52,117,283-293`) with the fused
                                  (+ residual) -> ReLU -> dropout epilogue (`:33-38,57-62`)
  seq_mean / logits               AdaptiveAvgPool1d(1) + Flatten (`:109,157`), the final Linear (`:120,304`)
Models: `forward(kind, sd, x, train)` for 'standard' (`:138-161`) and 'light' (`:321-330`) from a
state dict, differentiable by torch autograd; `rnd` rounds where the native bf16 path stores bf16.
"""
from __future__ import annotations

import zlib
from typing import Callable, Dict, Optional

import numpy as np
import torch

from detparams import det_tensor


# ------------------------------------------------------------------ deterministic state
def det_state(shapes, seed: int = 0) -> Dict[str, torch.Tensor]:
    """tests/golden/detparams.py values keyed by state_dict name, with BatchNorm entries (found by their
    `.running_var` sibling) moved to usable ranges: weight 1 + 0.1 n, bias 0.02 n, running_mean 0.1 n,
    running_var 0.5 + 0.5 |n|, num_batches_tracked 0 (int64)."""
    shapes = [(k, tuple(s)) for k, s in shapes]
    bns = {k[: -len("running_var")] for k, _ in shapes if k.endswith(".running_var")}
    out = {}
    for k, s in shapes:
        pre, leaf = k[: k.rfind(".") + 1], k[k.rfind(".") + 1:]
        if pre in bns and leaf == "num_batches_tracked":
            out[k] = torch.zeros(s, dtype=torch.long)
            continue
        t = det_tensor(k, s, seed).float()
        if pre in bns:
            n = t / 0.02  # det_tensor draws 0.02 * n for these 1-D keys
            t = {"weight": 1.0 + 0.1 * n, "bias": 0.02 * n, "running_mean": 0.1 * n,
                 "running_var": 0.5 + 0.5 * n.abs()}[leaf]
        out[k] = t.float()
    return out


def sample_idx(key: str, numel: int, k: int = 8) -> np.ndarray:
    g = np.random.default_rng(zlib.crc32(("idx:" + key).encode()))
    return np.sort(g.choice(numel, size=min(k, numel), replace=False))


# ------------------------------------------------------------------ operators
def conv1d_cols(x: torch.Tensor, B: int, L: int) -> torch.Tensor:
    """cols[b*L + l][c*3 + k] = x[b*L + l + k - 1][c] inside the sample, 0 outside."""
    C = x.shape[1]
    z = x.new_zeros(B, 1, C)
    xp = torch.cat([z, x.reshape(B, L, C), z], dim=1)
    return torch.stack([xp[:, k:k + L] for k in range(3)], dim=-1).reshape(B * L, 3 * C)


def conv1d_cols_bwd(dcols: torch.Tensor, B: int, L: int, res: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dx[b*L + l][c] = (res +) sum_k dcols[b*L + l - k + 1][c*3 + k] over 0 <= l - k + 1 < L."""
    C = dcols.shape[1] // 3
    d = dcols.reshape(B, L, C, 3)
    dx = d.new_zeros(B, L + 2, C)
    for k in range(3):
        dx[:, k:k + L] += d[..., k]
    dx = dx[:, 1:L + 1].reshape(B * L, C)
    return dx if res is None else dx + res


def batchnorm(x, gamma, beta, running_mean, running_var, train: bool, momentum: float = 0.1, eps: float = 1e-5,
              res=None, relu: bool = False, keep=None, scale: float = 1.0):
    """(y, mean, rstd, new running_mean, new running_var). train: biased batch variance for the
    normalisation, unbiased M/(M-1) for the running update."""
    M = x.shape[0]
    if train:
        mean = x.mean(0)
        var = ((x - mean) ** 2).mean(0)
        new_rm = new_rv = None
        if running_mean is not None:
            new_rm = (1 - momentum) * running_mean + momentum * mean.detach()
            new_rv = (1 - momentum) * running_var + momentum * var.detach() * (M / (M - 1))
    else:
        mean, var, new_rm, new_rv = running_mean, running_var, running_mean, running_var
    rstd = 1.0 / torch.sqrt(var + eps)
    y = (x - mean) * rstd * gamma + beta
    if res is not None:
        y = y + res
    if relu:
        y = torch.relu(y)
    if keep is not None:
        y = torch.where(keep, y * scale, torch.zeros_like(y))
    return y, mean, rstd, new_rm, new_rv


def batchnorm_bwd(dy, x, mean, rstd, gamma, beta, train: bool, res=None, relu: bool = False, keep=None,
                  scale: float = 1.0, gate=None):
    """(dx, dres, dgamma, dbeta) of batchnorm, from the formulas. gate (bool, optional): the ReLU gate
    to use instead of recomputing it (a lower-precision run that must not flip borderline elements)."""
    xh = (x - mean) * rstd
    g = dy
    if relu:
        if gate is None:
            v = xh * gamma + beta
            if res is not None:
                v = v + res
            gate = v > 0
        g = torch.where(gate, g, torch.zeros_like(g))
    if keep is not None:
        g = torch.where(keep, g * scale, torch.zeros_like(g))
    dbeta = g.sum(0)
    dgamma = (g * xh).sum(0)
    if train:
        M = x.shape[0]
        dx = gamma * rstd * (g - dbeta / M - xh * (dgamma / M))
    else:
        dx = gamma * rstd * g
    return dx, g, dgamma, dbeta


def seq_mean(x: torch.Tensor, B: int, L: int) -> torch.Tensor:
    return x.reshape(B, L, -1).mean(1)


def logits(x: torch.Tensor, W: torch.Tensor, b: Optional[torch.Tensor]) -> torch.Tensor:
    y = x @ W.t()
    return y if b is None else y + b


# ------------------------------------------------------------------ models
def bf16_round(t: torch.Tensor) -> torch.Tensor:
    """Round to bf16 and back, transparent to autograd (what storing an activation as bf16 does)."""
    return t + (t.detach().to(torch.bfloat16).to(t.dtype) - t.detach())


def forward(kind: str, sd: Dict[str, torch.Tensor], x: torch.Tensor, train: bool,
            rnd: Optional[Callable[[torch.Tensor], torch.Tensor]] = None):
    """Logits of create_latent_cnn(kind) with state `sd` on x (B, L, D), and the buffers after the call
    ({key: tensor}; train mode moves the running statistics and counts the batch). `rnd` (default:
    identity) is applied wherever the native bf16 path stores bf16: the input rows, the GEMM weight
    operands, every GEMM / BatchNorm / pool output. BatchNorm parameters, biases, statistics, the final
    Linear's weight and the logits stay in full precision, as they do natively."""
    rnd = rnd or (lambda t: t)
    B, L, D = x.shape
    buf = {}

    def stage(t, conv, bn, k3, res=None):
        w = rnd(sd[conv + ".weight"])
        a = conv1d_cols(t, B, L) if k3 else t
        h = a @ w.reshape(w.shape[0], -1).t()
        if conv + ".bias" in sd:
            h = h + sd[conv + ".bias"]
        h = rnd(h)
        y, _, _, rm, rv = batchnorm(h, sd[bn + ".weight"], sd[bn + ".bias"], sd[bn + ".running_mean"],
                                    sd[bn + ".running_var"], train, res=res, relu=True)
        buf[bn + ".running_mean"], buf[bn + ".running_var"] = rm, rv
        buf[bn + ".num_batches_tracked"] = sd[bn + ".num_batches_tracked"] + (1 if train else 0)
        return rnd(y)

    t = rnd(x.reshape(B * L, D))
    if kind == "standard":
        for i in range(4):
            t = stage(t, f"conv_layers.{i}.conv", f"conv_layers.{i}.bn", True)
        for j in range(2):
            o = stage(t, f"res_blocks.{j}.conv1", f"res_blocks.{j}.bn1", True)
            t = stage(o, f"res_blocks.{j}.conv2", f"res_blocks.{j}.bn2", True, res=t)
        pooled = rnd(seq_mean(t, B, L))
        h = stage(pooled, "classifier.1", "classifier.2", False)
        return logits(h, sd["classifier.5.weight"], sd["classifier.5.bias"]), buf
    if kind == "light":
        for ci in (0, 4, 8):
            t = stage(t, f"encoder.{ci}", f"encoder.{ci + 1}", True)
        pooled = rnd(seq_mean(t, B, L))
        g = rnd(torch.relu(pooled @ rnd(sd["classifier.1.weight"]).t() + sd["classifier.1.bias"]))
        return logits(g, sd["classifier.4.weight"], sd["classifier.4.bias"]), buf
    raise ValueError(kind)


def loss_fn(lg: torch.Tensor, labels: torch.Tensor, ls: float = 0.1) -> torch.Tensor:
    """CrossEntropyLoss(label_smoothing=ls), mean reduction, from its definition."""
    lp = lg - torch.logsumexp(lg, dim=1, keepdim=True)
    nll = -lp.gather(1, labels[:, None]).squeeze(1)
    smooth = -lp.mean(1)
    return ((1 - ls) * nll + ls * smooth).mean()


# ------------------------------------------------------------------ fixtures
def load_fixture(kind: str):
    import os

    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"latent_cnn_{kind}.npz"))


def fixture_inputs(kind: str, fx):
    """(state dict, x, labels) the fixture was recorded with, rebuilt from the key names alone."""
    from detparams import det_input, det_labels

    shapes = [(k, tuple(int(d) for d in s.split(",")) if s else ()) for k, s in zip(fx["sd_keys"], fx["sd_shapes"])]
    seed = int(fx["input_seed"])
    name = f"latent_cnn_{kind}"
    B, C = fx["logits"].shape
    return det_state(shapes), det_input(name, (B, 18, 512), seed), det_labels(name, B, seed=seed)


def check_grads(grads: Dict[str, torch.Tensor], fx, rel: float) -> None:
    """Every parameter's gradient against the fixture's {L2, sum, samples}: relative error `rel` of the
    L2 norm; the sum within rel * L2 * sqrt(numel) (Cauchy-Schwarz for an element-wise relative error);
    each sample within rel * (|ref| + L2 / sqrt(numel))."""
    assert sorted(grads) == sorted(fx["grad_keys"].tolist())
    top = float(fx["grad_l2"].max())
    for i, k in enumerate(fx["grad_keys"].tolist()):
        g = grads[k].detach().double().cpu().reshape(-1)
        n, l2 = g.numel(), float(fx["grad_l2"][i])
        if l2 < 1e-4 * top:
            # a bias in front of a train-mode BatchNorm: its gradient is exactly 0 in real arithmetic (the
            # batch mean absorbs it) and the recorded value is rounding noise; only its smallness is checked
            assert k.endswith(".bias") and g.norm().item() < 1e-4 * top, (k, g.norm().item())
            continue
        assert abs(g.norm().item() - l2) <= rel * l2, (k, "l2", g.norm().item(), l2)
        assert abs(g.sum().item() - float(fx["grad_sum"][i])) <= rel * l2 * n ** 0.5, (k, "sum")
        idx = fx["grad_idx"][i]
        idx = idx[idx >= 0]
        ref = torch.from_numpy(fx["grad_samples"][i][: len(idx)])
        err = (g[idx] - ref).abs()
        assert (err <= rel * (ref.abs() + l2 / n ** 0.5)).all(), (k, "samples", err.max().item())
