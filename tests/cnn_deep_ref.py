"""Reference arithmetic for LatentCNNDeep (reference `models_fer_vit/latent_cnn.py:164-261`), restated in
plain torch on top of tests/cnn_ref.py (test infrastructure; CPU, float64 or float32).

  attnpool / attnpool_bwd   Conv1d(C, 1, 1) -> Softmax(dim=2) -> weighted sum over the sequence
                            (`:207-211, 256-257`) on token-major rows [B*L][C], and its hand-written backward
                            (the formulas of csrc/attnpool.hip)
  det_state_deep            cnn_ref.det_state with the LayerNorm entries (the fixture's `ln_prefixes`) moved
                            to weight 1 + 0.1 n, bias 0.02 n
  forward_deep              the model from a state dict, differentiable by torch autograd; `rnd` rounds where
                            the native bf16 path stores bf16
"""
from __future__ import annotations

from typing import Callable, Dict, Optional

import torch

import cnn_ref as R
from detparams import det_tensor

KIND = "deep"


# ------------------------------------------------------------------ deterministic state
def det_state_deep(shapes, ln_prefixes, seed: int = 0) -> Dict[str, torch.Tensor]:
    """cnn_ref.det_state; left alone the LayerNorm weight would be the generic 0.02 n and flatten the model."""
    out = R.det_state(shapes, seed)
    for k, s in shapes:
        pre, leaf = k[: k.rfind(".") + 1], k[k.rfind(".") + 1:]
        if pre in ln_prefixes:
            n = det_tensor(k, tuple(s), seed).float() / 0.02
            out[k] = {"weight": 1.0 + 0.1 * n, "bias": 0.02 * n}[leaf].float()
    return out


def fixture_inputs(fx):
    """(state dict, x, labels) the 'deep' fixture was recorded with, rebuilt from the key names alone."""
    from detparams import det_input, det_labels

    shapes = [(k, tuple(int(d) for d in s.split(",")) if s else ()) for k, s in zip(fx["sd_keys"], fx["sd_shapes"])]
    seed = int(fx["input_seed"])
    name = f"latent_cnn_{KIND}"
    B = fx["logits"].shape[0]
    return (det_state_deep(shapes, fx["ln_prefixes"].tolist()), det_input(name, (B, 18, 512), seed),
            det_labels(name, B, seed=seed))


# ------------------------------------------------------------------ operators
def attnpool(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], B: int, L: int):
    """(y [B, C], a [B, L]): s = x w + bias, a = softmax over each sample's L scores, y = sum_l a_l x_l."""
    C = x.shape[1]
    x3 = x.reshape(B, L, C)
    s = x3 @ w.reshape(C)
    if bias is not None:
        s = s + bias.reshape(())
    a = torch.softmax(s, dim=1)
    return (a[:, :, None] * x3).sum(1), a


def attnpool_bwd(dy: torch.Tensor, x: torch.Tensor, w: torch.Tensor, a: torch.Tensor, B: int, L: int):
    """(dx [B*L, C], dw_part [B, C], dbias_part [B], da [B, L], ds [B, L]) from the saved probabilities."""
    C = x.shape[1]
    x3 = x.reshape(B, L, C)
    da = (x3 * dy[:, None, :]).sum(2)
    ds = a * (da - (a * da).sum(1, keepdim=True))
    dx = a[:, :, None] * dy[:, None, :] + ds[:, :, None] * w.reshape(C)
    return dx.reshape(B * L, C), (ds[:, :, None] * x3).sum(1), ds.sum(1), da, ds


def layernorm(x, gamma, beta, eps: float = 1e-5):
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * gamma + beta


# ------------------------------------------------------------------ model
def forward_deep(sd: Dict[str, torch.Tensor], x: torch.Tensor, train: bool,
                 rnd: Optional[Callable[[torch.Tensor], torch.Tensor]] = None):
    """(logits, buffers after the call, attention weights [B, L]) of create_latent_cnn('deep') with state
    `sd` on x (B, L, D). `rnd` (default: identity) is applied wherever the native bf16 path stores bf16:
    the input rows, the GEMM weight operands, every GEMM / LayerNorm / gate / BatchNorm / pool output.
    LayerNorm and BatchNorm parameters, biases, statistics, the attention weight and bias, the
    probabilities and the final Linear stay in full precision, as they do natively."""
    rnd = rnd or (lambda t: t)
    B, L, D = x.shape
    buf = {}

    def stage(t, conv, bn, k3, res=None):
        w = rnd(sd[conv + ".weight"])
        a = R.conv1d_cols(t, B, L) if k3 else t
        h = a @ w.reshape(w.shape[0], -1).t()
        if conv + ".bias" in sd:
            h = h + sd[conv + ".bias"]
        h = rnd(h)
        y, _, _, rm, rv = R.batchnorm(h, sd[bn + ".weight"], sd[bn + ".bias"], sd[bn + ".running_mean"],
                                      sd[bn + ".running_var"], train, res=res, relu=True)
        buf[bn + ".running_mean"], buf[bn + ".running_var"] = rm, rv
        buf[bn + ".num_batches_tracked"] = sd[bn + ".num_batches_tracked"] + (1 if train else 0)
        return rnd(y)

    t = rnd(x.reshape(B * L, D))
    h = rnd(t @ rnd(sd["input_proj.0.weight"]).t() + sd["input_proj.0.bias"])
    n = rnd(layernorm(h, sd["input_proj.1.weight"], sd["input_proj.1.bias"]))
    t = rnd(torch.relu(n))
    for blk, n_res in (("conv_block1", 1), ("conv_block2", 1), ("conv_block3", 2)):
        t = stage(t, f"{blk}.0.conv", f"{blk}.0.bn", True)
        for j in range(1, 1 + n_res):
            o = stage(t, f"{blk}.{j}.conv1", f"{blk}.{j}.bn1", True)
            t = stage(o, f"{blk}.{j}.conv2", f"{blk}.{j}.bn2", True, res=t)
    pooled, attn = attnpool(t, sd["attention.0.weight"], sd["attention.0.bias"], B, L)
    h = stage(rnd(pooled), "classifier.0", "classifier.1", False)
    return R.logits(h, sd["classifier.4.weight"], sd["classifier.4.bias"]), buf, attn
