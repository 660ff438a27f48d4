"""Fused softmax cross-entropy (nn.CrossEntropyLoss(label_smoothing, weight), mean
reduction; `train/train_image_vit.py:262-267`) on device, loss and dlogits in one launch."""
from __future__ import annotations

import torch

from . import ops


class _CEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, weight, ls):
        loss, dl = ops.cross_entropy(logits.contiguous().float(), labels.contiguous(), weight, ls)
        ctx.dl = dl
        return loss

    @staticmethod
    def backward(ctx, g):
        return ctx.dl * g, None, None, None


class CrossEntropyLoss(torch.nn.Module):
    def __init__(self, weight=None, label_smoothing: float = 0.0):
        super().__init__()
        self.weight = weight
        self.label_smoothing = float(label_smoothing)

    def forward(self, logits, labels):
        w = None if self.weight is None else self.weight.to(logits.device).float().contiguous()
        return _CEFn.apply(logits, labels.long(), w, self.label_smoothing)


class _CEMixFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, perm, lam, weight, ls):
        loss, dl = ops.cross_entropy_mix(logits.contiguous().float(), labels.contiguous(), perm, lam, weight, ls)
        ctx.dl = dl
        return loss

    @staticmethod
    def backward(ctx, g):
        return ctx.dl * g, None, None, None, None, None


class MixupCrossEntropyLoss(torch.nn.Module):
    """lam * CE(logits, y) + (1 - lam) * CE(logits, y[perm]) (`train/train_latent_vit_v2.py:127-130`) with lam
    and perm read from a fervit.mixup.DeviceMixup's device buffers: one launch for the loss and dlogits, and
    nothing of the draw on the host, so a captured step follows each replay's draw."""

    def __init__(self, weight=None, label_smoothing: float = 0.0):
        super().__init__()
        self.weight = weight
        self.label_smoothing = float(label_smoothing)

    def forward(self, logits, labels, mixup):
        if logits.shape[0] != mixup.B:
            raise ValueError(f"MixupCrossEntropyLoss: batch of {logits.shape[0]}, the mixup drew for {mixup.B}")
        w = None if self.weight is None else self.weight.to(logits.device).float().contiguous()
        return _CEMixFn.apply(logits, labels.long(), mixup.perm, mixup.lam, w, self.label_smoothing)
