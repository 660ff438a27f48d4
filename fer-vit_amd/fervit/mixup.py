"""DeviceMixup: the mixup of the latent trainers (`train/train_latent_vit_v2.py:118-130`) with lam and the batch
permutation drawn on the device, so that a captured training step (fervit.graph.StepGraph) draws afresh on every
replay: the draw kernel mixes the device step counter into the host seed it was captured with, as the dropout
kernels do. The reference-faithful host draw (numpy's Beta, a CPU randperm) stays in
train.common.run_train_epoch."""
from __future__ import annotations

from typing import Optional

import torch

from . import ops, runtime


class DeviceMixup:
    """Owns the device `lam` (one fp32) and `perm` (int32) buffers, at fixed addresses for the life of the object.

        mix = DeviceMixup(alpha=1.0)
        mix.draw(x.shape[0])                # lam ~ Beta(alpha, alpha), or exactly 1 for alpha <= 0; a permutation
        logits = model(mix.mix(x))          # lam * x + (1 - lam) * x[perm]
        loss = MixupCrossEntropyLoss()(logits, y, mix)
    """

    def __init__(self, alpha: float = 1.0, device=None):
        self.alpha = float(alpha)
        self.B = 0
        self._lam: Optional[torch.Tensor] = None
        self._perm: Optional[torch.Tensor] = None
        if device is not None:
            self._buffers(torch.device(device))

    def _buffers(self, device) -> None:
        if self._lam is None or self._lam.device != device:
            self._lam = torch.ones(1, dtype=torch.float32, device=device)
            self._perm = torch.arange(ops.MIXUP_MAX_B, dtype=torch.int32, device=device)

    def draw(self, B: int, device=None) -> "DeviceMixup":
        """A new lam and a new permutation of B samples, seeded from runtime.next_seed()."""
        if not 1 <= B <= ops.MIXUP_MAX_B:
            raise ValueError(f"DeviceMixup: batch size {B} outside 1..{ops.MIXUP_MAX_B}")
        if self._lam is None or device is not None:
            self._buffers(torch.device(device) if device is not None
                          else torch.device("cuda", torch.cuda.current_device()))
        ops.mixup_draw(self.alpha, B, runtime.next_seed(), self._lam, self._perm)
        self.B = B
        return self

    @property
    def lam(self) -> torch.Tensor:
        return self._lam

    @property
    def perm(self) -> torch.Tensor:
        return self._perm[:self.B]

    def mix(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The mixed batch of the last draw; x [B, ...] fp32, B the drawn batch size."""
        if x.shape[0] != self.B:
            raise ValueError(f"DeviceMixup.mix: batch of {x.shape[0]}, drew for {self.B}")
        return ops.mixup_apply(x.contiguous(), self.perm, self._lam, out)
