"""Classification metrics kept on the device (reference `eval/evaluate_model.py:135-159`, and the
accuracy / f1 the trainers take from sklearn on the host).

    meter = ClassificationMeter(num_classes=7, device="cuda")
    for x, y in loader:
        preds, conf = meter.update(model(x), y)      # one launch, no sync
    report = meter.compute()                         # one launch, one host transfer

`update` is one fer_cls_stats launch: argmax by torch's rule, softmax confidence, and the batch added to
the int64 confusion matrix (row = label, column = prediction) on the device. A label outside
[0, num_classes) (-100, -1, ...) is counted as skipped and left out of the matrix. `compute` is one
fer_cls_report launch and one transfer of the report and the matrix. Nothing here has a CPU path.
"""
from __future__ import annotations

from typing import Dict

import torch

from . import ops


class ClassificationMeter:
    def __init__(self, num_classes: int, device) -> None:
        if int(num_classes) < 1:
            raise ValueError("ClassificationMeter: num_classes must be >= 1")
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("fervit: the HIP path needs tensors on a ROCm device (no CPU fallback)")
        self.num_classes = int(num_classes)
        # one buffer: the matrix, then the two counters (rows counted, rows skipped), zeroed by one fill
        self._state = torch.zeros(self.num_classes * self.num_classes + 2, dtype=torch.int64, device=device)
        self.confusion = self._state[:-2].view(self.num_classes, self.num_classes)
        self.counters = self._state[-2:]

    def reset(self) -> None:
        self._state.zero_()

    def update(self, logits: torch.Tensor, labels: torch.Tensor, want_probs: bool = False):
        """Adds one batch; returns (preds int64 [B], conf fp32 [B]) and, with want_probs, probs fp32 [B, C].
        One launch on the current stream, no host sync; works under torch.cuda.graph capture."""
        if logits.dim() != 2 or logits.shape[1] != self.num_classes:
            raise ValueError(f"ClassificationMeter: logits must be [B, {self.num_classes}]")
        logits = logits.detach()
        if logits.dtype != torch.float32 or (logits.shape[1] > 1 and logits.stride(1) != 1):
            logits = logits.float().contiguous()
        labels = labels.detach()
        if labels.dtype != torch.int64 or (labels.numel() > 1 and labels.stride(0) != 1):
            labels = labels.long().contiguous()
        preds, conf, probs = ops.cls_stats(logits, labels, confusion=self.confusion, counters=self.counters,
                                           want_probs=want_probs)
        return (preds, conf, probs) if want_probs else (preds, conf)

    def compute(self) -> Dict:
        """accuracy, f1_macro, f1_weighted (sklearn's definitions, zero_division = 0, macro over the classes
        present in labels or predictions), per_class {precision, recall, f1, support} as lists, confusion
        (numpy int64 [C, C]), n and skipped."""
        C = self.num_classes
        report = ops.cls_report(self.confusion)
        # the int64 state rides along as the bit pattern of fp64 words: one transfer for everything
        host = torch.cat([report, self._state.view(torch.float64)]).cpu()
        rep = host[:4 + 4 * C]
        state = host[4 + 4 * C:].view(torch.int64)
        per = rep[4:].view(C, 4)
        return {
            "accuracy": float(rep[0]),
            "f1_macro": float(rep[1]),
            "f1_weighted": float(rep[2]),
            "n": int(rep[3]),
            "per_class": {
                "precision": per[:, 0].tolist(),
                "recall": per[:, 1].tolist(),
                "f1": per[:, 2].tolist(),
                "support": [int(v) for v in per[:, 3].tolist()],
            },
            "confusion": state[:-2].view(C, C).numpy().copy(),
            "skipped": int(state[-1]),
        }
