"""The numbers of the reference's `eval/evaluate_model.py`, without its plots.

    meter = ClassificationMeter(7, device)
    results = evaluate_model(model, test_loader, device, meter)      # predictions, labels, probabilities
    summary = classification_summary(meter, emotion_names)           # what evaluation_results.json holds
    cls_sim, tok_sim = fervit.explain.token_similarity(model, latents)   # visualize_attention's two arrays

evaluate_model (`eval/evaluate_model.py:135-159`) keeps the reference's three keys; argmax, softmax and the
confusion matrix are one device launch per batch (ClassificationMeter.update) and everything crosses to
the host in one transfer at the end. classification_summary is sklearn's
classification_report(output_dict=True) and the accuracy the reference's main() writes, taken from the
meter's device report. Figures (matplotlib, seaborn) are the caller's concern.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch

from fervit.metrics import ClassificationMeter


def evaluate_model(model, data_loader, device, meter: Optional[ClassificationMeter] = None) -> Dict:
    """Reference `evaluate_model`: {'predictions' int64 [n], 'labels' int64 [n], 'probabilities' fp32 [n, C]}
    as numpy. `meter` (made here when not given, then sized by the first batch's logits) accumulates the
    confusion matrix of the same pass."""
    model.eval()
    preds, labs, probs = [], [], []
    with torch.no_grad():
        for x, y in data_loader:
            x = x.to(device, non_blocking=True)
            y = y.to(device, non_blocking=True).long()
            logits = model(x)
            if meter is None:
                meter = ClassificationMeter(logits.shape[1], logits.device)
            p, _, pr = meter.update(logits, y, want_probs=True)
            preds.append(p)
            labs.append(y)
            probs.append(pr)
    if not preds:
        return {"predictions": np.zeros(0, np.int64), "labels": np.zeros(0, np.int64),
                "probabilities": np.zeros((0, 0), np.float32)}
    n, C = sum(p.numel() for p in preds), probs[0].shape[1]
    # one transfer: the three records as bytes of one buffer
    host = torch.cat([torch.cat(preds).view(torch.uint8), torch.cat(labs).view(torch.uint8),
                      torch.cat(probs).reshape(-1).view(torch.uint8)]).cpu()
    return {
        "predictions": host[:8 * n].view(torch.int64).numpy().copy(),
        "labels": host[8 * n:16 * n].view(torch.int64).numpy().copy(),
        "probabilities": host[16 * n:].view(torch.float32).view(n, C).numpy().copy(),
    }


def classification_summary(meter: ClassificationMeter, class_names: Sequence[str], model_config=None,
                           checkpoint_path: Optional[str] = None) -> Dict:
    """The dict the reference's main() writes to evaluation_results.json: accuracy, classification_report
    (sklearn's output_dict layout: one entry per class present in labels or predictions, 'accuracy',
    'macro avg', 'weighted avg'), model_config, checkpoint_path, test_dataset_size."""
    r = meter.compute()
    C = meter.num_classes
    if len(class_names) != C:
        raise ValueError(f"classification_summary: {len(class_names)} class names for {C} classes")
    per, cm = r["per_class"], r["confusion"]
    present = [c for c in range(C) if cm[c].sum() + cm[:, c].sum() > 0]
    report = {class_names[c]: {"precision": per["precision"][c], "recall": per["recall"][c], "f1-score": per["f1"][c],
                               "support": per["support"][c]} for c in present}
    n = r["n"]

    def avg(key, weighted):
        if not present or (weighted and n == 0):
            return 0.0
        if weighted:
            return float(sum(per[key][c] * per["support"][c] for c in present) / n)
        return float(sum(per[key][c] for c in present) / len(present))

    report["accuracy"] = r["accuracy"]
    report["macro avg"] = {"precision": avg("precision", False), "recall": avg("recall", False),
                           "f1-score": r["f1_macro"], "support": n}
    report["weighted avg"] = {"precision": avg("precision", True), "recall": avg("recall", True),
                              "f1-score": r["f1_weighted"], "support": n}
    return {"accuracy": r["accuracy"], "classification_report": report, "model_config": model_config,
            "checkpoint_path": checkpoint_path, "test_dataset_size": n}
