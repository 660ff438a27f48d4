"""Shared pieces of the training steps (`train/train_*.py` train_epoch / evaluate, SURVEY §8
a16), re-done without per-step host synchronisation: the reference calls `loss.item()` and
`preds.cpu()` every step (`train/train_image_vit.py:132-137`), which stalls the stream; here
the loss sum, predictions and labels stay on the device and cross to the host once per epoch,
where accuracy / F1 are computed by the same sklearn calls as the reference.
"""
from __future__ import annotations

import random
from collections import Counter
from typing import Dict, List, Optional

import numpy as np
import torch

from fervit import ops
from fervit._lib import check, lib
from fervit.graph import StepGraph
from fervit.loss import MixupCrossEntropyLoss
from fervit.mixup import DeviceMixup
from fervit.optim import FusedAdamW, clip_grad_norm_ as fused_clip_grad_norm_


def set_seed(seed: int = 42) -> None:
    """`train/train_image_vit.py:30-41`."""
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)


def calculate_class_weights(dataset) -> torch.Tensor:
    """total / (num_classes * count) per class (`train/train_image_vit.py:82-107`); uses the
    packed shard's label table when available instead of loading every sample."""
    if hasattr(dataset, "get_class_counts") and not hasattr(dataset, "indices"):
        counts = Counter(dataset.get_class_counts())
        total = sum(counts.values())
    else:
        base = getattr(dataset, "dataset", dataset)
        idx = getattr(dataset, "indices", range(len(dataset)))
        labels = [int(base[i][1]) for i in idx]
        counts, total = Counter(labels), len(labels)
    nc = len(counts)
    return torch.FloatTensor([total / (nc * counts[i]) if i in counts else 1.0 for i in range(nc)])


def _core(model):
    return getattr(model, "module", model)  # DistributedDataParallel wrapper


def clip_gradients(model, optimizer, max_norm: float) -> None:
    """clip_grad_norm_ without a host round trip: on the flat gradient buffer (coefficient
    consumed by FusedAdamW) or torch's for other optimizers."""
    if isinstance(optimizer, FusedAdamW) and hasattr(_core(model), "fer_flat"):
        fused_clip_grad_norm_(_core(model), max_norm, optimizer=optimizer)
    else:
        torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm)


class EpochStats:
    """Device-side loss sum and prediction / label record of one epoch."""

    def __init__(self, device):
        self.loss = torch.zeros((), dtype=torch.float64, device=device)
        self.preds: List[torch.Tensor] = []
        self.labels: List[torch.Tensor] = []

    def add(self, loss: torch.Tensor, n: int, logits: torch.Tensor, labels: torch.Tensor) -> None:
        self.loss += loss.detach().double() * n
        self.preds.append(logits.detach().argmax(dim=1))
        self.labels.append(labels.detach())

    def finish(self, n_samples: int) -> Dict:
        from sklearn.metrics import accuracy_score, f1_score

        preds = torch.cat(self.preds).cpu().numpy() if self.preds else np.zeros(0, np.int64)
        labels = torch.cat(self.labels).cpu().numpy() if self.labels else np.zeros(0, np.int64)
        return {
            "loss": float(self.loss.item()) / max(n_samples, 1),
            "accuracy": accuracy_score(labels, preds),
            "f1_macro": f1_score(labels, preds, average="macro"),
            "f1_weighted": f1_score(labels, preds, average="weighted"),
            "predictions": preds.tolist(),
            "labels": labels.tolist(),
        }


def run_train_epoch(model, loader, optimizer, criterion, device, mixup: Optional[float] = None, grad_clip=None,
                    metric_forward: bool = False):
    """One epoch of the reference step: [mixup, when `mixup` is not None (the latent trainers:
    lam ~ Beta(a, a) from numpy's global RNG, or 1 for a <= 0, and a CPU randperm every step,
    as `train/train_latent_vit_v2.py:118-125`)], zero_grad, forward,
    criterion (mixed as lam*CE(y) + (1-lam)*CE(y[perm])), backward, [clip], step; metrics from
    the training logits, or (metric_forward) from a second no-grad forward on the unmixed
    batch (`train_latent_vit_v2.py:137-141`). Returns (avg_loss, accuracy, f1_macro)."""
    model.train()
    stats = EpochStats(device)
    n = 0
    for x, y in loader:
        x = x.to(device, non_blocking=True)
        y = y.to(device, non_blocking=True)
        b = x.size(0)
        n += b
        if mixup is not None:
            lam = np.random.beta(mixup, mixup) if mixup > 0 else 1.0
            index = torch.randperm(b).to(device)
            xin = lam * x + (1 - lam) * x[index]
        else:
            lam, index, xin = 1.0, None, x
        optimizer.zero_grad()
        logits = model(xin)
        if index is not None:
            loss = lam * criterion(logits, y) + (1 - lam) * criterion(logits, y[index])
        else:
            loss = criterion(logits, y)
        loss.backward()
        if grad_clip is not None and grad_clip > 0:
            clip_gradients(model, optimizer, grad_clip)
        optimizer.step()
        if metric_forward:
            with torch.no_grad():
                stats.add(loss, b, model(x), y)
        else:
            stats.add(loss, b, logits, y)
    ds = getattr(loader, "dataset", None)
    r = stats.finish(len(ds) if ds is not None else n)
    return r["loss"], r["accuracy"], r["f1_macro"]


class ReplayedTrainEpoch:
    """run_train_epoch's step as one replayed HIP graph (fervit.graph.StepGraph), mixup included: lam and the
    permutation are drawn on the device (fervit.mixup.DeviceMixup) and the two-target loss reads them there
    (MixupCrossEntropyLoss), so nothing of the step is decided on the host and every replay draws afresh.

    The step function, on the static input buffers `x`, `y` ([batch_size, ...]):
        draw -> mix -> zero_grad -> forward -> mixed CE -> backward -> [fused clip] -> FusedAdamW.step
        -> [no-grad forward on the unmixed batch] -> argmax
    writing the static `loss` (fp32 scalar) and `pred` (int64 [batch_size]) buffers. The first `warmup` full
    batches run it eagerly (real training steps, which also size the library workspaces); then it is captured
    once and replayed for every later full batch, across epochs. A last batch shorter than batch_size runs the
    same function eagerly on the leading rows of the buffers, behind an eager fer_step_advance (the counter the
    dropout and mixup seeds and the frozen optimizer's bias correction read). Loss sum and predictions stay on
    the device; run_epoch reads them once, through EpochStats.finish. close() releases the graph and folds the
    replays into the optimizer's host step counts.

    `mixup`: None (no mixup) or the Beta parameter (<= 0: lam = 1, as the reference). `criterion`: a
    CrossEntropyLoss (fervit's or torch's); with mixup its weight and label_smoothing go into a
    MixupCrossEntropyLoss (or pass one). Unlike run_train_epoch's numpy / CPU draws, the draws here come from
    fervit's seed stream (fervit.manual_seed)."""

    def __init__(self, model, optimizer, criterion, device, batch_size: int, mixup: Optional[float] = None,
                 grad_clip=None, metric_forward: bool = False, warmup: int = 2):
        core = _core(model)
        if not isinstance(optimizer, FusedAdamW) or optimizer.model is not core or not hasattr(core, "fer_flat"):
            raise TypeError("ReplayedTrainEpoch needs a FusedAdamW bound to the model (FusedAdamW(..., model=model)): "
                            "the captured step holds its fused update and device step count")
        if warmup < 1:
            raise ValueError("ReplayedTrainEpoch: at least one eager warm-up step sizes the workspaces before capture")
        if not 1 <= batch_size <= ops.MIXUP_MAX_B:
            raise ValueError(f"ReplayedTrainEpoch: batch_size outside 1..{ops.MIXUP_MAX_B}")
        self.model, self.optimizer, self.criterion = model, optimizer, criterion
        self.device = torch.device(device)
        self.batch_size, self.grad_clip, self.metric_forward, self.warmup = batch_size, grad_clip, metric_forward, warmup
        self.mixup = DeviceMixup(mixup, self.device) if mixup is not None else None
        if self.mixup is None or isinstance(criterion, MixupCrossEntropyLoss):
            self.mixed_criterion = criterion
        elif hasattr(criterion, "label_smoothing") and hasattr(criterion, "weight"):
            self.mixed_criterion = MixupCrossEntropyLoss(criterion.weight, criterion.label_smoothing)
        else:
            raise TypeError("ReplayedTrainEpoch: with mixup the criterion is a CrossEntropyLoss (weight, "
                            "label_smoothing) or a MixupCrossEntropyLoss")
        self.x: Optional[torch.Tensor] = None
        self.y = torch.zeros(batch_size, dtype=torch.int64, device=self.device)
        self.loss = torch.zeros((), dtype=torch.float32, device=self.device)
        self.pred = torch.zeros(batch_size, dtype=torch.int64, device=self.device)
        self.logits: Optional[torch.Tensor] = None  # the training logits of the latest step
        self.graph: Optional[StepGraph] = None
        self.stream = torch.cuda.Stream(self.device)  # warm-up and capture (its workspaces: StepGraph.capture)
        self.warm = 0  # eager full-batch steps taken so far
        self.last: Optional[Dict] = None  # EpochStats.finish of the latest epoch

    def step(self, n: int) -> torch.Tensor:
        """One training step on the first n rows of the static buffers."""
        x, y = self.x[:n], self.y[:n]
        xin = self.mixup.draw(n).mix(x) if self.mixup is not None else x
        self.optimizer.zero_grad()
        logits = self.model(xin)
        loss = self.mixed_criterion(logits, y, self.mixup) if self.mixup is not None else self.criterion(logits, y)
        loss.backward()
        if self.grad_clip is not None and self.grad_clip > 0:
            clip_gradients(self.model, self.optimizer, self.grad_clip)
        self.optimizer.step()
        self.logits = logits.detach()
        if self.metric_forward:
            with torch.no_grad():
                self.pred[:n].copy_(self.model(x).argmax(dim=1))
        else:
            self.pred[:n].copy_(self.logits.argmax(dim=1))
        self.loss.copy_(loss.detach())
        return self.loss

    def load(self, x: torch.Tensor, y: torch.Tensor) -> int:
        """Copy a batch into the static buffers; returns its size."""
        n = x.size(0)
        if n > self.batch_size:
            raise ValueError(f"ReplayedTrainEpoch: batch of {n} samples, built for {self.batch_size}")
        if self.x is None:
            self.x = torch.zeros((self.batch_size, *x.shape[1:]), dtype=torch.float32, device=self.device)
        self.x[:n].copy_(x, non_blocking=True)
        self.y[:n].copy_(y, non_blocking=True)
        return n

    def _run(self, n: int) -> None:
        if n < self.batch_size:  # the tail: eager, under the captured step's counter when there is one
            if self.graph is not None:
                check(lib().fer_step_advance(self.graph.counter.data_ptr(), ops.stream()), "step_advance")
            self.step(n)
            return
        if self.graph is None and self.warm < self.warmup:
            cur = torch.cuda.current_stream(self.device)
            self.stream.wait_stream(cur)
            with torch.cuda.stream(self.stream):
                self.step(n)
            cur.wait_stream(self.stream)
            self.warm += 1
            return
        if self.graph is None:
            self.graph = StepGraph(lambda: self.step(self.batch_size), self.optimizer, warmup=0).capture(self.stream)
        self.graph.replay()

    def run_epoch(self, loader, on_step=None):
        """One epoch over `loader`; returns (avg_loss, accuracy, f1_macro) as run_train_epoch does. `on_step(self)`
        is called after every step has been enqueued (logging, tests): the buffers then hold that step's results
        in stream order."""
        self.model.train()
        stats = EpochStats(self.device)
        total = 0
        for x, y in loader:
            n = self.load(x, y)
            total += n
            self._run(n)
            stats.loss.add_(self.loss, alpha=n)
            stats.preds.append(self.pred[:n].clone())
            stats.labels.append(self.y[:n].clone())
            if on_step is not None:
                on_step(self)
        ds = getattr(loader, "dataset", None)
        self.last = stats.finish(len(ds) if ds is not None else total)
        return self.last["loss"], self.last["accuracy"], self.last["f1_macro"]

    def close(self) -> None:
        """Back to eager stepping (StepGraph.release); a later full batch captures again."""
        if self.graph is not None:
            self.graph.release()
            self.graph = None


@torch.no_grad()
def run_evaluate(model, loader, criterion, device) -> Dict:
    """`train/train_image_vit.py:147-178` (same keys), one host transfer per call."""
    model.eval()
    stats = EpochStats(device)
    n = 0
    for x, y in loader:
        x = x.to(device, non_blocking=True)
        y = y.to(device, non_blocking=True)
        logits = model(x)
        stats.add(criterion(logits, y), x.size(0), logits, y)
        n += x.size(0)
    ds = getattr(loader, "dataset", None)
    return stats.finish(len(ds) if ds is not None else n)


def layerwise_param_groups(vit, lr: float, weight_decay: float, log=print) -> list:
    """`train/train_hybrid_latent_vit.py:63-117` / `train_expression_aware_vit.py:66-96`:
    input_proj, adapters and head at 10x lr, transformer at lr (trainable only), pos/cls at 5x
    without weight decay."""
    groups = []
    p = list(vit.input_proj.parameters())
    if p:
        groups.append({"params": p, "lr": lr * 10, "weight_decay": weight_decay})
        log(f"Input projection: lr={lr * 10:.2e}")
    p = [q for q in vit.transformer.parameters() if q.requires_grad]
    if p:
        groups.append({"params": p, "lr": lr, "weight_decay": weight_decay})
        log(f"Transformer: lr={lr:.2e}, params={len(p)}")
    if getattr(vit, "use_adapter", False):
        p = [q for q in vit.adapters.parameters() if q.requires_grad]
        if p:
            groups.append({"params": p, "lr": lr * 10, "weight_decay": weight_decay})
            log(f"Adapters: lr={lr * 10:.2e}")
    p = list(vit.head.parameters())
    if p:
        groups.append({"params": p, "lr": lr * 10, "weight_decay": weight_decay})
        log(f"Head: lr={lr * 10:.2e}")
    groups.append({"params": [vit.pos_embed, vit.cls_token], "lr": lr * 5, "weight_decay": 0})
    log(f"Position/CLS: lr={lr * 5:.2e}")
    return groups
