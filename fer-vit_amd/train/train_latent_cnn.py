"""`train/train_latent_cnn.py` step functions (train_epoch 104-144, evaluate 147-179): mixup with
alpha fixed at 1.0 (`:116`), no gradient clipping, metrics from a second no-grad forward on the
unmixed batch. That metric forward runs under model.train() (`:134-136`), so it normalises with batch
statistics and moves BatchNorm's running statistics a second time each step (num_batches_tracked
advances by two per batch); kept as the reference has it."""
from __future__ import annotations

from .common import ReplayedTrainEpoch, calculate_class_weights, run_evaluate, run_train_epoch, set_seed  # noqa: F401


def train_epoch(model, loader, optimizer, criterion, device, mixup: float = 1.0):
    return run_train_epoch(model, loader, optimizer, criterion, device, mixup=mixup, metric_forward=True)


def make_replayed_epoch(model, optimizer, criterion, device, batch_size: int, mixup: float = 1.0, warmup: int = 2):
    """train_epoch's step as a replayed graph with the mixup drawn on the device (common.ReplayedTrainEpoch);
    the metric forward stays under model.train(), as above."""
    return ReplayedTrainEpoch(model, optimizer, criterion, device, batch_size, mixup=mixup, metric_forward=True,
                              warmup=warmup)


def evaluate(model, loader, criterion, device):
    return run_evaluate(model, loader, criterion, device)
