"""`train/train_latent_vit_v2.py` step functions (train_epoch 107-149, evaluate 152-183):
args.mixup (default 1.0) and args.grad_clip (default 1.0, `:441`)."""
from __future__ import annotations

from .common import ReplayedTrainEpoch, calculate_class_weights, run_evaluate, run_train_epoch, set_seed  # noqa: F401


def train_epoch(model, loader, optimizer, criterion, device, args):
    return run_train_epoch(model, loader, optimizer, criterion, device, mixup=float(args.mixup),
                           grad_clip=float(args.grad_clip) if args.grad_clip and args.grad_clip > 0 else None,
                           metric_forward=True)


def make_replayed_epoch(model, optimizer, criterion, device, batch_size: int, args, warmup: int = 2):
    """train_epoch's step (args.mixup, args.grad_clip) as a replayed graph with the mixup drawn on the device
    (common.ReplayedTrainEpoch): `runner.run_epoch(loader)` per epoch, `runner.close()` at the end."""
    return ReplayedTrainEpoch(model, optimizer, criterion, device, batch_size, mixup=float(args.mixup),
                              grad_clip=float(args.grad_clip) if args.grad_clip and args.grad_clip > 0 else None,
                              metric_forward=True, warmup=warmup)


def evaluate(model, loader, criterion, device):
    return run_evaluate(model, loader, criterion, device)
