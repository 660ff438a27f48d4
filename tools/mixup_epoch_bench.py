"""Times the latent trainers' default training epoch -- mixup 1.0, grad-clip 1.0, a second no-grad forward for the
metrics (`train/train_latent_vit_v2.py:107-149`) -- on latent_vit at batch 256, eager against replayed, interleaved
on one device.

    python tools/mixup_epoch_bench.py [--batch 256] [--dtype bf16] [--steps 20] [--rounds 6]

  A  eager:    train.common.run_train_epoch (numpy Beta draw, CPU randperm + copy, two fer_cross_entropy launches
               and torch glue per step)
  B  replayed: train.common.ReplayedTrainEpoch (device draw, mixing and two-target loss kernels inside one
               captured graph, replayed per batch)
Each arm has its own model and FusedAdamW (lr 1e-4, wd 0.05) and runs over the same `steps` device-resident
batches per block. Two untimed blocks per arm (B's first holds its two eager warm-up steps and the capture), then
`rounds` alternating blocks A, B, A, B, ...; a block is one epoch call, timed on the host from the call to its
return (the return reads the epoch's loss and predictions, so the device is idle again). One JSON line per arm:
median and fastest block in ms per step, and the ratio B / A."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fer-vit_amd"))


def build(dtype):
    from fervit.loss import CrossEntropyLoss
    from fervit.optim import FusedAdamW
    from models_fer_vit.latent_vit import LatentViT

    torch.manual_seed(42)
    m = LatentViT().cuda()
    m.set_precision(dtype)
    opt = FusedAdamW(m.parameters(), lr=1e-4, weight_decay=0.05, model=m)
    return m, opt, CrossEntropyLoss(label_smoothing=0.1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--steps", type=int, default=20, help="batches per block (one epoch call)")
    ap.add_argument("--rounds", type=int, default=6, help="timed blocks per arm")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mixup_epoch_bench: needs a ROCm device (timings on a CPU say nothing)")
    import fervit
    from train.common import ReplayedTrainEpoch, run_train_epoch, set_seed

    set_seed(42)
    fervit.manual_seed(1234)
    g = torch.Generator(device="cuda").manual_seed(7)
    loader = [(torch.randn(args.batch, 18, 512, device="cuda", generator=g),
               torch.randint(0, 7, (args.batch,), device="cuda", generator=g)) for _ in range(args.steps)]
    ma, oa, ca = build(args.dtype)
    mb, ob, cb = build(args.dtype)
    runner = ReplayedTrainEpoch(mb, ob, cb, "cuda", args.batch, mixup=1.0, grad_clip=1.0, metric_forward=True)
    arms = {"A eager run_train_epoch": lambda: run_train_epoch(ma, loader, oa, ca, "cuda", mixup=1.0, grad_clip=1.0,
                                                               metric_forward=True),
            "B ReplayedTrainEpoch": lambda: runner.run_epoch(loader)}
    ms = {k: [] for k in arms}
    try:
        for rnd in range(-2, args.rounds):
            for k, epoch in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                loss = epoch()[0]
                dt = (time.perf_counter() - t0) * 1e3 / args.steps
                assert loss == loss, k  # not NaN
                if rnd >= 0:
                    ms[k].append(dt)
    finally:
        runner.close()
    med = {k: statistics.median(v) for k, v in ms.items()}
    a, b = list(arms)
    for k, v in ms.items():
        rec = {"arm": k, "model": "latent_vit", "B": args.batch, "dtype": args.dtype, "mixup": 1.0, "grad_clip": 1.0,
               "metric_forward": True, "steps_per_block": args.steps, "blocks": len(v),
               "steps_timed": len(v) * args.steps, "median_ms_per_step": round(med[k], 4),
               "min_ms_per_step": round(min(v), 4), "device": torch.cuda.get_device_name(0)}
        if k == b:
            rec["replayed_over_eager"] = round(med[b] / med[a], 3)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
