"""Expression directions from the w+ latents of a training split (reference
`latent_analysis/compute_expression_direction.py`, InterFaceGAN's recipe: the normal of a linear SVM's decision
boundary is the attribute's direction), fitted on the device by fervit.directions.

    python latent_analysis/compute_expression_direction.py --latent_dir /path/to/latents/train \\
        --output_dir ./latent_analysis/directions --method both
    python latent_analysis/compute_expression_direction.py --shard train.shard --method binary

The reference's arguments, plus --shard for a packed shard (fervit.data). Prints the class distribution and, per
fit, the training accuracy and report from the device meter (fervit.metrics.ClassificationMeter).
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fervit.directions import (EMOTION_NAMES, NUM_CLASSES, compute_binary_directions,  # noqa: E402
                               compute_multiclass_directions, decision_function, save_directions)
from fervit.metrics import ClassificationMeter  # noqa: E402


def load_all_latents(latent_dir: str):
    """Every `*.pt` sample of `latent_dir` in sorted order: (fp32 [N, L, D], int64 [N]) numpy arrays."""
    files = sorted(f for f in os.listdir(latent_dir) if f.endswith(".pt"))
    if not files:
        raise ValueError(f"No .pt files found in {latent_dir}")
    print(f"Loading {len(files)} latent files from {latent_dir} ...")
    ws, labels = [], []
    for name in files:
        d = torch.load(os.path.join(latent_dir, name), map_location="cpu", weights_only=True)
        ws.append(d["latent"].float().numpy())
        labels.append(int(d["label"]))
    return np.stack(ws, 0), np.asarray(labels, dtype=np.int64)


def load_shard(path: str):
    """A packed shard (fervit.data.pack_latent_dir / write_shard): the same two arrays."""
    from fervit.data import PackedLatentDataset

    ds = PackedLatentDataset(path)
    x = torch.empty(len(ds), ds.L, ds.D, dtype=torch.float32)
    ds.gather(np.arange(len(ds)), x)
    labels = ds.labels.astype(np.int64)
    ds.close()
    return x.numpy(), labels


def print_class_distribution(all_labels) -> None:
    n = len(all_labels)
    print("\nClass distribution:")
    for k in range(NUM_CLASSES):
        count = int((all_labels == k).sum())
        print(f"  {EMOTION_NAMES[k]:>8}: {count:5d} ({count / n * 100:5.1f}%)")


def print_report(title, logits, labels, names) -> float:
    """Training accuracy and the per-class report of argmax(logits) from the device meter."""
    meter = ClassificationMeter(logits.shape[1], logits.device)
    meter.update(logits, labels)
    r = meter.compute()
    print(f"  {title} train accuracy: {r['accuracy']:.4f}")
    per = r["per_class"]
    print(f"    {'':>12} precision    recall  f1-score   support")
    for k, name in enumerate(names):
        print(f"    {name:>12} {per['precision'][k]:9.4f} {per['recall'][k]:9.4f} {per['f1'][k]:9.4f} {per['support'][k]:9d}")
    print(f"    {'macro f1':>12} {r['f1_macro']:9.4f}   weighted f1 {r['f1_weighted']:.4f}   n {r['n']}")
    return r["accuracy"]


def fit_summary(info) -> str:
    return (f"passes over X {info['total_passes']}, outer iterations {info['outer_iterations']}, "
            f"converged {info['converged']}")


def main(argv=None):
    ap = argparse.ArgumentParser(description="Expression direction vectors from linear SVMs on w+ latents, on the device")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--latent_dir", type=str, help="Directory containing .pt latent files (train split)")
    src.add_argument("--shard", type=str, help="Packed latent shard (fervit.data) of the train split")
    ap.add_argument("--output_dir", type=str, default="./latent_analysis/directions")
    ap.add_argument("--method", type=str, default="both", choices=["binary", "multiclass", "both"],
                    help="binary: each class against the rest | multiclass: one 7-class one-vs-rest fit")
    ap.add_argument("--seq_len", type=int, default=18)
    ap.add_argument("--latent_dim", type=int, default=512)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("compute_expression_direction: needs a ROCm device (there is no CPU path)")

    all_w, all_labels = load_shard(args.shard) if args.shard else load_all_latents(args.latent_dir)
    print(f"Loaded: all_w={all_w.shape}, labels={all_labels.shape}")
    print_class_distribution(all_labels)
    X = torch.from_numpy(all_w).reshape(len(all_w), -1).cuda()
    y = torch.from_numpy(all_labels).cuda()
    names = [EMOTION_NAMES[k] for k in range(NUM_CLASSES)]

    if args.method in ("binary", "both"):
        print("\n" + "=" * 60 + "\nComputing BINARY direction vectors (one-vs-rest) ...\n" + "=" * 60)
        dirs, fit = compute_binary_directions(X, y)
        print("  " + fit_summary(fit["info"]))
        Z = decision_function(X, fit["coef"], fit["intercept"])
        for k in range(NUM_CLASSES):
            pos = int((all_labels == k).sum())
            print(f"\n  [{EMOTION_NAMES[k]}] pos={pos}, neg={len(all_labels) - pos}")
            # a two-column logit (0, z): argmax is 1 exactly where the decision value is positive
            print_report(EMOTION_NAMES[k], torch.stack([torch.zeros_like(Z[:, k]), Z[:, k]], 1), (y == k).long(),
                         ["rest", EMOTION_NAMES[k]])
        save_directions(dirs, args.output_dir, "binary", args.seq_len, args.latent_dim)

    if args.method in ("multiclass", "both"):
        print("\n" + "=" * 60 + "\nComputing MULTICLASS direction vectors (7-class SVM) ...\n" + "=" * 60)
        dirs, fit = compute_multiclass_directions(X, y)
        print("  " + fit_summary(fit["info"]))
        print_report("7-class", decision_function(X, fit["coef"], fit["intercept"]), y, names)
        save_directions(dirs, args.output_dir, "multiclass", args.seq_len, args.latent_dim)

    print("\nDone!")


if __name__ == "__main__":
    main()
