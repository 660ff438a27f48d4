"""Training latents pushed along the kept non-expression directions (reference `data/augment_latents.py`).

`augment_latents_with_directions` writes the reference's expanded directory, every file's variants from one
`ops.latent_shift` launch. A training run does not need that directory: `fervit.data.PackedLatentLoader` with
`augment=dict(directions=...)` draws "(direction, step) or unchanged" per sample on the device, which is the
per-sample distribution of reading the expanded directory uniformly, and `fervit.data.augment_shard` writes the
expanded set as one packed shard where a file is wanted.
"""
import os
import sys
from typing import List

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fervit import ops  # noqa: E402
from fervit.data import augment_shard  # noqa: E402,F401


def augment_latents_with_directions(latent_dir: str, output_dir: str, directions: np.ndarray,
                                    direction_indices: List[int],
                                    step_sizes: List[float] = [-2.0, -1.0, 1.0, 2.0]):
    """`data/augment_latents.py:8-77`: for every `.pt` sample of `latent_dir`, the original and one file per kept
    direction and step, `{base}_dir{d}_step{step:.1f}.pt` = {"latent": w + step * directions[d], "label",
    "augmented": True, "direction_idx": d, "step": step}, into `output_dir`. An existing file is left alone.
    The variants of a file are one device launch; the latents written are bit-equal to the reference's."""
    os.makedirs(output_dir, exist_ok=True)
    direction_indices = [int(i) for i in direction_indices]
    steps = [float(s) for s in step_sizes]
    K, S = len(direction_indices), len(steps)
    if K and S:
        dirs = torch.as_tensor(np.asarray(directions)[direction_indices], dtype=torch.float32).cuda().contiguous()
        steps_t = torch.tensor(steps, dtype=torch.float32, device="cuda")
    pt_files = [f for f in os.listdir(latent_dir) if f.endswith(".pt")]
    for fname in pt_files:
        data = torch.load(os.path.join(latent_dir, fname), weights_only=False)
        w, label = data["latent"], data["label"]
        out_path = os.path.join(output_dir, fname)
        if not os.path.exists(out_path):
            torch.save(data, out_path)
        if not (K and S):
            continue
        base = os.path.splitext(fname)[0]
        names = [[os.path.join(output_dir, f"{base}_dir{d}_step{step:.1f}.pt") for step in steps]
                 for d in direction_indices]
        if all(os.path.exists(p) for row in names for p in row):
            continue
        x = w.detach().to(device="cuda", dtype=torch.float32).reshape(1, -1, w.shape[-1]).contiguous()
        variants = ops.latent_shift(x, dirs, steps_t).reshape(K, S, *w.shape).cpu()
        for ki, d in enumerate(direction_indices):
            for si, step in enumerate(steps):
                if not os.path.exists(names[ki][si]):
                    torch.save({"latent": variants[ki, si].clone(), "label": label, "augmented": True,
                                "direction_idx": d, "step": step_sizes[si]}, names[ki][si])
    original_count = len(pt_files)
    aug_count = original_count * K * S
    print(f"\nDone: {original_count} originals + {aug_count} augmented = {original_count + aug_count} samples")
    print(f"Output: {output_dir}")
