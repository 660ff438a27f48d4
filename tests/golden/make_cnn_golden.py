"""Generate the LatentCNN fixtures by running the REFERENCE model code.

Run once, where the reference checkout exists (as make_golden.py):
    python tests/golden/make_cnn_golden.py
It imports the reference's torch-only `models_fer_vit/latent_cnn.py`, builds
create_latent_cnn('standard') and ('light') with dropout 0.0, loads the deterministic state of
tests/cnn_ref.py det_state (detparams.py values by state_dict key, BatchNorm entries moved to usable
ranges), and records into latent_cnn_<kind>.npz:
  sd_keys / sd_shapes / sd_dtypes and the parameter count,
  the train-mode logits and CrossEntropyLoss(label_smoothing=0.1) at B = 4, L = 18,
  per-parameter gradient {sum, L2, 8 samples},
  every buffer after that step (running_mean, running_var, num_batches_tracked),
  8 samples of every parameter after one AdamW step (lr 1e-3, weight decay 0.05),
  eval-mode logits of the deterministic parameters with those updated buffers.
Nothing of the reference is copied into the repository; only these numeric vectors are.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from cnn_ref import det_state, sample_idx  # noqa: E402
from detparams import det_input, det_labels  # noqa: E402

REF = "/root/reference"
B, L, D = 4, 18, 512


def run_case(kind: str) -> dict:
    """SURVEY section 7 fixture rule: argmax equality needs a top-1 / top-2 margin >= 1e-2 on every row, in
    the train and in the eval logits. BatchNorm couples the rows of a batch, so instead of picking rows
    the whole batch is redrawn: the first input seed that passes is used and stored (`input_seed`)."""
    for seed in range(16):
        rec = _run_case(kind, seed)
        if min(rec["margin"].min(), rec["margin_eval"].min()) >= 1e-2:
            return rec
    raise AssertionError(f"{kind}: no input seed passes the margin rule")


def _run_case(kind: str, seed: int) -> dict:
    from models_fer_vit.latent_cnn import create_latent_cnn

    torch.manual_seed(0)
    model = create_latent_cnn(kind, dropout=0.0)
    sd0 = model.state_dict()
    det = det_state([(k, v.shape) for k, v in sd0.items()])
    model.load_state_dict(det)
    name = f"latent_cnn_{kind}"
    x, labels = det_input(name, (B, L, D), seed), det_labels(name, B, seed=seed)
    model.train()
    logits = model(x)
    loss = torch.nn.CrossEntropyLoss(label_smoothing=0.1)(logits, labels)
    loss.backward()
    rec = {"logits": logits.detach().numpy(), "loss": np.float64(loss.item()), "labels": labels.numpy(),
           "sd_keys": np.array(list(sd0.keys())),
           "sd_shapes": np.array([",".join(str(d) for d in v.shape) for v in sd0.values()]),
           "sd_dtypes": np.array([str(v.dtype) for v in sd0.values()]),
           "n_params": np.int64(sum(p.numel() for p in model.parameters())), "input_seed": np.int64(seed)}
    top = torch.topk(logits.detach(), 2, dim=1).values
    rec["margin"] = (top[:, 0] - top[:, 1]).numpy()
    keys, gsum, gl2, gsamp, gidx = [], [], [], [], []
    for k, p in model.named_parameters():
        g = p.grad.detach().reshape(-1).double()
        idx = sample_idx(k, g.numel())
        keys.append(k)
        gsum.append(g.sum().item())
        gl2.append(g.norm().item())
        s, ii = np.full(8, np.nan), np.full(8, -1, np.int64)
        s[: len(idx)], ii[: len(idx)] = g[idx].numpy(), idx
        gsamp.append(s)
        gidx.append(ii)
    rec.update(grad_keys=np.array(keys), grad_sum=np.array(gsum), grad_l2=np.array(gl2),
               grad_samples=np.array(gsamp), grad_idx=np.array(gidx))
    bufs = {k: v.detach().clone() for k, v in model.named_buffers()}
    for k, v in bufs.items():
        rec["buf:" + k] = v.numpy()
    torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=0.05).step()
    psamp = []
    for k, p in model.named_parameters():
        idx = sample_idx(k, p.numel())
        s = np.full(8, np.nan)
        s[: len(idx)] = p.detach().reshape(-1)[idx].double().numpy()
        psamp.append(s)
    rec["adamw_samples"] = np.array(psamp)
    ev = dict(det)
    ev.update(bufs)
    model.load_state_dict(ev)
    model.eval()
    with torch.no_grad():
        le = model(x)
    rec["logits_eval"] = le.numpy()
    top = torch.topk(le, 2, dim=1).values
    rec["margin_eval"] = (top[:, 0] - top[:, 1]).numpy()
    print(f"{name}: seed={seed} entries={len(sd0)} params={int(rec['n_params'])} loss={rec['loss']:.6f} "
          f"min-margin train={rec['margin'].min():.3g} eval={rec['margin_eval'].min():.3g}")
    return rec


def main() -> None:
    sys.path.insert(0, REF)
    torch.set_num_threads(8)
    for kind in ("standard", "light"):
        np.savez_compressed(os.path.join(HERE, f"latent_cnn_{kind}.npz"), **run_case(kind))


if __name__ == "__main__":
    main()
