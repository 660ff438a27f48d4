"""Generate the LatentCNN2D fixture by running the REFERENCE model code (as make_cnn_deep_golden.py does
for 'deep').

Run once, where the reference checkout exists:
    python tests/golden/make_cnn_2d_golden.py
It imports the reference's torch-only `models_fer_vit/latent_cnn.py`, builds create_latent_cnn('2d') with
dropout 0.0, loads the deterministic state of tests/cnn_ref.py det_state and records latent_cnn_2d.npz with
the record layout of make_cnn_deep_golden.py (B = 4, the (18, 512) input), plus
  pool_nonfirst  for each MaxPool2d of the train-mode forward (forward hooks, torch's own max_pool2d indices),
                 the fraction of 2x2 windows whose argmax is not the top-left pixel.
Seed rule: the first input seed whose train and eval top-1 / top-2 margins are >= 1e-2 on every row and
whose pool_nonfirst is >= 0.5 for both pools (a pool that always took the first pixel could not pass at
model level then).
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
from make_cnn_golden import REF  # noqa: E402

B, L, D = 4, 18, 512
KIND = "2d"


def run_case() -> dict:
    for seed in range(16):
        rec = _run_case(seed)
        if min(rec["margin"].min(), rec["margin_eval"].min()) >= 1e-2 and rec["pool_nonfirst"].min() >= 0.5:
            return rec
    raise AssertionError("2d: no input seed passes the margin and pooling rules")


def _nonfirst(inp: torch.Tensor) -> float:
    """Fraction of the 2x2 windows of an NCHW tensor whose max_pool2d index is not the window's top-left pixel."""
    _, idx = torch.nn.functional.max_pool2d(inp, (2, 2), return_indices=True)
    Ho, Wo, W = idx.shape[2], idx.shape[3], inp.shape[3]
    first = (2 * torch.arange(Ho)[:, None]) * W + 2 * torch.arange(Wo)[None, :]
    return (idx != first).double().mean().item()


def _run_case(seed: int) -> dict:
    from models_fer_vit.latent_cnn import create_latent_cnn

    torch.manual_seed(0)
    model = create_latent_cnn(KIND, dropout=0.0)
    sd0 = model.state_dict()
    det = det_state([(k, tuple(v.shape)) for k, v in sd0.items()])
    model.load_state_dict(det)
    name = f"latent_cnn_{KIND}"
    x, labels = det_input(name, (B, L, D), seed), det_labels(name, B, seed=seed)
    seen = []
    hooks = [m.register_forward_hook(lambda mod, inp, out: seen.append(_nonfirst(inp[0].detach())))
             for m in model.modules() if isinstance(m, torch.nn.MaxPool2d)]
    model.train()
    logits = model(x)
    for h in hooks:
        h.remove()
    loss = torch.nn.CrossEntropyLoss(label_smoothing=0.1)(logits, labels)
    loss.backward()
    rec = {"logits": logits.detach().numpy(), "loss": np.float64(loss.item()), "labels": labels.numpy(),
           "sd_keys": np.array(list(sd0.keys())),
           "sd_shapes": np.array([",".join(str(d) for d in v.shape) for v in sd0.values()]),
           "sd_dtypes": np.array([str(v.dtype) for v in sd0.values()]),
           "n_params": np.int64(sum(p.numel() for p in model.parameters())), "input_seed": np.int64(seed),
           "pool_nonfirst": np.array(seen, dtype=np.float64)}
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
          f"min-margin train={rec['margin'].min():.3g} eval={rec['margin_eval'].min():.3g} "
          f"pool_nonfirst={rec['pool_nonfirst'].round(3).tolist()}")
    return rec


def main() -> None:
    sys.path.insert(0, REF)
    torch.set_num_threads(8)
    np.savez_compressed(os.path.join(HERE, f"latent_cnn_{KIND}.npz"), **run_case())


if __name__ == "__main__":
    main()
