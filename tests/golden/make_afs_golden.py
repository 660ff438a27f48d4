"""Generate the AFS style-extractor fixture by running the REFERENCE model code.

Run once, where the reference checkout exists:
    python tests/golden/make_afs_golden.py
It loads the reference's torch-only `afs/style_extractor.py` BY FILE PATH (the package __init__ imports pSp),
builds the default StyleExtractor(), loads the deterministic state of tests/cnn_ref.py det_state and, with
B = 4 in train mode, runs the trainer's three-call pattern (tests/afs_ref.py train_step):
    s = h(w_src), t = h(w_tgt), w_new = (w_src - s) + t, n = h(w_new),
    loss = l1(n, t.detach()) + <probe, w_new>     (all three calls receive gradient)
and records afs_style_extractor.npz:
  out_src, out_tgt, out_new, loss        the three outputs and the loss
  grad_keys / grad_sum / grad_l2 / grad_samples / grad_idx
                                         gradient checksums in cnn_ref.check_grads' layout
  buf:<key>                              every BatchNorm buffer after the step (num_batches_tracked == 3)
  out_eval                               the eval-mode output on w_src with those buffers
  adamw_samples                          sampled parameters after one torch.optim.AdamW step
  sd_keys / sd_shapes / sd_dtypes / n_params
Nothing of the reference is copied into the repository; only these numeric vectors are.
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from afs_ref import B_FIX, D_FIX, G_FIX, train_step  # noqa: E402
from cnn_ref import det_state, sample_idx  # noqa: E402
from detparams import det_input  # noqa: E402
from make_cnn_golden import REF  # noqa: E402


def load_reference():
    spec = importlib.util.spec_from_file_location("ref_style_extractor", os.path.join(REF, "afs", "style_extractor.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_case() -> dict:
    ref = load_reference()
    torch.manual_seed(0)
    model = ref.StyleExtractor()
    sd0 = model.state_dict()
    det = det_state([(k, tuple(v.shape)) for k, v in sd0.items()])
    model.load_state_dict(det)
    shape = (B_FIX, G_FIX, D_FIX)
    w_src, w_tgt = det_input("afs_src", shape), det_input("afs_tgt", shape)
    model.train()
    s, t, n, loss = train_step(model, w_src, w_tgt)
    loss.backward()
    rec = {"out_src": s.detach().numpy(), "out_tgt": t.detach().numpy(), "out_new": n.detach().numpy(),
           "loss": np.float64(loss.item()), "sd_keys": np.array(list(sd0.keys())),
           "sd_shapes": np.array([",".join(str(d) for d in v.shape) for v in sd0.values()]),
           "sd_dtypes": np.array([str(v.dtype) for v in sd0.values()]),
           "n_params": np.int64(sum(p.numel() for p in model.parameters()))}
    keys, gsum, gl2, gsamp, gidx = [], [], [], [], []
    for k, p in model.named_parameters():
        g = p.grad.detach().reshape(-1).double()
        idx = sample_idx(k, g.numel())
        keys.append(k)
        gsum.append(g.sum().item())
        gl2.append(g.norm().item())
        sv, ii = np.full(8, np.nan), np.full(8, -1, np.int64)
        sv[: len(idx)], ii[: len(idx)] = g[idx].numpy(), idx
        gsamp.append(sv)
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
        sv = np.full(8, np.nan)
        sv[: len(idx)] = p.detach().reshape(-1)[idx].double().numpy()
        psamp.append(sv)
    rec["adamw_samples"] = np.array(psamp)
    ev = dict(det)
    ev.update(bufs)
    model.load_state_dict(ev)
    model.eval()
    with torch.no_grad():
        rec["out_eval"] = model(w_src).numpy()
    nbt = {int(v) for k, v in bufs.items() if k.endswith("num_batches_tracked")}
    print(f"afs_style_extractor: entries={len(sd0)} params={int(rec['n_params'])} loss={rec['loss']:.6f} "
          f"num_batches_tracked={sorted(nbt)} |out_new| max {np.abs(rec['out_new']).max():.3g}")
    return rec


def main() -> None:
    torch.set_num_threads(8)
    np.savez_compressed(os.path.join(HERE, "afs_style_extractor.npz"), **run_case())


if __name__ == "__main__":
    main()
