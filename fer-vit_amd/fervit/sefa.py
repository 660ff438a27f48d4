"""Non-expression directions (reference `sefa/factorize.py`, `sefa/verify_directions.py`): SeFa's closed-form
factorisation of a StyleGAN weight, and the check that walking a latent along a direction leaves the FER
model's prediction alone.

    dirs = factorize_weight(weight, num_semantics=10)["directions"]            # [K, D]
    results = verify_non_expression_directions(dirs, latents, model)           # label_change_rate per direction
    keep = select_directions(results, max_change_rate=0.05)

The factorisation is one symmetric eigendecomposition of a D x D matrix (D = 512) per run: it stays on the host
in float64. The verification is where the reference spends its time: K x samples x steps model forwards at
batch 1, each followed by a host read of the argmax. Here one launch of `ops.latent_shift` builds every
(direction, step) variant of a batch of samples, the model runs them at full batch size, `ops.label_change`
reduces the logits to change counts on the device, and the host reads the counts once at the end.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import ops

DEFAULT_STEPS = (-3.0, -1.5, 0.0, 1.5, 3.0)


# ------------------------------------------------------------------ factorisation
def factorize_weight(weight, layer_idx: Optional[Sequence[int]] = None, num_semantics: int = 10) -> Dict[str, np.ndarray]:
    """SeFa on a weight A [rows, D] (`sefa/factorize.py:40-59`): the eigenvectors of A^T A with the
    `num_semantics` largest eigenvalues, eigenvalues descending. `layer_idx` keeps those rows of A first.
    Computed in float64 on the host, returned as float32: {"directions": [K, D], "eigenvalues": [K]}.
    An eigenvector's sign is whatever the eigensolver returns, as in the reference."""
    A = weight.detach().cpu().numpy() if isinstance(weight, torch.Tensor) else np.asarray(weight)
    if A.ndim != 2:
        raise ValueError(f"factorize_weight: weight must be a matrix, got shape {A.shape}")
    A = A.astype(np.float64)
    if layer_idx is not None:
        A = A[list(layer_idx), :]
    D = A.shape[1]
    if not 1 <= num_semantics <= D:
        raise ValueError(f"factorize_weight: num_semantics must be in [1, {D}], got {num_semantics}")
    eigenvalues, eigenvectors = np.linalg.eigh(A.T @ A)
    order = np.argsort(eigenvalues)[::-1]
    eigenvalues, eigenvectors = eigenvalues[order], eigenvectors[:, order]
    return {"directions": np.ascontiguousarray(eigenvectors[:, :num_semantics].T, dtype=np.float32),
            "eigenvalues": eigenvalues[:num_semantics].astype(np.float32)}


def factorize_stylegan_weights(stylegan_pkl_path: str, layer_idx: Optional[List[int]] = None,
                               num_semantics: int = 10) -> Dict[str, np.ndarray]:
    """The reference's entry (`sefa/factorize.py:6-59`): unpickle a StyleGAN2-ADA generator, take
    `G.mapping.fc0.weight` and factorise it. Unpickling needs the `stylegan2-ada-pytorch` sources on the path,
    exactly as in the reference; that package is not part of this repository, so this loader is untested here
    (`factorize_weight`, which does all of the arithmetic, is)."""
    import pickle
    import sys

    sys.path.insert(0, "stylegan2-ada-pytorch")
    with open(stylegan_pkl_path, "rb") as f:
        G = pickle.load(f)["G_ema"].to("cpu")
    return factorize_weight(G.mapping.fc0.weight.detach(), layer_idx, num_semantics)


# ------------------------------------------------------------------ verification
def _as_directions(directions, device) -> torch.Tensor:
    d = torch.as_tensor(np.asarray(directions) if not isinstance(directions, torch.Tensor) else directions)
    d = d.to(device=device, dtype=torch.float32).contiguous()
    if d.dim() not in (2, 3) or d.shape[0] < 1:
        raise ValueError(f"directions must be [K, D] or [K, L, D], got {tuple(d.shape)}")
    return d


def label_changes_along_directions(directions, sample_latents, fer_model, step_sizes=DEFAULT_STEPS, device="cuda",
                                   max_samples: Optional[int] = 50, batch_size: int = 1024) -> Dict[str, object]:
    """The device part of `verify_non_expression_directions`, no host read: a dict of device tensors
    `base_preds` int64 [n], `preds` int64 [K, S, n], `changed` uint8 [K, n], `counts` int64 [K],
    `step_counts` int64 [K, S], and `steps` (the S non-zero step sizes, a list) and `n`.

    Samples are taken in blocks of at most batch_size // S, and for each block the directions in chunks whose
    K_c * S * n_c rows fit `batch_size` (one direction and one sample at the least)."""
    dev = torch.device(device)
    steps = [float(s) for s in step_sizes if float(s) != 0.0]  # `verify_directions.py:54`
    x = sample_latents if max_samples is None else sample_latents[:max_samples]
    x = torch.as_tensor(x).to(device=dev, dtype=torch.float32).contiguous()
    if x.dim() != 3:
        raise ValueError(f"sample_latents must be [N, L, D], got {tuple(x.shape)}")
    dirs = _as_directions(directions, dev)
    if tuple(dirs.shape[1:]) not in ((x.shape[2],), tuple(x.shape[1:])):
        raise ValueError(f"directions {tuple(dirs.shape)} do not match latents {tuple(x.shape)}")
    K, S, n = dirs.shape[0], len(steps), x.shape[0]
    fer_model.eval()
    out = {"steps": steps, "n": n,
           "base_preds": torch.empty(n, dtype=torch.int64, device=dev),
           "preds": torch.empty(K, S, n, dtype=torch.int64, device=dev),
           "changed": torch.zeros(K, n, dtype=torch.uint8, device=dev),
           "counts": torch.zeros(K, dtype=torch.int64, device=dev),
           "step_counts": torch.zeros(K, S, dtype=torch.int64, device=dev)}
    if n == 0 or S == 0:
        return out
    batch_size = max(1, int(batch_size))
    steps_t = torch.tensor(steps, dtype=torch.float32, device=dev)
    n_c = min(n, max(1, batch_size // S))
    k_c = max(1, batch_size // (S * n_c))
    with torch.no_grad():
        base = torch.cat([fer_model(x[i:i + batch_size]).float() for i in range(0, n, batch_size)], 0)
        out["base_preds"].copy_(base.argmax(1))
        for i0 in range(0, n, n_c):
            xs, bs = x[i0:i0 + n_c], base[i0:i0 + n_c]
            for k0 in range(0, K, k_c):
                dk = dirs[k0:k0 + k_c]
                logits = fer_model(ops.latent_shift(xs, dk, steps_t)).float()
                preds, changed, _, _ = ops.label_change(bs, logits, dk.shape[0], S, counts=out["counts"][k0:k0 + k_c],
                                                        step_counts=out["step_counts"][k0:k0 + k_c])
                out["preds"][k0:k0 + k_c, :, i0:i0 + n_c] = preds
                out["changed"][k0:k0 + k_c, i0:i0 + n_c] = changed
    return out


def verify_non_expression_directions(directions, sample_latents, fer_model, stylegan_generator=None,
                                     step_sizes=DEFAULT_STEPS, device: str = "cuda", max_samples: Optional[int] = 50,
                                     batch_size: int = 1024, verbose: bool = True) -> List[dict]:
    """`sefa/verify_directions.py:6-78`: for each direction, the share of samples whose predicted label changes
    at any non-zero step along it. Returns the reference's list of {"direction_idx", "label_change_rate"}, each
    with "step_change_rate" added: {step: share of samples whose prediction at that step differs}.

    directions [K, D] (broadcast over the layers, the reference's case) or [K, L, D]; sample_latents [N, L, D];
    fer_model: any model of this package that maps fp32 [B, L, D] to logits (put in eval mode here).
    max_samples = 50 is the reference's cap (`:45`), None takes every sample. `stylegan_generator` is unused,
    as in the reference. One host read, after the last launch."""
    r = label_changes_along_directions(directions, sample_latents, fer_model, step_sizes, device, max_samples,
                                       batch_size)
    n, steps = r["n"], r["steps"]
    counts, step_counts = r["counts"].cpu().numpy(), r["step_counts"].cpu().numpy()
    results = []
    for k in range(counts.shape[0]):
        rate = float(counts[k]) / n if n else 0.0
        results.append({"direction_idx": k, "label_change_rate": rate,
                        "step_change_rate": {s: float(step_counts[k, j]) / n for j, s in enumerate(steps)}})
        if verbose:
            print(f"Direction {k:02d}: label change rate = {rate:.3f}")
    return results


def select_directions(results: List[dict], max_change_rate: float) -> List[int]:
    """Indices of the directions whose label_change_rate is at most `max_change_rate`, in the results' order:
    the `direction_indices` of `augment_latents_with_directions`."""
    return [int(r["direction_idx"]) for r in results if r["label_change_rate"] <= max_change_rate]
