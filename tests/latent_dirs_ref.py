"""Host replicas of the direction kernels (csrc/latent_dirs.hip fer_latent_shift, csrc/wplus.hip
fer_latent_dir_draw, csrc/metrics.hip fer_label_change), for tests that rebuild exactly what a kernel did."""
import numpy as np
import torch

import dropmask

DIR_XOR = 0xD1B54A32D192ED03  # csrc/wplus.hip


def dir_draw(seed: int, n: int, n_choices: int, p_keep: float) -> np.ndarray:
    """fer_latent_dir_draw with the step counter unset: int32 [n]. u = u01(hash(seed ^ DIR_XOR, 2i)) in the
    kernel's float32 arithmetic; -1 where u <= p_keep (float32), else (hash(., 2i + 1) * n_choices) >> 32."""
    s = (seed ^ DIR_XOR) & 0xFFFFFFFFFFFFFFFF
    i = np.arange(n, dtype=np.uint64)
    u = dropmask.u01(dropmask.fer_hash(s, 2 * i))
    pick = (dropmask.fer_hash(s, 2 * i + 1) * np.uint64(n_choices)) >> np.uint64(32)  # < 2^32 * 2^31: fits uint64
    return np.where(u <= np.float32(p_keep), -1, pick.astype(np.int64)).astype(np.int32)


def shift_rows(x: torch.Tensor, dirs: torch.Tensor, steps: torch.Tensor, src, c) -> torch.Tensor:
    """out[r] = x[src[r]] + steps[c[r] % S] * dirs[c[r] // S] in torch on the CPU (two fp32 roundings, the
    reference's `w + step * direction`); a c outside [0, K*S) copies the row. x [n, L, D], dirs [K, D] or
    [K, L, D], all fp32 CPU tensors."""
    K, S = dirs.shape[0], steps.shape[0]
    out = torch.empty(len(src), *x.shape[1:], dtype=torch.float32)
    for r, (i, cc) in enumerate(zip(src, c)):
        if 0 <= cc < K * S:
            d = dirs[cc // S]
            out[r] = x[i] + steps[cc % S] * (d.unsqueeze(0) if d.dim() == 1 else d)
        else:
            out[r] = x[i]
    return out


def shift_grid(x: torch.Tensor, dirs: torch.Tensor, steps: torch.Tensor) -> torch.Tensor:
    """Grid mode: rows (k*S + s)*n + i, vectorised (the same two torch operators)."""
    n = x.shape[0]
    K, S = dirs.shape[0], steps.shape[0]
    d = dirs[:, None, :] if dirs.dim() == 2 else dirs               # [K, 1 or L, D]
    prod = steps[None, :, None, None] * d[:, None]                   # [K, S, 1 or L, D]
    return (x[None, None] + prod[:, :, None]).reshape(K * S * n, *x.shape[1:])


def label_change(base: np.ndarray, shifted: np.ndarray, K: int, S: int):
    """(preds [K, S, n], changed [K, n], counts [K], step_counts [K, S]) by torch.argmax on the CPU (lowest
    index of the maximum, a NaN is the maximum and the first NaN wins)."""
    n = base.shape[0]
    bp = torch.from_numpy(np.ascontiguousarray(base)).argmax(1).numpy()
    preds = torch.from_numpy(np.ascontiguousarray(shifted)).argmax(1).numpy().reshape(K, S, n)
    diff = preds != bp[None, None, :]
    changed = diff.any(1)
    return preds.astype(np.int64), changed.astype(np.uint8), changed.sum(1).astype(np.int64), \
        diff.sum(2).astype(np.int64)
