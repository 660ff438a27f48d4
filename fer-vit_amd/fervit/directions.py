"""Expression directions on the device (reference `latent_analysis/compute_expression_direction.py:58-142`:
LinearSVC(max_iter=10000, C=0.1, class_weight='balanced') on the flattened w+ latents, the unit-normalised
`coef_` rows saved as `{prefix}_directions.pt`).

    coef, intercept, info = fit_linear_svm(X, labels, 7, method="binary")
    directions, fit = compute_binary_directions(X, labels)
    save_directions(directions, out_dir, "binary")        # loads with LatentDecomposer.from_file

The fit is the optimum of liblinear's L2-regularised squared-hinge problem with a regularised bias
(intercept_scaling = 1), one column per class k:

    f_k(w, b) = 1/2 |w|^2 + 1/2 b^2 + sum_i c_i max(0, 1 - s_i (w.x_i + b))^2,   s_i = +1 if y_i == k else -1
    binary      c_i = C N / (2 n_k)  for s_i = +1,  C N / (2 (N - n_k))  for s_i = -1   (balanced over {0, 1})
    multiclass  c_i = C N / (K n_k)  for s_i = +1,  C                    for s_i = -1   (liblinear's one-vs-rest
                                                                                  weights only the positive side)

f_k is strongly convex with modulus 1, so the optimum is unique and |theta - theta*| <= |grad f_k(theta)|.

Solver: a truncated Newton method over all columns of a group (<= 8 classes) at once. Every pass over X is one
of the two HIP passes (`ops.svm_hinge` / `ops.svm_scale`: Z = X W^T + b with an epilogue; `ops.svm_xtr`: R^T X);
the [K, F] + [K] vector algebra is torch on the device. Per outer iteration: gradient w - 2 X^T R; conjugate
gradients on (I + 2 X^T D X) d = -grad until |residual| <= 0.1 |grad|; Armijo backtracking from step 1. Step
length, CG coefficients and both stopping rules are per column: a column that has converged gets a zero search
direction and a zero step (never a division by its vanished residual) and rides along in the launches unchanged.
A column has converged when |grad f_k| <= tol |(w, b)|, i.e. when its relative distance from the optimum is at
most tol. There is no CPU path.
"""
from __future__ import annotations

import os
import warnings
from typing import Dict, Tuple

import torch

from . import ops

EMOTION_NAMES = {0: "angry", 1: "disgust", 2: "fear", 3: "happy", 4: "neutral", 5: "sad", 6: "surprise"}
NUM_CLASSES = 7

CG_FORCING = 0.1     # CG stops at |residual| <= CG_FORCING |grad| (liblinear's TRON uses the same 0.1)
ARMIJO = 1e-4        # sufficient-decrease constant
MAX_HALVINGS = 20    # step lengths 1, 1/2, ..., 2^-20


def class_weights(counts, method: str, C: float):
    """(Cp [K], Cn [K]) as float64 CPU tensors from the per-class sample counts."""
    n = torch.as_tensor(counts, dtype=torch.float64)
    N, K = n.sum(), n.numel()
    if method == "binary":
        return C * N / (2.0 * n), C * N / (2.0 * (N - n))
    if method == "multiclass":
        return C * N / (K * n), torch.full_like(n, C)
    raise ValueError(f"fit_linear_svm: method must be 'binary' or 'multiclass', not {method!r}")


def _dot(aW, ab, bW, bb):
    """<(aW, ab), (bW, bb)> per column."""
    return (aW * bW).sum(1) + ab * bb


def _solve_group(X, labels, classes, Cp, Cn, max_iter, tol, max_cg):
    """Newton-CG on the columns `classes` (<= 8) together; returns (W [P, F], b [P], per-column info lists)."""
    N, F = X.shape
    P = classes.numel()
    dev = X.device
    W = torch.zeros(P, F, dtype=torch.float32, device=dev)
    b = torch.zeros(P, dtype=torch.float32, device=dev)
    # the loss is a fixed-order fp32 sum of N non-negative terms (butterfly and four waves inside 256 rows, then
    # the blocks in order): its rounding error is at most this many units of 2^-23 f, on either side of the test
    f_slack = 2.0 ** -23 * 2 * (16 + (N + 255) // 256)

    def objective(W_, b_):
        R_, Dw_, loss, _ = ops.svm_hinge(X, W_, b_, labels, classes, Cp, Cn)
        return R_, Dw_, 0.5 * _dot(W_, b_, W_, b_) + loss

    R, Dw, f = objective(W, b)
    passes = 1
    active = [True] * P          # host copy of the per-column "still iterating" mask
    converged = [False] * P
    col_passes, col_iters = [0] * P, [0] * P
    rel = torch.full((P,), float("inf"))

    def charge(n):
        for k in range(P):
            if active[k]:
                col_passes[k] += n

    charge(1)
    for _ in range(max_iter):
        G, gb = ops.svm_xtr(X, R)
        charge(1)
        gW, gB = W - 2.0 * G, b - 2.0 * gb
        gn = _dot(gW, gB, gW, gB).sqrt()
        tn = _dot(W, b, W, b).sqrt()
        rel_now = (gn / tn).cpu()                       # inf at the zero start
        done = (gn <= tol * tn).cpu()
        for k in range(P):
            if active[k]:
                rel[k] = rel_now[k]
                if bool(done[k]):
                    active[k], converged[k] = False, True
        if not any(active):
            break
        for k in range(P):
            col_iters[k] += int(active[k])
        act = torch.tensor(active, device=dev)
        actf = act.to(torch.float32)

        # ---- conjugate gradients on (I + 2 X^T D X) d = -grad, frozen columns carry zeros
        dW, dB = torch.zeros_like(W), torch.zeros_like(b)
        rW, rB = -gW * actf[:, None], -gB * actf
        pW, pB = rW.clone(), rB.clone()
        rs = _dot(rW, rB, rW, rB)
        stop = (CG_FORCING * gn) ** 2
        cg = act & (rs > stop)
        for _j in range(max_cg):
            if not bool(cg.any()):
                break
            S = ops.svm_scale(X, pW, pB, Dw)
            HG, Hgb = ops.svm_xtr(X, S)
            charge(2)
            HW, HB = pW + 2.0 * HG, pB + 2.0 * Hgb
            zero = torch.zeros_like(rs)
            alpha = torch.where(cg, rs / _dot(pW, pB, HW, HB), zero)
            dW += alpha[:, None] * pW
            dB += alpha * pB
            rW -= alpha[:, None] * HW
            rB -= alpha * HB
            rs_new = _dot(rW, rB, rW, rB)
            cg = cg & (rs_new > stop)
            beta = torch.where(cg, rs_new / rs, zero)
            cgf = cg.to(torch.float32)
            pW = (rW + beta[:, None] * pW) * cgf[:, None]
            pB = (rB + beta * pB) * cgf
            rs = rs_new

        # ---- Armijo backtracking, a step length per column
        gd = _dot(gW, gB, dW, dB)
        step = actf.clone()
        ok = ~act
        for _t in range(MAX_HALVINGS + 1):
            Wn, bn = W + step[:, None] * dW, b + step * dB
            Rn, Dwn, fn = objective(Wn, bn)
            charge(1)
            ok = ok | (fn <= f + ARMIJO * step * gd + f_slack * f.abs())
            if bool(ok.all()):
                break
            step = torch.where(ok, step, 0.5 * step)
        else:
            # no step length reduced some column's objective: it stays where it is and stops iterating
            step = torch.where(ok, step, torch.zeros_like(step))
            Wn, bn = W + step[:, None] * dW, b + step * dB
            Rn, Dwn, fn = objective(Wn, bn)
            charge(1)
            for k, good in enumerate(ok.cpu().tolist()):
                if not good:
                    active[k] = False
        W, b, R, Dw, f = Wn, bn, Rn, Dwn, fn
    return W, b, {"outer_iterations": col_iters, "passes": col_passes, "converged": converged,
                  "relative_gradient": [float(v) for v in rel]}


def fit_linear_svm(X, labels, num_classes: int, method: str = "binary", C: float = 0.1, max_iter: int = 100,
                   tol: float = 2e-4, max_cg: int = 250):
    """One-vs-rest linear SVMs of `num_classes` classes on X (device fp32 [N, F] or [N, L, D]) and integer
    labels [N]: (coef fp32 [K, F], intercept fp32 [K], info). `tol` bounds |grad f_k| / |(w_k, b_k)|, and with it
    each class's relative distance from its optimum; `max_iter` caps the outer Newton iterations and `max_cg` the
    CG iterations inside one. info holds, per class, `outer_iterations`, `passes` (over X, while the class was
    still iterating), `converged` and `relative_gradient` (the last |grad| / |(w, b)| the solver saw), and
    `total_passes`. A class that does not converge warns and reports converged = False (as sklearn does)."""
    if not (torch.is_tensor(X) and X.is_cuda) or not (torch.is_tensor(labels) and labels.is_cuda):
        raise RuntimeError("fervit: the HIP path needs tensors on a ROCm device (no CPU fallback)")
    if X.dtype != torch.float32 or X.dim() not in (2, 3):
        raise ValueError("fit_linear_svm: X must be fp32 [N, F] or [N, L, D]")
    X = X.reshape(X.shape[0], -1)
    if X.stride(1) != 1:
        X = X.contiguous()
    N, K = X.shape[0], int(num_classes)
    if labels.dim() != 1 or labels.shape[0] != N or labels.is_floating_point() or N < 1 or K < 1:
        raise ValueError("fit_linear_svm: labels must be an integer [N] tensor, N >= 1, num_classes >= 1")
    labels = labels.long().contiguous()
    lo, hi = int(labels.min()), int(labels.max())
    if lo < 0 or hi >= K:
        raise ValueError(f"fit_linear_svm: labels must lie in [0, {K}); found {lo if lo < 0 else hi}")
    counts = torch.bincount(labels, minlength=K).cpu()
    if int(counts.min()) == 0:
        raise ValueError(f"fit_linear_svm: class {int(counts.argmin())} has no samples")
    Cp, Cn = class_weights(counts, method, float(C))
    coef = torch.empty(K, X.shape[1], dtype=torch.float32, device=X.device)
    intercept = torch.empty(K, dtype=torch.float32, device=X.device)
    info = {"outer_iterations": [], "passes": [], "converged": [], "relative_gradient": [], "method": method}
    for k0 in range(0, K, ops.SVM_COLUMNS):
        k1 = min(K, k0 + ops.SVM_COLUMNS)
        classes = torch.arange(k0, k1, dtype=torch.int64, device=X.device)
        W, b, part = _solve_group(X, labels, classes, Cp[k0:k1].float().to(X.device), Cn[k0:k1].float().to(X.device),
                                  int(max_iter), float(tol), int(max_cg))
        coef[k0:k1], intercept[k0:k1] = W, b
        for key, v in part.items():
            info[key] += v
    info["total_passes"] = sum(max(info["passes"][k0:k0 + ops.SVM_COLUMNS]) for k0 in range(0, K, ops.SVM_COLUMNS))
    if not all(info["converged"]):
        late = [k for k, c in enumerate(info["converged"]) if not c]
        warnings.warn(f"fit_linear_svm: classes {late} did not reach tol = {tol:g} (relative gradient "
                      f"{[info['relative_gradient'][k] for k in late]}); raise max_iter or tol", RuntimeWarning)
    return coef, intercept, info


def decision_function(X, coef, intercept):
    """X [N, F] or [N, L, D] -> coef x + intercept, fp32 [N, K], by the forward pass in groups of 8 classes."""
    X = X.reshape(X.shape[0], -1)
    K = coef.shape[0]
    Z = torch.empty(X.shape[0], K, dtype=torch.float32, device=X.device)
    for k0 in range(0, K, ops.SVM_COLUMNS):
        k1 = min(K, k0 + ops.SVM_COLUMNS)
        Z[:, k0:k1] = ops.svm_decision(X, coef[k0:k1].contiguous(), intercept[k0:k1].contiguous())
    return Z


def _directions(coef) -> Dict[int, torch.Tensor]:
    unit = coef / (coef.norm(dim=1, keepdim=True) + 1e-12)
    return {k: unit[k] for k in range(unit.shape[0])}


def _fit_directions(X, labels, method, num_classes, fit_args):
    coef, intercept, info = fit_linear_svm(X, labels, num_classes, method=method, **fit_args)
    return _directions(coef), {"coef": coef, "intercept": intercept, "info": info}


def compute_binary_directions(all_w_flat, all_labels, num_classes: int = NUM_CLASSES,
                              **fit_args) -> Tuple[Dict[int, torch.Tensor], Dict]:
    """One class against the rest, balanced over the two sides (`compute_expression_direction.py:58-87`):
    ({class: unit direction fp32 [F] on the device}, {"coef", "intercept", "info"})."""
    return _fit_directions(all_w_flat, all_labels, "binary", num_classes, fit_args)


def compute_multiclass_directions(all_w_flat, all_labels, num_classes: int = NUM_CLASSES,
                                  **fit_args) -> Tuple[Dict[int, torch.Tensor], Dict]:
    """The K-class one-vs-rest fit, balanced over the K classes (`compute_expression_direction.py:90-116`)."""
    return _fit_directions(all_w_flat, all_labels, "multiclass", num_classes, fit_args)


def save_directions(directions, output_dir: str, prefix: str, seq_len: int = 18, latent_dim: int = 512) -> str:
    """`{output_dir}/{prefix}_directions.pt` with the reference's keys (`directions` {class: fp32 [seq_len,
    latent_dim]}, `emotion_names`, `seq_len`, `latent_dim`, `method`): plain tensors, ints and strings, so the file
    loads with weights_only=True (LatentDecomposer.from_file)."""
    os.makedirs(output_dir, exist_ok=True)
    out_path = os.path.join(output_dir, f"{prefix}_directions.pt")
    torch.save({
        "directions": {int(k): torch.as_tensor(n).detach().to("cpu", torch.float32).reshape(seq_len, latent_dim).clone()
                       for k, n in directions.items()},
        "emotion_names": dict(EMOTION_NAMES),
        "seq_len": int(seq_len),
        "latent_dim": int(latent_dim),
        "method": str(prefix),
    }, out_path)
    print(f"\nSaved {prefix} directions -> {out_path}")
    return out_path
