"""Tensor-level wrappers around the C ABI (one call = one or two kernel launches).

Every wrapper takes device tensors, checks shapes/strides on the host before the
launch (kernels assume what the host verified), and enqueues on PyTorch's current
HIP stream. Nothing here has a CPU path.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import torch

from . import _lib
from ._lib import Epilogue, GemmDesc, check, lib

ACT = {"none": 0, "gelu": 1, "relu": 2, "mul": 3}  # "mul": aux_act only (v *= aux)
PRE_GATE = 16  # act flag: `pre` receives act'(pre) * keep * drop_scale (include/fervit.h)

# Optional callable(desc, epilogue, launch) used by bench.py to bracket launches with HIP events.
LAUNCH_PROBE = None


def dcode(t: torch.Tensor) -> int:
    if t.dtype == torch.bfloat16:
        return 0
    if t.dtype == torch.float32:
        return 1
    raise TypeError(f"fervit: unsupported activation dtype {t.dtype}")


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def C_ref(x):
    return ctypes.byref(x)


def _dev(t: torch.Tensor) -> None:
    if not t.is_cuda:
        raise RuntimeError("fervit: the HIP path needs tensors on a ROCm device (no CPU fallback)")


# ------------------------------------------------------------------ workspace
class _Workspace:
    """Grow-only fp32 scratch per (device, slot, stream): users on one stream are ordered by it,
    and the weight-gradient stream (runtime.WGRAD) gets buffers of its own."""

    def __init__(self):
        self.buf = {}

    def get(self, nbytes: int, device, slot: int = 0) -> torch.Tensor:
        key = (device, slot, torch.cuda.current_stream(device).cuda_stream)
        b = self.buf.get(key)
        n = max(1, (int(nbytes) + 3) // 4)
        if b is None or b.numel() < n:
            b = torch.empty(int(n * 1.25) + 1024, dtype=torch.float32, device=device)
            self.buf[key] = b
        return b


WS = _Workspace()


def drop_args(p: float):
    """(thresh, scale): an element is dropped iff its 16-bit uniform < thresh = round(p*65536)."""
    if p <= 0.0:
        return 0, 1.0
    if p >= 1.0:
        return 65536, 0.0
    thr = max(1, min(65535, int(round(p * 65536.0))))
    return thr, 1.0 / (1.0 - p)


def seed64(seed: int) -> int:
    """A Python int seed as the ABI's uint64_t."""
    return seed & 0xFFFFFFFFFFFFFFFF


# The argument groups most entry points share, each as the tuple the header spells out.
def _row(t: Optional[torch.Tensor], ld: int):
    """(pointer, row stride) of an optional row operand; `ld` goes with a null pointer."""
    return (None, ld) if t is None else (t.data_ptr(), t.stride(0))


def _drop(p: float, seed: int):
    """(drop_thresh, drop_scale, seed) of dropout probability p."""
    return (*drop_args(p), seed64(seed))


def _ws(nbytes: int, device, slot: int = 0, need: bool = True):
    """(pointer, bytes) of the workspace; (null, 0) when the call needs none."""
    if not need:
        return None, 0
    w = WS.get(nbytes, device, slot)
    return w.data_ptr(), w.numel() * 4


def _alloc(out: Optional[torch.Tensor], like: torch.Tensor, shape=None, dtype=None) -> torch.Tensor:
    """`out` when given, else a new tensor on like's device, with like's shape and dtype unless given."""
    if out is not None:
        return out
    if shape is None and dtype is None:
        return torch.empty_like(like)
    return torch.empty(like.shape if shape is None else shape, dtype=like.dtype if dtype is None else dtype,
                       device=like.device)


# ------------------------------------------------------------------ GEMM
def gemm(A: torch.Tensor, B: torch.Tensor, out: torch.Tensor, *, a_kc: bool = True, b_kc: bool = True,
         M: int, N: int, K: int, lda: Optional[int] = None, ldb: Optional[int] = None, ldc: Optional[int] = None,
         bias: Optional[torch.Tensor] = None, act: str = "none", pre: Optional[torch.Tensor] = None,
         res: Optional[torch.Tensor] = None, dropout: float = 0.0, seed: int = 0, drop_ld: Optional[int] = None,
         aux: Optional[torch.Tensor] = None, aux_act: str = "none", alpha: float = 1.0, accumulate: bool = False,
         post_scale: Optional[torch.Tensor] = None, split_ws: bool = True,
         colsum: Optional[torch.Tensor] = None, colsum_accumulate: bool = False,
         pre_gate: bool = False, ws_exact: bool = False) -> torch.Tensor:
    """out[m][n] = epilogue(sum_k A(m,k) B(n,k)); see include/fervit.h for the layouts.
    colsum: optional fp32 [N] receiving (or, with colsum_accumulate, adding) sum_m out[m][n].
    pre_gate: `pre` receives act'(pre) * dropout keep * scale (consumed by aux_act="mul").
    ws_exact: report the split-K workspace as the bytes asked for, not the (grow-only, shared) buffer's size.
    The library caps the split count by the workspace it is given, so where that cap binds (a few output
    tiles over a very long K) the summation order would otherwise depend on what ran before on the stream."""
    _dev(A)
    if A.dtype != B.dtype:
        raise TypeError("gemm: A and B dtypes differ")
    d = GemmDesc()
    d.dtype = dcode(A)
    d.A, d.B = A.data_ptr(), B.data_ptr()
    d.lda = lda if lda is not None else (K if a_kc else M)
    d.ldb = ldb if ldb is not None else (K if b_kc else N)
    d.a_kc, d.b_kc = int(a_kc), int(b_kc)
    d.M, d.N, d.K = M, N, K
    t256 = -(-M // 256) * -(-N // 256)
    if colsum is not None:
        d.ws, d.ws_bytes = _ws(lib().fer_gemm_colsum_ws(M, N), A.device, slot=1)
    elif split_ws and d.dtype == 0 and K >= 1024 and t256 < 256:
        # split-K slabs: the library targets ~one 256x256 workgroup per CU (or 512 128^2 ones)
        nb = 4 * M * N * min(32, max(2, 512 // t256)) + 4 * (-(-M // 128) * -(-N // 128)) + 256  # + tile tickets
        d.ws, d.ws_bytes = _ws(nb, A.device, slot=1)
        if ws_exact:
            d.ws_bytes = nb
    e = Epilogue()
    e.c = out.data_ptr()
    e.ldc = ldc if ldc is not None else N
    e.c_f32 = int(out.dtype == torch.float32)
    e.accumulate = int(accumulate)
    e.alpha = alpha
    e.bias = ptr(bias)
    e.act = ACT[act] | (PRE_GATE if pre_gate else 0)
    e.pre, e.ldp = _row(pre, N)
    e.res, e.ldr = _row(res, N)
    e.drop_thresh, e.drop_scale, e.seed = _drop(dropout, seed)
    e.drop_ld = drop_ld if drop_ld is not None else N
    e.aux, e.ldx = _row(aux, N)
    e.aux_act = ACT[aux_act]
    e.post_scale = ptr(post_scale)
    e.colsum = ptr(colsum)
    e.colsum_accumulate = int(colsum_accumulate)
    if LAUNCH_PROBE is not None:
        LAUNCH_PROBE(d, e, lambda: check(lib().fer_gemm(C_ref(d), C_ref(e), stream()), "gemm"))
    else:
        check(lib().fer_gemm(C_ref(d), C_ref(e), stream()), "gemm")
    return out


def linear_fwd(x, w, b=None, out=None, **kw):
    """y = x w^T + b for x [M,K], w [N,K] (nn.Linear)."""
    M, K = x.shape
    N = w.shape[0]
    return gemm(x, w, _alloc(out, x, (M, N)), M=M, N=N, K=K, bias=b, **kw)


def linear_dgrad(dy, w, out=None, **kw):
    """dx = dy w for dy [M,N], w [N,K]."""
    M, N = dy.shape
    K = w.shape[1]
    return gemm(dy, w, _alloc(out, dy, (M, K)), a_kc=True, b_kc=False, M=M, N=K, K=N, lda=N, ldb=K, **kw)


def linear_wgrad_group(items, splits: int = 0):
    """dW_i (+)= dy_i^T x_i for several nn.Linear weights sharing the token count, in one launch
    (csrc/gemm.hip gemm_wgrad_group_kernel). items: (dy [M,N] bf16, x [M,K] bf16, out fp32 [N,K],
    accumulate) tuples; at most 8."""
    n = len(items)
    arr = (_lib.WgradItem * n)()
    for i, (dy, x, out, acc) in enumerate(items):
        _dev(dy)
        if dy.dtype != torch.bfloat16 or x.dtype != torch.bfloat16 or out.dtype != torch.float32:
            raise TypeError("linear_wgrad_group: bf16 dy / x and fp32 out")
        M, N = dy.shape
        K = x.shape[1]
        if x.shape[0] != M or tuple(out.shape) != (N, K) or dy.stride(1) != 1 or x.stride(1) != 1 or out.stride(1) != 1:
            raise ValueError("linear_wgrad_group: shapes / row-major layouts")
        arr[i] = _lib.WgradItem(dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0),
                                M, N, K, int(bool(acc)))
    nb = lib().fer_wgrad_group_ws(arr, n, splits)
    check(lib().fer_wgrad_group(arr, n, splits, *_ws(nb, items[0][0].device, slot=1, need=nb > 0), stream()),
          "wgrad_group")


def linear_wgrad(dy, x, out, accumulate=False, **kw):
    """dW (+)= dy^T x for dy [M,N], x [M,K]; out fp32 [N,K]."""
    M, N = dy.shape
    K = x.shape[1]
    return gemm(dy, x, out, a_kc=False, b_kc=False, M=N, N=K, K=M, lda=dy.stride(0), ldb=x.stride(0),
                accumulate=accumulate, **kw)


# ------------------------------------------------------------------ LayerNorm
def layernorm_fwd(x, w, b, eps, out=None, mean=None, rstd=None):
    M, D = x.shape
    out = _alloc(out, x)
    check(lib().fer_layernorm_fwd(dcode(x), x.data_ptr(), x.stride(0), w.data_ptr(), b.data_ptr(), 1, 1,
                                  out.data_ptr(), out.stride(0), ptr(mean), ptr(rstd), M, D, eps, stream()),
          "layernorm_fwd")
    return out


def layernorm_bwd(dy, x, mean, rstd, w, dx=None, res=None, dx_drop=None, dropout=0.0, seed=0, dgamma=None,
                  dbeta=None, dbias=None, accumulate=False):
    M, D = x.shape
    dx = _alloc(dx, x)
    check(lib().fer_layernorm_bwd(dcode(x), dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), mean.data_ptr(),
                                  rstd.data_ptr(), w.data_ptr(), 1, 1, *_row(res, D), dx.data_ptr(), dx.stride(0),
                                  ptr(dx_drop), *_drop(dropout, seed), ptr(dgamma), ptr(dbeta), ptr(dbias),
                                  int(accumulate), *_ws(lib().fer_layernorm_bwd_ws(M, D), x.device), M, D, stream()),
          "layernorm_bwd")
    return dx


# ------------------------------------------------------------------ attention
def attention_saved(qkv, B, N, H, dh, dropout=0.0) -> torch.Tensor:
    """fp32 buffer for the state fer_attention_fwd keeps for the backward: lse [B*H*N] first
    (`saved[:B*H*N]`), then the dropout keep bits of the fast bf16 path."""
    thr, _ = drop_args(dropout)
    n = lib().fer_attention_saved_floats(dcode(qkv), B, N, H, dh, thr)
    return torch.empty(n, dtype=torch.float32, device=qkv.device)


def attention_fwd(qkv, out, saved, B, N, H, dh, dropout=0.0, seed=0):
    """out = attention(qkv); `saved` from attention_saved() (same B, N, H, dh, dropout)."""
    nb = lib().fer_attention_ws(dcode(qkv), B, N, H)
    check(lib().fer_attention_fwd(dcode(qkv), qkv.data_ptr(), qkv.stride(0), out.data_ptr(), out.stride(0),
                                  saved.data_ptr(), saved.numel(), B, N, H, dh, 1.0 / math.sqrt(dh),
                                  *_drop(dropout, seed), *_ws(nb, qkv.device, need=bool(nb)), stream()),
          "attention_fwd")
    return out


def attention_bwd(qkv, out, dout, saved, dqkv, B, N, H, dh, dropout=0.0, seed=0, colsum=None,
                  colsum_accumulate=False):
    """dqkv = d(attention)/d(qkv); colsum (fp32 [3*H*dh], optional) (+)= column sums of dqkv
    (the in_proj bias gradient), fused into the backward kernel."""
    nb = lib().fer_attention_ws(dcode(qkv), B, N, H)
    check(lib().fer_attention_bwd(dcode(qkv), qkv.data_ptr(), qkv.stride(0), out.data_ptr(), out.stride(0),
                                  dout.data_ptr(), dout.stride(0), saved.data_ptr(), saved.numel(), dqkv.data_ptr(),
                                  dqkv.stride(0), *_ws(nb, qkv.device, need=bool(nb)), B, N, H, dh,
                                  1.0 / math.sqrt(dh), *_drop(dropout, seed), ptr(colsum), int(colsum_accumulate),
                                  stream()), "attention_bwd")
    return dqkv


def attention_probs(qkv, B, N, H, dh, *, average_heads=True, q_start=0, q_count=None, out=None):
    """fp32 softmax(Q K^T / sqrt(dh)) of query rows q_start .. q_start+q_count-1 (default: all rows
    from q_start) of the qkv buffer attention_fwd takes; eval semantics (no dropout).
    average_heads: [B, q_count, N], the mean over heads (what nn.MultiheadAttention returns with
    need_weights=True); else [B, H, q_count, N]. The per-head tensor is never written when averaging."""
    _dev(qkv)
    code = dcode(qkv)
    B, N, H, dh, q_start = int(B), int(N), int(H), int(dh), int(q_start)
    if min(B, N, H, dh) < 1:
        raise ValueError("attention_probs: B, N, H, dh must be >= 1")
    if qkv.dim() != 2 or qkv.shape[0] != B * N or qkv.shape[1] < 3 * H * dh or qkv.stride(1) != 1 \
            or qkv.stride(0) < 3 * H * dh:
        raise ValueError("attention_probs: qkv must be [B*N, >= 3*H*dh] with unit column stride")
    nq = N - q_start if q_count is None else int(q_count)
    if q_start < 0 or nq < 1 or q_start + nq > N:
        raise ValueError(f"attention_probs: query rows {q_start}..{q_start + nq - 1} outside [0, {N})")
    shape = (B, nq, N) if average_heads else (B, H, nq, N)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=qkv.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous() or out.device != qkv.device:
        raise ValueError(f"attention_probs: out must be a contiguous fp32 {shape} tensor on qkv's device")
    check(lib().fer_attention_probs(code, qkv.data_ptr(), qkv.stride(0), B, N, H, dh, 1.0 / math.sqrt(dh),
                                    int(bool(average_heads)), q_start, nq, out.data_ptr(), out.numel(), stream()),
          "attention_probs")
    return out


def attention_rollout_cls(maps, residual=0.5, out=None):
    """CLS row [B, N] of the attention rollout of head-averaged maps [L, B, N, N] (fp32):
    row 0 of A'_L ... A'_1 with A'_l = residual * I + (1 - residual) * A_l."""
    _dev(maps)
    if maps.dtype != torch.float32 or maps.dim() != 4 or maps.shape[2] != maps.shape[3] or not maps.is_contiguous():
        raise ValueError("attention_rollout_cls: maps must be a contiguous fp32 [L, B, N, N] tensor")
    if not 0.0 <= float(residual) < 1.0:
        raise ValueError("attention_rollout_cls: residual must be in [0, 1)")
    L, B, N, _ = maps.shape
    if L < 1 or B < 1 or N < 1:
        raise ValueError("attention_rollout_cls: empty maps")
    if out is None:
        out = torch.empty(B, N, dtype=torch.float32, device=maps.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (B, N) or not out.is_contiguous() or out.device != maps.device:
        raise ValueError("attention_rollout_cls: out must be a contiguous fp32 [B, N] tensor on maps' device")
    check(lib().fer_attention_rollout_cls(maps.data_ptr(), L, B, N, float(residual), out.data_ptr(), stream()),
          "attention_rollout_cls")
    return out


# ------------------------------------------------------------------ evaluation metrics
def _out(name, t, like, shape, dtype):
    """An optional caller-given output: `dtype`, `shape`, unit last stride, on like's device."""
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or t.device != like.device or \
            (t.dim() and t.shape[-1] > 1 and t.stride(-1) != 1):
        raise ValueError(f"{name} must be a {dtype} {tuple(shape)} tensor with unit last stride on the input's device")
    return t


def cls_stats(logits, labels, *, confusion=None, counters=None, want_preds=True, want_conf=True, want_probs=False):
    """One fer_cls_stats launch on fp32 logits [B, C] (unit column stride) and int64 labels [B]: returns
    (preds int64 [B], conf fp32 [B], probs fp32 [B, C]), None for what was not asked for. `confusion`
    (int64 [C, C], contiguous) and `counters` (int64 [2]: rows counted, rows skipped) are accumulated in
    place; a label outside [0, C) is skipped. No host sync: usable under graph capture."""
    _dev(logits)
    _dev(labels)
    if logits.dtype != torch.float32 or logits.dim() != 2 or logits.shape[1] < 1 or \
            (logits.shape[1] > 1 and logits.stride(1) != 1):
        raise ValueError("cls_stats: logits must be fp32 [B, C >= 1] with unit column stride")
    B, C = logits.shape
    if labels.dtype != torch.int64 or tuple(labels.shape) != (B,) or (B > 1 and labels.stride(0) != 1):
        raise ValueError("cls_stats: labels must be a contiguous int64 [B] tensor")
    if confusion is not None and not _out("cls_stats: confusion", confusion, logits, (C, C), torch.int64).is_contiguous():
        raise ValueError("cls_stats: confusion must be contiguous")
    if counters is not None:
        _out("cls_stats: counters", counters, logits, (2,), torch.int64)
    preds = torch.empty(B, dtype=torch.int64, device=logits.device) if want_preds else None
    conf = torch.empty(B, dtype=torch.float32, device=logits.device) if want_conf else None
    probs = torch.empty(B, C, dtype=torch.float32, device=logits.device) if want_probs else None
    if B == 0:
        return preds, conf, probs
    check(lib().fer_cls_stats(logits.data_ptr(), logits.stride(0) if B > 1 else max(C, logits.stride(0)),
                              labels.data_ptr(), B, C, ptr(preds), ptr(conf), ptr(probs), C, ptr(confusion),
                              ptr(counters), stream()), "cls_stats")
    return preds, conf, probs


def cls_report(confusion, out=None):
    """fer_cls_report of a contiguous int64 [C, C] confusion matrix: fp64 [4 + 4 C] on the device
    (accuracy, f1_macro, f1_weighted, n, then precision, recall, f1, support per class)."""
    _dev(confusion)
    if confusion.dtype != torch.int64 or confusion.dim() != 2 or confusion.shape[0] != confusion.shape[1] \
            or confusion.shape[0] < 1 or not confusion.is_contiguous():
        raise ValueError("cls_report: confusion must be a contiguous int64 [C, C] tensor, C >= 1")
    C = confusion.shape[0]
    if out is None:
        out = torch.empty(4 + 4 * C, dtype=torch.float64, device=confusion.device)
    elif not _out("cls_report: out", out, confusion, (4 + 4 * C,), torch.float64).is_contiguous():
        raise ValueError("cls_report: out must be contiguous")
    check(lib().fer_cls_report(confusion.data_ptr(), C, out.data_ptr(), stream()), "cls_report")
    return out


def token_cosine(tokens, eps=1e-8, want_cls=True, want_tok=True):
    """fer_token_cosine of tokens [B, N, D] (bf16 or fp32; unit column stride, batch stride N * row
    stride): (cls_sim fp32 [B, N-1], tok_sim fp32 [B, N-1, N-1]), None for what was not asked for."""
    _dev(tokens)
    code = dcode(tokens)
    if tokens.dim() != 3 or tokens.shape[1] < 2 or tokens.shape[2] < 1:
        raise ValueError("token_cosine: tokens must be [B, N >= 2, D]")
    B, N, D = tokens.shape
    if tokens.stride(2) != 1 or tokens.stride(1) < D or (B > 1 and tokens.stride(0) != N * tokens.stride(1)):
        raise ValueError("token_cosine: tokens need unit column stride and a batch stride of N rows")
    if not (want_cls or want_tok):
        raise ValueError("token_cosine: no output requested")
    cls = torch.empty(B, N - 1, dtype=torch.float32, device=tokens.device) if want_cls else None
    tok = torch.empty(B, N - 1, N - 1, dtype=torch.float32, device=tokens.device) if want_tok else None
    check(lib().fer_token_cosine(code, tokens.data_ptr(), tokens.stride(1), B, N, D, float(eps), ptr(cls), N - 1,
                                 ptr(tok), N - 1, stream()), "token_cosine")
    return cls, tok


def label_change(base, shifted, K, S, *, counts=None, step_counts=None, want_preds=True, want_changed=True):
    """One fer_label_change launch: base fp32 [n, C] and shifted fp32 [K*S*n, C] logits (unit column stride,
    shifted in latent_shift's grid order) -> (preds int64 [K, S, n], changed uint8 [K, n], counts int64 [K],
    step_counts int64 [K, S]); None for preds / changed not asked for. `counts` and `step_counts` are
    accumulated in place when given (contiguous), else start from zero. No host sync."""
    _dev(base)
    _dev(shifted)
    for name, t in (("base", base), ("shifted", shifted)):
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] < 1 or (t.shape[1] > 1 and t.stride(1) != 1):
            raise ValueError(f"label_change: {name} must be fp32 [rows, C >= 1] with unit column stride")
    n, C = base.shape
    if K < 1 or S < 1 or tuple(shifted.shape) != (K * S * n, C):
        raise ValueError("label_change: shifted must be [K * S * n, C] with K, S >= 1")
    dev = base.device
    if counts is None:
        counts = torch.zeros(K, dtype=torch.int64, device=dev)
    elif not _out("label_change: counts", counts, base, (K,), torch.int64).is_contiguous():
        raise ValueError("label_change: counts must be contiguous")
    if step_counts is None:
        step_counts = torch.zeros(K, S, dtype=torch.int64, device=dev)
    elif not _out("label_change: step_counts", step_counts, base, (K, S), torch.int64).is_contiguous():
        raise ValueError("label_change: step_counts must be contiguous")
    preds = torch.empty(K, S, n, dtype=torch.int64, device=dev) if want_preds else None
    changed = torch.empty(K, n, dtype=torch.uint8, device=dev) if want_changed else None
    if n:
        check(lib().fer_label_change(base.data_ptr(), base.stride(0) if n > 1 else max(C, base.stride(0)),
                                     shifted.data_ptr(), max(C, shifted.stride(0)), K, S, n, C, ptr(preds),
                                     ptr(changed), counts.data_ptr(), step_counts.data_ptr(), stream()),
              "label_change")
    return preds, changed, counts, step_counts


# ------------------------------------------------------------------ latent directions
def _latents(name, t):
    """fp32 [n, L, D] with contiguous samples (the sample stride is free, at least L * D)."""
    _dev(t)
    if t.dtype != torch.float32 or t.dim() != 3 or t.shape[1] < 1 or t.shape[2] < 1:
        raise ValueError(f"latent_shift: {name} must be fp32 [n, L, D]")
    n, L, D = t.shape
    if (D > 1 and t.stride(2) != 1) or (L > 1 and t.stride(1) != D) or (n > 1 and t.stride(0) < L * D):
        raise ValueError(f"latent_shift: {name} needs contiguous [L, D] samples at a stride of at least L * D")
    return L * D if n <= 1 else t.stride(0)


def latent_shift(x, directions, steps, choice=None, out=None):
    """fer_latent_shift: x fp32 [n, L, D] pushed along `directions` (fp32 [K, D], broadcast over the layers, or
    [K, L, D]) by `steps` (fp32 [S] on the device). choice=None: every (direction, step) variant,
    out [K*S*n, L, D] in (direction, step, sample) order. choice int32 [n]: row i takes pair choice[i] = k*S + s,
    or stays bit for bit when the value is outside [0, K*S); out [n, L, D], and out=x shifts in place.
    The product and the sum are rounded separately: bit-equal to torch's `x + step * d` on the CPU."""
    ldx = _latents("x", x)
    n, L, D = x.shape
    for t in (directions, steps):
        _dev(t)
    if directions.dtype != torch.float32 or not directions.is_contiguous() or directions.shape[0] < 1 or \
            tuple(directions.shape[1:]) not in ((D,), (L, D)):
        raise ValueError("latent_shift: directions must be contiguous fp32 [K, D] or [K, L, D], K >= 1")
    K, dir_layers = directions.shape[0], (1 if directions.dim() == 2 else L)
    if steps.dtype != torch.float32 or steps.dim() != 1 or steps.shape[0] < 1 or not steps.is_contiguous():
        raise ValueError("latent_shift: steps must be a contiguous fp32 [S] tensor, S >= 1")
    S = steps.shape[0]
    if choice is not None:
        _dev(choice)
        if choice.dtype != torch.int32 or tuple(choice.shape) != (n,) or not choice.is_contiguous():
            raise ValueError("latent_shift: choice must be a contiguous int32 [n] tensor")
    rows = n if choice is not None else K * S * n
    if out is None:
        out = torch.empty(rows, L, D, dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != (rows, L, D) or out.device != x.device:
        raise ValueError(f"latent_shift: out must be [{rows}, {L}, {D}] on x's device")
    ldo = _latents("out", out)
    if choice is None and rows and out.untyped_storage().data_ptr() == x.untyped_storage().data_ptr():
        raise ValueError("latent_shift: in place only with a choice")
    check(lib().fer_latent_shift(x.data_ptr(), ldx, directions.data_ptr(), dir_layers, steps.data_ptr(), ptr(choice),
                                 out.data_ptr(), ldo, n, K, S, L, D, stream()), "latent_shift")
    return out


def latent_dir_draw(n, n_choices, p_keep, seed, device="cuda", out=None):
    """fer_latent_dir_draw: int32 [n] on `device`, -1 (unchanged) with probability p_keep, else uniform over
    [0, n_choices): the `choice` of latent_shift."""
    if out is None:
        out = torch.empty(n, dtype=torch.int32, device=device)
    elif out.dtype != torch.int32 or tuple(out.shape) != (n,) or not out.is_contiguous():
        raise ValueError("latent_dir_draw: out must be a contiguous int32 [n] tensor")
    _dev(out)
    check(lib().fer_latent_dir_draw(out.data_ptr(), n, int(n_choices), float(p_keep), seed64(seed), stream()),
          "latent_dir_draw")
    return out


# ------------------------------------------------------------------ linear-SVM passes
SVM_COLUMNS = 8  # columns (one-vs-rest problems) per launch


def svm_slab() -> int:
    """Rows per slab of fer_svm_xtr's fixed summation order."""
    return lib().fer_svm_slab()


def _svm_x(X, what):
    _dev(X)
    if X.dtype != torch.float32 or X.dim() != 2 or X.shape[0] < 1 or X.shape[1] < 1 or \
            (X.shape[1] > 1 and X.stride(1) != 1) or (X.shape[0] > 1 and X.stride(0) < X.shape[1]):
        raise ValueError(f"{what}: X must be fp32 [N >= 1, F >= 1] with unit column stride")
    N, F = X.shape
    return N, F, (X.stride(0) if N > 1 else max(F, X.stride(0)))


def _svm_cols(name, t, like, rows, P, dtype=torch.float32):
    """A contiguous [rows, P] (or [P] for rows = None) operand on like's device."""
    shape = (P,) if rows is None else (rows, P)
    if t.dtype != dtype or tuple(t.shape) != shape or t.device != like.device or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {dtype} {shape} tensor on X's device")
    return t


def _svm_forward(X, W, bias, epilogue, labels, classes, Cp, Cn, Dw, want_z):
    what = "svm_hinge" if epilogue == 0 else "svm_scale"
    N, F, ldx = _svm_x(X, what)
    if W.dim() != 2 or not 1 <= W.shape[0] <= SVM_COLUMNS:
        raise ValueError(f"{what}: W must be [P, F] with 1 <= P <= {SVM_COLUMNS}")
    P = W.shape[0]
    _svm_cols(f"{what}: W", W, X, P, F)
    _svm_cols(f"{what}: bias", bias, X, None, P)
    R = torch.empty(N, P, dtype=torch.float32, device=X.device)
    Z = torch.empty(N, P, dtype=torch.float32, device=X.device) if want_z else None
    loss = None
    if epilogue == 0:
        _svm_cols(f"{what}: labels", labels, X, None, N, torch.int64)
        _svm_cols(f"{what}: classes", classes, X, None, P, torch.int64)
        _svm_cols(f"{what}: Cp", Cp, X, None, P)
        _svm_cols(f"{what}: Cn", Cn, X, None, P)
        Dw = torch.empty(N, P, dtype=torch.float32, device=X.device)
        loss = torch.empty(P, dtype=torch.float32, device=X.device)
    else:
        _svm_cols(f"{what}: Dw", Dw, X, N, P)
    check(lib().fer_svm_forward(X.data_ptr(), ldx, W.data_ptr(), F, bias.data_ptr(), N, F, P, epilogue, ptr(labels),
                                ptr(classes), ptr(Cp), ptr(Cn), ptr(Z), P, R.data_ptr(), P, Dw.data_ptr(), P, ptr(loss),
                                *_ws(lib().fer_svm_ws(N, F), X.device), stream()), what)
    return R, Dw, loss, Z


def svm_hinge(X, W, bias, labels, classes, Cp, Cn, want_z=False):
    """fer_svm_forward with the hinge epilogue on X fp32 [N, F], W [P, F], bias [P], labels int64 [N], classes
    int64 [P], Cp, Cn [P]: (R [N, P] residual c a s m, Dw [N, P] curvature weights c a, loss [P] = sum c a m^2,
    Z [N, P] = X W^T + bias or None)."""
    return _svm_forward(X, W, bias, 0, labels, classes, Cp, Cn, None, want_z)


def svm_scale(X, V, vbias, Dw):
    """fer_svm_forward with the scale epilogue: Dw * (X V^T + vbias) [N, P], the inner half of a Hessian-vector
    product."""
    return _svm_forward(X, V, vbias, 1, None, None, None, None, Dw, False)[0]


def svm_decision(X, W, bias):
    """Z = X W^T + bias [N, P] alone (the scale epilogue with zero weights; its product is dropped)."""
    Dw = torch.zeros(X.shape[0], W.shape[0], dtype=torch.float32, device=X.device)
    return _svm_forward(X, W, bias, 1, None, None, None, None, Dw, True)[3]


def svm_xtr(X, R):
    """fer_svm_xtr: (G [P, F] = R^T X, gb [P] = column sums of R), in the fixed slab order."""
    N, F, ldx = _svm_x(X, "svm_xtr")
    if R.dim() != 2 or not 1 <= R.shape[1] <= SVM_COLUMNS:
        raise ValueError(f"svm_xtr: R must be [N, P] with 1 <= P <= {SVM_COLUMNS}")
    P = R.shape[1]
    _svm_cols("svm_xtr: R", R, X, N, P)
    G = torch.empty(P, F, dtype=torch.float32, device=X.device)
    gb = torch.empty(P, dtype=torch.float32, device=X.device)
    check(lib().fer_svm_xtr(X.data_ptr(), ldx, R.data_ptr(), P, N, F, P, G.data_ptr(), F, gb.data_ptr(),
                            *_ws(lib().fer_svm_ws(N, F), X.device), stream()), "svm_xtr")
    return G, gb


# ------------------------------------------------------------------ misc
def colsum(x, out, accumulate=False, scale=None):
    M, N = x.shape
    check(lib().fer_colsum(dcode(x), x.data_ptr(), x.stride(0), M, N, out.data_ptr(), int(accumulate), ptr(scale),
                           *_ws(lib().fer_colsum_ws(M, N), x.device), stream()), "colsum")
    return out


def im2col_patch(x, P, dtype):
    B, Cc, Hh, Ww = x.shape
    n = (Hh // P) * (Ww // P)
    K = Cc * P * P
    cols = torch.empty(B * n, K, dtype=dtype, device=x.device)
    check(lib().fer_im2col_patch(dcode(cols), x.data_ptr(), B, Cc, Hh, Ww, P, cols.data_ptr(), K, stream()),
          "im2col")
    return cols


def tokens_fwd(emb, cls, pos, B, n, D, dropout=0.0, seed=0):
    t = torch.empty(B * (n + 1), D, dtype=emb.dtype, device=emb.device)
    check(lib().fer_tokens_fwd(dcode(emb), emb.data_ptr(), cls.data_ptr(), pos.data_ptr(), t.data_ptr(), B, n, D,
                               *_drop(dropout, seed), stream()), "tokens_fwd")
    return t


def tokens_bwd(dt, B, n, D, dcls, dpos, accumulate, dropout=0.0, seed=0, want_demb=True):
    demb = torch.empty(B * n, D, dtype=dt.dtype, device=dt.device) if want_demb else None
    check(lib().fer_tokens_bwd(dcode(dt), dt.data_ptr(), ptr(demb), ptr(dcls), ptr(dpos), int(accumulate), B, n, D,
                               *_drop(dropout, seed), *_ws(lib().fer_tokens_bwd_ws(B, n + 1, D), dt.device), stream()),
          "tokens_bwd")
    return demb


def head_fwd(t, N, lnw, lnb, eps, W, b, B, dropout=0.0, seed=0):
    D = t.shape[1]
    C = W.shape[0]
    logits = torch.empty(B, C, dtype=torch.float32, device=t.device)
    stats = torch.empty(B, 2, dtype=torch.float32, device=t.device)
    check(lib().fer_head_fwd(dcode(t), t.data_ptr(), N * t.stride(0), lnw.data_ptr(), lnb.data_ptr(), eps,
                             W.data_ptr(), b.data_ptr(), logits.data_ptr(), stats.data_ptr(), B, D, C,
                             *_drop(dropout, seed), stream()), "head_fwd")
    return logits, stats


def head_bwd(t, N, lnw, lnb, W, stats, dlogits, B, grads, accumulate, dropout=0.0, seed=0):
    D = t.shape[1]
    C = W.shape[0]
    dt = torch.empty_like(t)
    g_lnw, g_lnb, g_W, g_b = grads
    check(lib().fer_head_bwd(dcode(t), t.data_ptr(), N * t.stride(0), lnw.data_ptr(), lnb.data_ptr(), W.data_ptr(),
                             stats.data_ptr(), dlogits.data_ptr(), dt.data_ptr(), 1, t.shape[0], t.stride(0),
                             ptr(g_lnw), ptr(g_lnb), ptr(g_W), ptr(g_b), int(accumulate), B, D, C,
                             *_drop(dropout, seed), *_ws(lib().fer_head_bwd_ws(B, D, C), t.device), stream()),
          "head_bwd")
    return dt


def cross_entropy(logits, labels, weight=None, label_smoothing=0.0, grad_scale=1.0, want_grad=True):
    B, Cc = logits.shape
    loss = torch.empty((), dtype=torch.float32, device=logits.device)
    dl = torch.empty_like(logits) if want_grad else None
    check(lib().fer_cross_entropy(logits.data_ptr(), labels.data_ptr(), ptr(weight), B, Cc, label_smoothing,
                                  grad_scale, loss.data_ptr(), ptr(dl), stream()), "cross_entropy")
    return loss, dl


MIXUP_MAX_B = 2048  # include/fervit.h fer_mixup_draw


def mixup_draw(alpha: float, B: int, seed: int, lam: torch.Tensor, perm: torch.Tensor, n_sets: int = 1):
    """lam [n_sets] fp32 ~ Beta(alpha, alpha) (1 for alpha <= 0) and perm [n_sets * B] int32, drawn on the
    device from `seed` mixed with the step counter (when one is registered) and the set index."""
    _dev(lam)
    if lam.dtype != torch.float32 or perm.dtype != torch.int32 or not (lam.is_contiguous() and perm.is_contiguous()):
        raise TypeError("mixup_draw: lam is contiguous fp32, perm contiguous int32")
    if lam.numel() < n_sets or perm.numel() < n_sets * B:
        raise ValueError("mixup_draw: lam holds n_sets floats, perm n_sets * B indices")
    check(lib().fer_mixup_draw(float(alpha), B, seed64(seed), n_sets, lam.data_ptr(), perm.data_ptr(), stream()),
          "mixup_draw")
    return lam, perm


def mixup_apply(x: torch.Tensor, perm: torch.Tensor, lam: torch.Tensor, out: Optional[torch.Tensor] = None):
    """out[b] = lam * x[b] + (1 - lam) * x[perm[b]] over the rows of a contiguous fp32 batch x [B, ...]; lam is
    one device float. `out` must not overlap x."""
    _dev(x)
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise TypeError("mixup_apply: x is a contiguous fp32 batch")
    B = x.shape[0]
    if perm.dtype != torch.int32 or perm.numel() < B or lam.dtype != torch.float32 or lam.numel() < 1:
        raise TypeError("mixup_apply: perm holds B int32 indices, lam one fp32 value")
    out = _alloc(out, x)
    if out.shape != x.shape or out.dtype != x.dtype or not out.is_contiguous():
        raise TypeError("mixup_apply: out has x's shape, dtype and layout")
    check(lib().fer_mixup_apply(x.data_ptr(), perm.data_ptr(), lam.data_ptr(), out.data_ptr(), B,
                                x.numel() // max(B, 1), stream()), "mixup_apply")
    return out


def cross_entropy_mix(logits, labels, perm, lam, weight=None, label_smoothing=0.0, grad_scale=1.0, want_grad=True):
    """lam * CE(logits, labels) + (1 - lam) * CE(logits, labels[perm]) and its dlogits in one launch; perm
    (int32 [B], None: the identity) and lam (one fp32) are device tensors."""
    B, Cc = logits.shape
    if perm is not None and (perm.dtype != torch.int32 or perm.numel() < B):
        raise TypeError("cross_entropy_mix: perm holds B int32 indices")
    loss = torch.empty((), dtype=torch.float32, device=logits.device)
    dl = torch.empty_like(logits) if want_grad else None
    check(lib().fer_cross_entropy_mix(logits.data_ptr(), labels.data_ptr(), ptr(perm), lam.data_ptr(), ptr(weight), B,
                                      Cc, label_smoothing, grad_scale, loss.data_ptr(), ptr(dl), stream()),
          "cross_entropy_mix")
    return loss, dl


def cast_bf16(x, out=None):
    out = _alloc(out, x, dtype=torch.bfloat16)
    check(lib().fer_cast_f32_bf16(x.data_ptr(), out.data_ptr(), x.numel(), stream()), "cast")
    return out


def cast_f32(x, out=None):
    out = _alloc(out, x, dtype=torch.float32)
    check(lib().fer_cast_bf16_f32(x.data_ptr(), out.data_ptr(), x.numel(), stream()), "cast")
    return out


def axpy(x, t, scale_ptr, out=None):
    out = _alloc(out, x)
    check(lib().fer_axpy(dcode(x), x.data_ptr(), t.data_ptr(), scale_ptr.data_ptr(), out.data_ptr(), x.numel(),
                         stream()), "axpy")
    return out


def dot(a, b, out, accumulate=False):
    check(lib().fer_dot(dcode(a), a.data_ptr(), ptr(b), a.numel(), out.data_ptr(), int(accumulate),
                        *_ws(4 * 1024 + 64, a.device, slot=2), stream()), "dot")
    return out


def dropout(x, p, seed):
    out = torch.empty_like(x)
    check(lib().fer_dropout(dcode(x), x.data_ptr(), out.data_ptr(), x.numel(), *_drop(p, seed), stream()), "dropout")
    return out


# ------------------------------------------------------------------ LatentCNN operators (csrc/convbn.hip)
def _rows(t: torch.Tensor, what: str) -> None:
    _dev(t)
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"{what}: [rows, cols] tensors with unit column stride")


def conv1d_cols(x, B, L, out=None):
    """im2col of nn.Conv1d(k=3, padding=1): x [B*L, C] -> cols [B*L, 3*C] in (cin, k) column order."""
    _rows(x, "conv1d_cols")
    M, Cc = x.shape
    if M != B * L:
        raise ValueError("conv1d_cols: x must have B*L rows")
    out = _alloc(out, x, (M, 3 * Cc))
    check(lib().fer_conv1d_cols(dcode(x), x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0), B, L, Cc,
                                stream()), "conv1d_cols")
    return out


def conv1d_cols_bwd(dcols, B, L, out=None, res=None):
    """dx [B*L, C] from dcols [B*L, 3*C] (the adjoint of conv1d_cols), plus `res` [B*L, C] when given."""
    _rows(dcols, "conv1d_cols_bwd")
    M, K = dcols.shape
    if M != B * L or K % 3:
        raise ValueError("conv1d_cols_bwd: dcols must be [B*L, 3*C]")
    out = _alloc(out, dcols, (M, K // 3))
    check(lib().fer_conv1d_cols_bwd(dcode(dcols), dcols.data_ptr(), dcols.stride(0), *_row(res, K // 3),
                                    out.data_ptr(), out.stride(0), B, L, K // 3, stream()), "conv1d_cols_bwd")
    return out


def batchnorm_fwd(x, gamma, beta, running_mean, running_var, num_batches_tracked, train, momentum=0.1, eps=1e-5,
                  res=None, relu=False, dropout=0.0, seed=0, out=None, mean=None, rstd=None):
    """y = dropout(relu?(BatchNorm(x) (+ res))) over the rows of x [M, C]; train: batch statistics and the
    running-statistic update on the device, else the running statistics. Returns (y, mean, rstd)."""
    _rows(x, "batchnorm_fwd")
    M, Cc = x.shape
    if train and M < 2:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
    out = _alloc(out, x)
    mean = _alloc(mean, x, (Cc,), torch.float32)
    rstd = _alloc(rstd, x, (Cc,), torch.float32)
    check(lib().fer_batchnorm_fwd(dcode(x), x.data_ptr(), x.stride(0), gamma.data_ptr(), beta.data_ptr(),
                                  ptr(running_mean), ptr(running_var), ptr(num_batches_tracked), int(bool(train)),
                                  momentum, eps, *_row(res, Cc), int(bool(relu)), *_drop(dropout, seed),
                                  out.data_ptr(), out.stride(0), mean.data_ptr(), rstd.data_ptr(), M, Cc, stream()),
          "batchnorm_fwd")
    return out, mean, rstd


def batchnorm_bwd(dy, x, mean, rstd, gamma, beta, train, res=None, relu=False, dropout=0.0, seed=0, dx=None,
                  dres=None, dgamma=None, dbeta=None, accumulate=False):
    """(dx, dres) of batchnorm_fwd; dgamma / dbeta (fp32 [C], optional) receive or accumulate the parameter
    gradients. dres: pass a tensor to receive the gated gradient of the residual branch."""
    _rows(x, "batchnorm_bwd")
    M, Cc = x.shape
    dx = _alloc(dx, x)
    check(lib().fer_batchnorm_bwd(dcode(x), dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), mean.data_ptr(),
                                  rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), *_row(res, Cc), int(bool(relu)),
                                  *_drop(dropout, seed), int(bool(train)), *_row(dx, Cc), *_row(dres, Cc),
                                  ptr(dgamma), ptr(dbeta), int(accumulate), M, Cc, stream()), "batchnorm_bwd")
    return dx, dres


def seq_mean_fwd(x, B, L, out=None):
    """[B*L, C] -> [B, C], the mean over the L rows of each sample."""
    _rows(x, "seq_mean_fwd")
    if x.shape[0] != B * L:
        raise ValueError("seq_mean_fwd: x must have B*L rows")
    Cc = x.shape[1]
    out = _alloc(out, x, (B, Cc))
    check(lib().fer_seq_mean_fwd(dcode(x), x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0), B, L, Cc,
                                 stream()), "seq_mean_fwd")
    return out


def seq_mean_bwd(dy, B, L, out=None):
    _rows(dy, "seq_mean_bwd")
    if dy.shape[0] != B:
        raise ValueError("seq_mean_bwd: dy must have B rows")
    Cc = dy.shape[1]
    out = _alloc(out, dy, (B * L, Cc))
    check(lib().fer_seq_mean_bwd(dcode(dy), dy.data_ptr(), dy.stride(0), out.data_ptr(), out.stride(0), B, L, Cc,
                                 stream()), "seq_mean_bwd")
    return out


def logits_fwd(x, W, bias=None, out=None):
    """fp32 logits [B, C] = x [B, D] W^T + bias for a small C (W [C, D], bias fp32)."""
    _rows(x, "logits_fwd")
    B, D = x.shape
    Cc = W.shape[0]
    out = _alloc(out, x, (B, Cc), torch.float32)
    check(lib().fer_logits_fwd(dcode(x), x.data_ptr(), x.stride(0), W.data_ptr(), ptr(bias), out.data_ptr(), B, D, Cc,
                               stream()), "logits_fwd")
    return out


def logits_bwd(x, W, dlogits, gate=None, dx=None, dW=None, dbias=None, accumulate=False, want_dx=True):
    """dx [B, D] (x's dtype, times `gate` when given); dW / dbias (fp32, optional) receive or accumulate."""
    _rows(x, "logits_bwd")
    B, D = x.shape
    Cc = W.shape[0]
    if dx is None and want_dx:
        dx = torch.empty_like(x)
    check(lib().fer_logits_bwd(dcode(x), x.data_ptr(), x.stride(0), W.data_ptr(), dlogits.data_ptr(), *_row(gate, D),
                               *_row(dx, D), ptr(dW), ptr(dbias), int(accumulate), B, D, Cc, stream()), "logits_bwd")
    return dx


# ------------------------------------------------------------------ LatentCNNDeep operators (csrc/attnpool.hip)
def attnpool_fwd(x, w, bias, B, L, out=None, probs=None, want_probs=True):
    """Attention pooling [B*L, C] -> [B, C]: softmax over each sample's L scores x w + bias, then the
    weighted sum of its rows. w fp32 [C] (any shape with C elements), bias fp32 with one element or None.
    Returns (y, probs): probs fp32 [B*L] for attnpool_bwd, None when want_probs is false."""
    _rows(x, "attnpool_fwd")
    if x.shape[0] != B * L:
        raise ValueError("attnpool_fwd: x must have B*L rows")
    Cc = x.shape[1]
    if w.dtype != torch.float32 or w.numel() != Cc or not w.is_contiguous():
        raise ValueError("attnpool_fwd: w must be a contiguous fp32 tensor of C elements")
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() != 1):
        raise ValueError("attnpool_fwd: bias must be one fp32 value")
    out = _alloc(out, x, (B, Cc))
    if probs is None and want_probs:
        probs = torch.empty(B * L, dtype=torch.float32, device=x.device)
    check(lib().fer_attnpool_fwd(dcode(x), x.data_ptr(), x.stride(0), w.data_ptr(), ptr(bias), out.data_ptr(),
                                 out.stride(0), ptr(probs), B, L, Cc, stream()), "attnpool_fwd")
    return out, probs


def attnpool_bwd(dy, x, w, probs, B, L, dx=None, dw=None, dbias=None, accumulate=False, want_dx=True):
    """dx [B*L, C] of attnpool_fwd; dw (fp32, C elements) / dbias (fp32, one element), optional, receive
    or accumulate the parameter gradients: the kernel writes per-sample partials, which are added over B
    in a fixed order, dw by colsum, the single dbias column (below colsum's 4-column pieces) by dot with
    a vector of ones."""
    _rows(x, "attnpool_bwd")
    _rows(dy, "attnpool_bwd")
    if x.shape[0] != B * L or dy.shape[0] != B or dy.shape[1] != x.shape[1]:
        raise ValueError("attnpool_bwd: x must be [B*L, C] and dy [B, C]")
    Cc = x.shape[1]
    if dx is None and want_dx:
        dx = torch.empty_like(x)
    f32 = torch.float32
    dw_part = torch.empty(B, Cc, dtype=f32, device=x.device) if dw is not None else None
    db_part = torch.empty(B, dtype=f32, device=x.device) if dbias is not None else None
    if dw is not None and (dw.dtype != f32 or dw.numel() != Cc or not dw.is_contiguous()):
        raise ValueError("attnpool_bwd: dw must be a contiguous fp32 tensor of C elements")
    if dbias is not None and (dbias.dtype != f32 or dbias.numel() != 1):
        raise ValueError("attnpool_bwd: dbias must be one fp32 value")
    check(lib().fer_attnpool_bwd(dcode(x), dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), w.data_ptr(),
                                 probs.data_ptr(), *_row(dx, Cc), ptr(dw_part), ptr(db_part), B, L, Cc, stream()),
          "attnpool_bwd")
    if dw is not None:
        colsum(dw_part, dw, accumulate=accumulate)
    if dbias is not None:
        dot(db_part, _ones(B, x.device), dbias, accumulate=accumulate)
    return dx


_ONES = {}


def _ones(n: int, device) -> torch.Tensor:
    t = _ONES.get((device, n))
    if t is None:
        t = _ONES[(device, n)] = torch.ones(n, dtype=torch.float32, device=device)
    return t


def relu_dropout_fwd(x, dropout=0.0, seed=0, out=None):
    """y = dropout(relu(x)) over [M, C]; the mask is a function of (seed, element index)."""
    _rows(x, "relu_dropout_fwd")
    M, Cc = x.shape
    out = _alloc(out, x)
    check(lib().fer_relu_dropout_fwd(dcode(x), x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0), M, Cc,
                                     *_drop(dropout, seed), stream()), "relu_dropout_fwd")
    return out


def relu_dropout_bwd(dy, x, dropout=0.0, seed=0, out=None):
    """dx = dy * [x > 0] * keep / (1 - p), gate and mask recomputed from the forward's x and seed."""
    _rows(x, "relu_dropout_bwd")
    _rows(dy, "relu_dropout_bwd")
    if dy.shape != x.shape:
        raise ValueError("relu_dropout_bwd: dy and x must have the same shape")
    M, Cc = x.shape
    out = _alloc(out, x)
    check(lib().fer_relu_dropout_bwd(dcode(x), dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0),
                                     out.data_ptr(), out.stride(0), M, Cc, *_drop(dropout, seed), stream()),
          "relu_dropout_bwd")
    return out


# ------------------------------------------------------------------ LatentCNN2D operators (csrc/conv2d.hip)
def _pixels(t: torch.Tensor, B: int, H: int, W: int, what: str) -> None:
    _rows(t, what)
    if t.shape[0] != B * H * W:
        raise ValueError(f"{what}: the operand must have B*H*W rows")


def conv2d_cols(x, B, H, W, out=None):
    """im2col of nn.Conv2d(3x3, padding=1): x [B*H*W, C] -> cols [B*H*W, 9*C] in (cin, kh, kw) column order."""
    _pixels(x, B, H, W, "conv2d_cols")
    M, Cc = x.shape
    out = _alloc(out, x, (M, 9 * Cc))
    check(lib().fer_conv2d_cols(dcode(x), x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0), B, H, W, Cc,
                                stream()), "conv2d_cols")
    return out


def conv2d_cols_bwd(dcols, B, H, W, out=None):
    """dx [B*H*W, C] from dcols [B*H*W, 9*C], the adjoint of conv2d_cols."""
    _pixels(dcols, B, H, W, "conv2d_cols_bwd")
    M, K = dcols.shape
    if K % 9:
        raise ValueError("conv2d_cols_bwd: dcols must be [B*H*W, 9*C]")
    out = _alloc(out, dcols, (M, K // 9))
    check(lib().fer_conv2d_cols_bwd(dcode(dcols), dcols.data_ptr(), dcols.stride(0), out.data_ptr(), out.stride(0),
                                    B, H, W, K // 9, stream()), "conv2d_cols_bwd")
    return out


def _c1_weight(w, what: str) -> int:
    if w.dtype != torch.float32 or not w.is_contiguous() or w.numel() % 9:
        raise ValueError(f"{what}: w must be a contiguous fp32 tensor of Cout*9 elements")
    return w.numel() // 9


def conv2d_c1_fwd(x, w, bias, B, H, W, out=None):
    """nn.Conv2d(1, Cout, 3, padding=1): x with B*H*W elements (the image as it lies, contiguous) ->
    y [B*H*W, Cout] in x's dtype; w fp32 [Cout, 1, 3, 3], bias fp32 [Cout] or None."""
    _dev(x)
    Cout = _c1_weight(w, "conv2d_c1_fwd")
    if x.numel() != B * H * W or not x.is_contiguous():
        raise ValueError("conv2d_c1_fwd: x must be contiguous with B*H*W elements")
    out = _alloc(out, x, (B * H * W, Cout))
    check(lib().fer_conv2d_c1_fwd(dcode(x), x.data_ptr(), 1, w.data_ptr(), ptr(bias), out.data_ptr(), out.stride(0),
                                  B, H, W, Cout, stream()), "conv2d_c1_fwd")
    return out


def conv2d_c1_parts(M: int) -> int:
    """Workgroups (= partial rows) of the first layer's weight gradient: strips of at least 256 pixels."""
    return max(1, min(1024, M // 256))


def conv2d_c1_bwd(dy, x, w, B, H, W, dw=None, accumulate=False, want_dx=False):
    """Backward of conv2d_c1_fwd: dw (fp32, Cout*9 elements, optional) receives or accumulates the weight
    gradient (per-workgroup partials added in a fixed order by colsum); returns dx (x's shape) or None."""
    _pixels(dy, B, H, W, "conv2d_c1_bwd")
    Cout = _c1_weight(w, "conv2d_c1_bwd")
    M = B * H * W
    if dy.shape[1] != Cout or x.numel() != M or not x.is_contiguous():
        raise ValueError("conv2d_c1_bwd: dy must be [B*H*W, Cout] and x contiguous with B*H*W elements")
    if dw is not None and (dw.dtype != torch.float32 or dw.numel() != Cout * 9 or not dw.is_contiguous()):
        raise ValueError("conv2d_c1_bwd: dw must be a contiguous fp32 tensor of Cout*9 elements")
    n_parts = conv2d_c1_parts(M)
    part = torch.empty(n_parts, Cout * 9, dtype=torch.float32, device=dy.device) if dw is not None else None
    dx = torch.empty_like(x) if want_dx else None
    if part is None and dx is None:
        return None
    check(lib().fer_conv2d_c1_bwd(dcode(dy), dy.data_ptr(), dy.stride(0), x.data_ptr(), 1, w.data_ptr(), ptr(part),
                                  n_parts, ptr(dx), 1, B, H, W, Cout, stream()), "conv2d_c1_bwd")
    if dw is not None:
        colsum(part, dw, accumulate=accumulate)
    return dx


def pool2_chdrop_fwd(x, B, H, W, pool, dropout=0.0, seed=0, out=None):
    """MaxPool2d((2, 2)) (pool) then Dropout2d over x [B*H*W, C] -> [B*(H//2)*(W//2), C] (or x's shape)."""
    _pixels(x, B, H, W, "pool2_chdrop_fwd")
    Cc = x.shape[1]
    Mo = B * (H // 2) * (W // 2) if pool else B * H * W
    out = _alloc(out, x, (Mo, Cc))
    check(lib().fer_pool2_chdrop_fwd(dcode(x), x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0), B, H, W, Cc,
                                     int(bool(pool)), *_drop(dropout, seed), stream()), "pool2_chdrop_fwd")
    return out


def pool2_chdrop_bwd(dy, x, B, H, W, pool, dropout=0.0, seed=0, out=None):
    """dx [B*H*W, C]: dy * keep / (1 - p) at each window's argmax (recomputed from the forward's x), 0 elsewhere."""
    _pixels(x, B, H, W, "pool2_chdrop_bwd")
    _rows(dy, "pool2_chdrop_bwd")
    Cc = x.shape[1]
    Mo = B * (H // 2) * (W // 2) if pool else B * H * W
    if tuple(dy.shape) != (Mo, Cc):
        raise ValueError("pool2_chdrop_bwd: dy must have the forward output's shape")
    out = _alloc(out, x)
    check(lib().fer_pool2_chdrop_bwd(dcode(x), dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), out.data_ptr(),
                                     out.stride(0), B, H, W, Cc, int(bool(pool)), *_drop(dropout, seed), stream()),
          "pool2_chdrop_bwd")
    return out


# ------------------------------------------------------------------ AFS style extractor (csrc/grouped.hip)
def _grp(t: torch.Tensor, what: str):
    """(ld, gs) of a grouped operand [G, rows, cols]: any row / group stride, unit column stride. A
    [B, G, K] tensor is the operand `t.transpose(0, 1)`, read or written in place."""
    _dev(t)
    if t.dim() != 3 or t.stride(2) != 1:
        raise ValueError(f"{what}: [G, rows, cols] tensors with unit column stride")
    return t.stride(1), (t.stride(0) if t.shape[0] > 1 else 0)


def _grp_vec(t: Optional[torch.Tensor], G: int, n: int, what: str, dtype=torch.float32) -> int:
    """Group stride of a per-group vector [G, n] (fp32 parameter, gradient or statistic)."""
    if t is None:
        return 0
    _dev(t)
    if t.dtype != dtype or t.dim() != 2 or t.shape != (G, n) or (n > 1 and t.stride(1) != 1):
        raise ValueError(f"{what}: a [G, {n}] {dtype} tensor with unit column stride")
    return t.stride(0) if G > 1 else 0


def _same_strides(ts, what: str):
    st = {_grp(t, what) for t in ts}
    if len(st) != 1 or len({t.dtype for t in ts}) != 1 or len({tuple(t.shape) for t in ts}) != 1:
        raise ValueError(f"{what}: the sets of one launch share shape, dtype and strides")
    return st.pop()


def _three(ts):
    return [ptr(ts[i]) if i < len(ts) else None for i in range(3)]


def grouped_linear_fwd(x, ws, bs=None, outs=None):
    """y_s[g] = x[g] w_s[g]^T + b_s[g] for 1-3 weight sets in one launch. x [G, M, K], w_s [G, N, K] (x's
    dtype), b_s [G, N] fp32 or None, y_s [G, M, N] (allocated contiguous unless given). Returns the list y."""
    if not 1 <= len(ws) <= 3:
        raise ValueError("grouped_linear_fwd: one to three weight sets")
    G, M, K = x.shape
    N = ws[0].shape[1]
    ldx, gsx = _grp(x, "grouped_linear_fwd")
    ldw, gsw = _same_strides(ws, "grouped_linear_fwd")
    if ws[0].shape != (G, N, K) or ws[0].dtype != x.dtype:
        raise ValueError("grouped_linear_fwd: w must be [G, N, K] in x's dtype")
    bs = [None] * len(ws) if bs is None else list(bs)
    if len(bs) != len(ws) or len({b is None for b in bs}) != 1:
        raise ValueError("grouped_linear_fwd: a bias for every set or for none")
    gsb = {_grp_vec(b, G, N, "grouped_linear_fwd bias") for b in bs}
    if len(gsb) != 1:
        raise ValueError("grouped_linear_fwd: the biases share one group stride")
    if outs is None:
        outs = [torch.empty(G, M, N, dtype=x.dtype, device=x.device) for _ in ws]
    ldy, gsy = _same_strides(outs, "grouped_linear_fwd")
    if len(outs) != len(ws) or outs[0].shape != (G, M, N) or outs[0].dtype != x.dtype:
        raise ValueError("grouped_linear_fwd: one [G, M, N] output per set, in x's dtype")
    check(lib().fer_grouped_linear_fwd(dcode(x), x.data_ptr(), ldx, gsx, *_three(ws), ldw, gsw, *_three(bs),
                                       gsb.pop(), *_three(outs), ldy, gsy, G, M, N, K, stream()),
          "grouped_linear_fwd")
    return outs


def grouped_linear_dgrad(dys, ws, out=None):
    """dx[g] = sum_s dy_s[g] w_s[g]: dy_s [G, M, N], w_s [G, N, K], dx [G, M, K]."""
    if not 1 <= len(ws) <= 3 or len(dys) != len(ws):
        raise ValueError("grouped_linear_dgrad: one to three weight sets, one gradient each")
    G, M, N = dys[0].shape
    K = ws[0].shape[2]
    lddy, gsdy = _same_strides(dys, "grouped_linear_dgrad")
    ldw, gsw = _same_strides(ws, "grouped_linear_dgrad")
    if ws[0].shape != (G, N, K) or ws[0].dtype != dys[0].dtype:
        raise ValueError("grouped_linear_dgrad: w must be [G, N, K] in dy's dtype")
    out = _alloc(out, dys[0], (G, M, K))
    lddx, gsdx = _grp(out, "grouped_linear_dgrad")
    if out.shape != (G, M, K) or out.dtype != dys[0].dtype:
        raise ValueError("grouped_linear_dgrad: dx must be [G, M, K] in dy's dtype")
    check(lib().fer_grouped_linear_dgrad(dcode(out), *_three(dys), lddy, gsdy, *_three(ws), ldw, gsw, out.data_ptr(),
                                         lddx, gsdx, G, M, N, K, stream()), "grouped_linear_dgrad")
    return out


def grouped_linear_wgrad(dys, x, dws=None, dbs=None, accumulate=False, skip_mask=0):
    """dw_s[g] (+)= dy_s[g]^T x[g] ([G, N, K] fp32), db_s[g] (+)= column sums of dy_s[g] ([G, N] fp32) in one
    launch; an entry of dws / dbs may be None. skip_mask: bit g = leave group g's outputs untouched."""
    if not 1 <= len(dys) <= 3:
        raise ValueError("grouped_linear_wgrad: one to three gradient sets")
    G, M, N = dys[0].shape
    K = x.shape[2]
    lddy, gsdy = _same_strides(dys, "grouped_linear_wgrad")
    ldx, gsx = _grp(x, "grouped_linear_wgrad")
    if x.shape != (G, M, K) or x.dtype != dys[0].dtype:
        raise ValueError("grouped_linear_wgrad: x must be [G, M, K] in dy's dtype")
    dws = [None] * len(dys) if dws is None else list(dws)
    dbs = [None] * len(dys) if dbs is None else list(dbs)
    if len(dws) != len(dys) or len(dbs) != len(dys):
        raise ValueError("grouped_linear_wgrad: one dw / db entry per gradient set")
    have = [w for w in dws if w is not None]
    lddw, gsdw = _same_strides(have, "grouped_linear_wgrad dw") if have else (K, 0)
    if have and (have[0].shape != (G, N, K) or have[0].dtype != torch.float32):
        raise ValueError("grouped_linear_wgrad: dw must be [G, N, K] fp32")
    gsdb = {_grp_vec(b, G, N, "grouped_linear_wgrad db") for b in dbs if b is not None}
    if len(gsdb) > 1:
        raise ValueError("grouped_linear_wgrad: the bias gradients share one group stride")
    check(lib().fer_grouped_linear_wgrad(dcode(x), *_three(dys), lddy, gsdy, x.data_ptr(), ldx, gsx, *_three(dws),
                                         lddw, gsdw, *_three(dbs), gsdb.pop() if gsdb else 0, int(accumulate),
                                         int(skip_mask), G, M, N, K, stream()), "grouped_linear_wgrad")


HIGHWAY_ACT = {"lrelu": 0, "relu": 1}


def highway_fwd(pn, pl, pg, gamma, beta, running_mean, running_var, num_batches_tracked, train, momentum=0.1,
                eps=1e-5, act="lrelu", out=None, want_stats=True):
    """y = s n + (1 - s) pl, s = sigmoid(pg), n = act(BatchNorm(pn)) over [G, B, C] pre-activations; gamma, beta,
    running_mean, running_var [G, C] fp32, num_batches_tracked [G] int64 (any group strides). train: batch
    statistics and the running-statistic update on the device. Returns (y, mean, rstd), statistics [G, C]."""
    G, B, Cc = pn.shape
    ldp, gsp = _same_strides([pn, pl, pg], "highway_fwd")
    if train and B < 2:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {(B, Cc)}")
    gs_par = {_grp_vec(gamma, G, Cc, "highway_fwd gamma"), _grp_vec(beta, G, Cc, "highway_fwd beta")}
    gs_stat = {_grp_vec(running_mean, G, Cc, "highway_fwd running_mean"),
               _grp_vec(running_var, G, Cc, "highway_fwd running_var")}
    if len(gs_par) != 1 or len(gs_stat) != 1:
        raise ValueError("highway_fwd: gamma / beta and running_mean / running_var share their group strides")
    nbt = num_batches_tracked
    gs_nbt = 0 if nbt is None else _grp_vec(nbt.view(G, 1), G, 1, "highway_fwd num_batches_tracked", torch.int64)
    out = _alloc(out, pn)
    ldy, gsy = _grp(out, "highway_fwd")
    if out.shape != pn.shape or out.dtype != pn.dtype:
        raise ValueError("highway_fwd: y must match pn")
    mean = rstd = None
    if want_stats:
        mean = torch.empty(G, Cc, dtype=torch.float32, device=pn.device)
        rstd = torch.empty_like(mean)
    check(lib().fer_highway_fwd(dcode(pn), pn.data_ptr(), pl.data_ptr(), pg.data_ptr(), ldp, gsp, gamma.data_ptr(),
                                beta.data_ptr(), gs_par.pop(), ptr(running_mean), ptr(running_var), gs_stat.pop(),
                                ptr(nbt), gs_nbt, int(bool(train)), momentum, eps, HIGHWAY_ACT[act], out.data_ptr(),
                                ldy, gsy, ptr(mean), ptr(rstd), G, B, Cc, stream()), "highway_fwd")
    return out, mean, rstd


def highway_bwd(dy, pn, pl, pg, mean, rstd, gamma, beta, train, act="lrelu", dgamma=None, dbeta=None,
                accumulate=False, skip_mask=0):
    """(dpn, dpl, dpg) of highway_fwd from dy [G, B, C] and the saved pre-activations and statistics;
    dgamma / dbeta ([G, C] fp32 at gamma's group stride, optional) receive or accumulate."""
    G, B, Cc = pn.shape
    ldp, gsp = _same_strides([pn, pl, pg], "highway_bwd")
    lddy, gsdy = _grp(dy, "highway_bwd")
    if dy.shape != pn.shape or dy.dtype != pn.dtype:
        raise ValueError("highway_bwd: dy must match pn")
    gs_par = {_grp_vec(t, G, Cc, "highway_bwd parameters") for t in (gamma, beta, dgamma, dbeta) if t is not None}
    if len(gs_par) != 1:
        raise ValueError("highway_bwd: gamma, beta, dgamma, dbeta share one group stride")
    if not (mean.is_contiguous() and rstd.is_contiguous() and mean.shape == (G, Cc) and rstd.shape == (G, Cc)):
        raise ValueError("highway_bwd: mean, rstd are the contiguous [G, C] statistics of highway_fwd")
    dp = [torch.empty(G, B, Cc, dtype=pn.dtype, device=pn.device) for _ in range(3)]
    check(lib().fer_highway_bwd(dcode(pn), dy.data_ptr(), lddy, gsdy, pn.data_ptr(), pl.data_ptr(), pg.data_ptr(), ldp,
                                gsp, mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), gs_par.pop(),
                                int(bool(train)), HIGHWAY_ACT[act], dp[0].data_ptr(), dp[1].data_ptr(),
                                dp[2].data_ptr(), Cc, B * Cc if G > 1 else 0, ptr(dgamma), ptr(dbeta),
                                int(accumulate), int(skip_mask), G, B, Cc, stream()), "highway_bwd")
    return dp


# ------------------------------------------------------------------ low-latency inference (csrc/skinny.hip)
def skinny_linear(x, w, bias=None, *, act="none", ln_a=None, res=None, ln_res=None, out=None):
    """One fer_skinny_linear launch for M <= 64 bf16 rows: out = act(x' w^T + bias) + res', with
    x' = x or LayerNorm(x) (ln_a = (gamma, beta, eps), normalised on load) and res' = nothing, res or
    LayerNorm(res) (ln_res = (gamma, beta, eps), added in fp32). x [M, K], w [N, K], res / out [M, N] bf16 with
    unit column stride; bias, gamma, beta fp32. act: "none", "relu" or "gelu". The library checks the contract
    (M, multiples of 8, strides, alignment) and the call raises FerError on a violation."""
    _dev(x)
    if act not in ("none", "relu", "gelu"):
        raise ValueError(f"skinny_linear: unknown activation {act!r}")
    M, K = x.shape
    N = w.shape[0]
    for name, t in (("x", x), ("w", w), ("res", res), ("out", out)):
        if t is not None and (t.dtype != torch.bfloat16 or t.dim() != 2 or t.stride(1) != 1):
            raise TypeError(f"skinny_linear: {name} must be a bf16 [rows, cols] tensor with unit column stride")
    for name, t in (("bias", bias), *((n, t) for ln, n in ((ln_a, "ln_a"), (ln_res, "ln_res")) if ln for t in ln[:2])):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise TypeError(f"skinny_linear: {name} must be contiguous fp32")
    if w.shape[1] != K or (res is not None and tuple(res.shape) != (M, N)) or (ln_res is not None and res is None):
        raise ValueError("skinny_linear: x [M, K], w [N, K], res [M, N]; ln_res needs res")
    out = _alloc(out, x, (M, N))
    if tuple(out.shape) != (M, N):
        raise ValueError("skinny_linear: out must be [M, N]")
    ga, ba, ea = (ln_a[0], ln_a[1], float(ln_a[2])) if ln_a else (None, None, 0.0)
    gr, br, er = (ln_res[0], ln_res[1], float(ln_res[2])) if ln_res else (None, None, 0.0)
    check(lib().fer_skinny_linear(x.data_ptr(), x.stride(0), w.data_ptr(), w.stride(0), ptr(bias), ACT[act], ptr(ga),
                                  ptr(ba), ea, *_row(res, N), ptr(gr), ptr(br), er, out.data_ptr(), out.stride(0),
                                  M, N, K, stream()), "skinny_linear")
    return out


def skinny_adapter(x, w1, b1, w2, b2, alpha, out=None):
    """One fer_skinny_adapter launch for M <= 64 bf16 rows: out = x + alpha * (GELU(x w1^T + b1) w2^T + b2).
    x / out [M, D], w1 [R, D], w2 [D, R] bf16 with unit column stride; b1 [R], b2 [D] contiguous fp32; alpha a
    one-element fp32 device tensor, read by the kernel (never copied to the host). out must not overlap x. The
    library checks the contract (M, D, R, strides, alignment, overlap) and the call raises FerError on a
    violation."""
    _dev(x)
    M, D = x.shape
    R = w1.shape[0]
    for name, t in (("x", x), ("w1", w1), ("w2", w2), ("out", out)):
        if t is not None and (t.dtype != torch.bfloat16 or t.dim() != 2 or t.stride(1) != 1):
            raise TypeError(f"skinny_adapter: {name} must be a bf16 [rows, cols] tensor with unit column stride")
    for name, t in (("b1", b1), ("b2", b2), ("alpha", alpha)):
        if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda:
            raise TypeError(f"skinny_adapter: {name} must be a contiguous fp32 device tensor")
    if (tuple(w1.shape) != (R, D) or tuple(w2.shape) != (D, R) or b1.numel() != R or b2.numel() != D
            or alpha.numel() != 1):
        raise ValueError("skinny_adapter: x [M, D], w1 [R, D], b1 [R], w2 [D, R], b2 [D], alpha [1]")
    out = _alloc(out, x, (M, D))
    if tuple(out.shape) != (M, D):
        raise ValueError("skinny_adapter: out must be [M, D]")
    check(lib().fer_skinny_adapter(x.data_ptr(), x.stride(0), w1.data_ptr(), w1.stride(0), b1.data_ptr(),
                                   w2.data_ptr(), w2.stride(0), b2.data_ptr(), alpha.data_ptr(), out.data_ptr(),
                                   out.stride(0), M, D, R, stream()), "skinny_adapter")
    return out
