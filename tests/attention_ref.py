"""Float64 reference and element-wise error model of the attention core, shared by
tests/test_gpu_attention_elementwise.py (the HIP kernels) and tests/test_attention_bound_cpu.py (a torch
emulation of the bf16 path and its mutants, which shows the model sound and sharp without a GPU).

Layout here is [B][H][N][dh] float64; `keep` is [B][H][N][N] bool or None. P is the exact softmax,
Pd = P * keep * drop_scale. Every bound is  out_round |ref| + inner S + c 2^-23 A + flush  with S, A sums of
reference magnitudes; `inner` is 2^-8 on the bf16 path (operands of the second MFMA rounded to bf16) and 0
on the fp32 path."""
import math

import numpy as np
import torch

from dropmask import keep_mask, keep_mask_torch
from elemwise import BF_ROUND, U, assert_close, measure_c

# ex2 (csrc/attention.hip, `ex2`) flushes results below 2^-126 to 0 and a bf16 / fp32 store loses what lies
# below the format's normal range: an absolute term of 2^-126 times the sum the lost probability multiplies.
FLUSH = 2.0 ** -126
OUTPUTS = ("out", "lse", "dq", "dk", "dv", "colsum")


def f32(v):
    return float(np.float32(v))


def bf_round(t):
    return t.to(torch.bfloat16).to(torch.float32)


def drop_params(p):
    """(thresh, drop_scale as the fp32 the ABI carries)."""
    if p <= 0:
        return 0, 1.0
    return max(1, min(65535, int(round(p * 65536.0)))), f32(1.0 / (1.0 - p))


# ---------------------------------------------------------------------- inputs
def make_inputs(B, N, H, dh, style, seed, device="cpu"):
    """(qkv [B*N][3*H*dh], dout [B*N][H*dh]) float32 holding bf16-representable values.
    normal: standard normal. peaked: Q times 3 and one key per head with 4 times the norm, so single keys
    dominate rows. offset: a shared K component makes every score of a row move by about +-40 (sign
    alternating by query) and key 0 by -+60 against it: rows with one dominant key whose other
    probabilities flush to 0, rows whose key 0 flushes, and running maxima far from 0."""
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(B, H, N, dh, generator=g) for _ in range(3))
    do = torch.randn(B, H, N, dh, generator=g)
    if style == "peaked":
        q *= 3
        for h in range(H):
            k[:, h, (5 * h + 3) % N] *= 4
    elif style == "offset":
        sgn = torch.where(torch.arange(N) % 2 == 0, 1.0, -1.0)
        q[..., 0] = sgn * 40.0 * math.sqrt(dh)
        k[..., 0] = 1.0
        k[:, :, 0, 0] = -1.5
    else:
        assert style == "normal", style
    D = H * dh
    qkv = torch.stack([q, k, v]).permute(1, 3, 0, 2, 4).reshape(B * N, 3 * D)  # [B][N][3][H][dh]
    dout = do.permute(0, 2, 1, 3).reshape(B * N, D)
    return bf_round(qkv).to(device), bf_round(dout).to(device)


def split_heads(x, B, N, H, dh, parts=1):
    """[B*N][parts*H*dh] -> `parts` tensors [B][H][N][dh] (one: the tensor itself)."""
    t = x.reshape(B, N, parts, H, dh).permute(2, 0, 3, 1, 4)
    return t[0] if parts == 1 else tuple(t)


def merge_heads(*ts):
    """[B][H][N][dh] tensors -> [B*N][len(ts)*H*dh]."""
    B, H, N, dh = ts[0].shape
    return torch.stack(ts).permute(1, 3, 0, 2, 4).reshape(B * N, len(ts) * H * dh)


def attn_keep(seed, B, N, H, p, device="cpu"):
    """The kernels' keep mask: element index (bh*N + q)*NP + k, NP = N rounded up to even."""
    if p <= 0:
        return None
    shape = (B, H, N, N + (N & 1))
    if str(device).startswith("cuda"):
        return keep_mask_torch(seed, shape, p, device=device)[..., :N]
    return keep_mask(seed, shape, p)[..., :N]


# ---------------------------------------------------------------------- reference and scales
class Ref:
    """fp64 forward of one case and the scales of its bounds; `bwd(out_given)` adds the backward the kernel
    computes from its own inputs (delta from the `out` tensor the call is handed)."""

    def __init__(self, qkv, dout, B, N, H, dh, scale, keep, drop_scale):
        self.shape = (B, N, H, dh)
        self.scale, self.ds = float(scale), float(drop_scale)
        self.q, self.k, self.v = (t.double() for t in split_heads(qkv, B, N, H, dh, 3))
        self.do = split_heads(dout, B, N, H, dh).double()
        self.keepf = None if keep is None else keep.to(self.q.device).double() * self.ds
        s = (self.q @ self.k.transpose(-1, -2)) * self.scale
        self.lse = torch.logsumexp(s, -1)
        self.P = torch.exp(s - self.lse[..., None])
        self.Pd = self.P if self.keepf is None else self.P * self.keepf
        self.out = self.Pd @ self.v
        self.S_o = self.Pd @ self.v.abs()
        # |score| scale of a row: what one fp32 rounding of a score or of lse is relative to
        self.s_q = 1.0 + self.scale * (self.q.abs() @ self.k.abs().transpose(-1, -2)).amax(-1)
        self.f_o = FLUSH * (1.0 + self.ds * self.v.abs().sum(-2, keepdim=True)) * (self.S_o > 0)

    def bwd(self, out_given):
        B, N, H, dh = self.shape
        o = split_heads(out_given, B, N, H, dh).double().to(self.q.device)
        delta = (o * self.do).sum(-1, keepdim=True)
        dP = self.do @ self.v.transpose(-1, -2)
        if self.keepf is not None:
            dP = dP * self.keepf
        dS = self.P * (dP - delta)
        self.dv = self.Pd.transpose(-1, -2) @ self.do
        self.dq = (dS @ self.k) * self.scale
        self.dk = (dS.transpose(-1, -2) @ self.q) * self.scale
        self.S_v = self.Pd.transpose(-1, -2) @ self.do.abs()
        self.S_q = (dS.abs() @ self.k.abs()) * self.scale
        self.S_k = (dS.abs().transpose(-1, -2) @ self.q.abs()) * self.scale
        # fp32 magnitude inside dS: the cancellation in dP - delta, and the relative error of P from the
        # fp32 scores and lse (each one rounding of a number of size s_q)
        mag = dP.abs() + delta.abs()
        A = self.P * mag * self.s_q[..., None]
        self.A_q = (A @ self.k.abs()) * self.scale
        self.A_k = (A.transpose(-1, -2) @ self.q.abs()) * self.scale
        self.f_v = FLUSH * (1.0 + self.ds * self.do.abs().sum(-2, keepdim=True)) * (self.S_v > 0)
        self.f_q = FLUSH * (1.0 + self.scale * (mag @ self.k.abs()))
        self.f_k = FLUSH * (1.0 + self.scale * (mag.transpose(-1, -2) @ self.q.abs()))
        return self

    def grads(self):
        """[B*N][3*H*dh], the ABI's dqkv layout."""
        return merge_heads(self.dq, self.dk, self.dv)


def c_table(cases, label):
    """c per output from float32 torch on the CPU running the reference's formula on `cases`
    (a list of (B, N, H, dh, style, p)); never from a kernel. Printed as `c-measure attention <output> <label>`."""
    pairs = {o: [] for o in OUTPUTS}
    for i, (B, N, H, dh, style, p) in enumerate(cases):
        qkv, dout = make_inputs(B, N, H, dh, style, 9000 + i)
        _, ds = drop_params(p)
        scale = f32(1.0 / math.sqrt(dh))
        keep = attn_keep(31 + i, B, N, H, p)
        r = Ref(qkv, dout, B, N, H, dh, scale, keep, ds)
        q, k, v = split_heads(qkv, B, N, H, dh, 3)
        do = split_heads(dout, B, N, H, dh)
        kf = None if keep is None else keep.float() * ds
        s = (q @ k.transpose(-1, -2)) * scale
        lse = torch.logsumexp(s, -1)
        P = torch.exp(s - lse[..., None])
        Pd = P if kf is None else P * kf
        out = Pd @ v
        r.bwd(merge_heads(out))  # the fp32 path hands its own fp32 out to the backward
        delta = (out * do).sum(-1, keepdim=True)
        dP = do @ v.transpose(-1, -2)
        dP = dP if kf is None else dP * kf
        dS = P * (dP - delta)
        dv, dq, dk = Pd.transpose(-1, -2) @ do, (dS @ k) * scale, (dS.transpose(-1, -2) @ q) * scale
        pairs["out"].append((out, r.out, r.S_o, r.f_o))
        pairs["lse"].append((lse, r.lse, r.s_q))
        pairs["dq"].append((dq, r.dq, r.A_q, r.f_q))
        pairs["dk"].append((dk, r.dk, r.A_k, r.f_k))
        pairs["dv"].append((dv, r.dv, r.S_v, r.f_v))
        pairs["colsum"].append((merge_heads(dq, dk, dv).sum(0), r.grads().sum(0),
                                merge_heads(r.A_q, r.A_k, r.S_v).sum(0),
                                merge_heads(r.f_q, r.f_k, r.f_v.expand_as(r.S_v)).sum(0)))
    return {o: measure_c(f"attention {o}", label, pairs[o]) for o in OUTPUTS}


# ---------------------------------------------------------------------- the checks both modules run
def check_forward(name, r, out, lse, c, dtype, l_round=0.0, worst=None):
    """out [B*N][H*dh] and lse [B*H*N] of a forward against the reference `r`."""
    bf = dtype == "bf16"
    inner = BF_ROUND if bf else 0.0
    w = {}
    w["out"] = assert_close(f"{name} out", out, merge_heads(r.out), merge_heads(r.S_o), c["out"],
                            BF_ROUND if bf else 0.0, extra=merge_heads(inner * r.S_o + r.f_o))
    w["lse"] = assert_close(f"{name} lse", lse, r.lse.reshape(-1), r.s_q.reshape(-1), c["lse"], 0.0, extra=l_round)
    _note(worst, w)


def check_backward(name, r, dqkv, c, dtype, worst=None):
    """dqkv [B*N][3*H*dh] against r (r.bwd(out) done)."""
    bf = dtype == "bf16"
    inner = BF_ROUND if bf else 0.0
    got = split_heads(dqkv, *r.shape, 3)
    w = {}
    for key, g, ref, S, A, fl in (("dq", got[0], r.dq, r.S_q, r.A_q, r.f_q), ("dk", got[1], r.dk, r.S_k, r.A_k, r.f_k),
                                  ("dv", got[2], r.dv, r.S_v, r.S_v, r.f_v)):
        w[key] = assert_close(f"{name} {key}", g, ref, A, c[key], BF_ROUND if bf else 0.0, extra=inner * S + fl)
    _note(worst, w)


def check_colsum(name, r, colsum, old, c, dtype, sums_rounded, worst=None):
    """colsum [3*H*dh] fp32 against the column sums of the fp64 gradient: the column sums of the element
    bounds, with their store term 2^-8 |ref| only where the kernel sums the stored (rounded) values; `old`
    (tensor or None): what the colsum held under colsum_accumulate = 1."""
    bf = dtype == "bf16"
    inner = BF_ROUND if bf else 0.0
    g = r.grads()
    ref = g.sum(0)
    A = merge_heads(r.A_q, r.A_k, r.S_v).sum(0)
    extra = (inner * merge_heads(r.S_q, r.S_k, r.S_v) + merge_heads(r.f_q, r.f_k, r.f_v.expand_as(r.S_v))).sum(0)
    if bf and sums_rounded:
        extra = extra + BF_ROUND * g.abs().sum(0)
    if old is not None:
        old = old.double().to(ref.device)
        ref = ref + old
        A = A + old.abs()
    w = {"colsum": assert_close(f"{name} colsum", colsum, ref, A, c["colsum"], 0.0, extra=extra)}
    _note(worst, w)


def _note(worst, w):
    if worst is not None:
        for k, v in w.items():
            worst[k] = max(worst.get(k, 0.0), v)
