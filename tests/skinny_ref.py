"""float64 restatement of fer_skinny_linear (include/fervit.h) for tests/test_infer_cpu.py and
tests/test_gpu_skinny_linear.py, the float32 torch composition `c` is measured on, and the seeded operands
both files use.

    out = act(A' W^T + bias) + R'
    A' = A or LN(A; gamma_a, beta_a, eps_a);  R' = nothing, res or LN(res; gamma_r, beta_r, eps_r)

The reference works on the values the kernel is handed (A, W, res already rounded to bf16 and widened; the
fp32 bias / gamma / beta; eps as the fp32 value the ABI carries) and leaves A' unrounded: the kernel's rounding
of A' to bf16 as the matrix operand is the caller's `extra` term BF_ROUND * sum_k |A'[m,k] W[n,k]|."""
import itertools
import math
import types

import numpy as np
import torch
import torch.nn.functional as F

ACTS = ("none", "relu", "gelu")
RES = ("none", "plain", "ln")
# every combination of A-LN off/on, bias off/on, act, res
FLAGS = [types.SimpleNamespace(ln_a=a, bias=b, act=c, res=r)
         for a, b, c, r in itertools.product((False, True), (False, True), ACTS, RES)]
MS = (1, 19, 33, 64)
KNS = ((512, 1536), (512, 512), (2048, 512), (512, 2048), (384, 1152), (64, 8))
EPS_A, EPS_R = 1e-5, 1e-6


def flag_id(f):
    return f"lnA{int(f.ln_a)}-bias{int(f.bias)}-{f.act}-res_{f.res}"


def f32v(v):
    return float(np.float32(v))


def _ln64(x, g, b, eps):
    mu = x.mean(dim=1, keepdim=True)
    var = ((x - mu) ** 2).mean(dim=1, keepdim=True)
    return (x - mu) / torch.sqrt(var + f32v(eps)) * g.double() + b.double()


def skinny_ref(A, W, bias=None, act="none", ln_a=None, res=None, ln_res=None, parts=False):
    """(ref, scale) in float64; scale = sum_k |A'[m,k] W[n,k]| + |bias| + |R'|. ln_a / ln_res: (gamma, beta, eps).
    parts=True: also (pre, sacc): the pre-activation and sum_k |A' W| alone."""
    A, W = A.double(), W.double()
    Ap = _ln64(A, *ln_a) if ln_a is not None else A
    pre = Ap @ W.t()
    sacc = Ap.abs() @ W.abs().t()
    scale = sacc.clone()
    if bias is not None:
        pre = pre + bias.double()
        scale = scale + bias.double().abs()
    if act == "relu":
        v = torch.relu(pre)
    elif act == "gelu":
        v = 0.5 * pre * (1.0 + torch.erf(pre * (1.0 / math.sqrt(2.0))))
    else:
        assert act == "none"
        v = pre
    if res is not None:
        Rp = _ln64(res.double(), *ln_res) if ln_res is not None else res.double()
        v = v + Rp
        scale = scale + Rp.abs()
    else:
        assert ln_res is None
    return (v, scale, pre, sacc) if parts else (v, scale)


def skinny_f32(A, W, bias=None, act="none", ln_a=None, res=None, ln_res=None):
    """The same formula as a float32 torch composition on the CPU: F.layer_norm, F.linear, F.relu / F.gelu, add."""
    A, W = A.float(), W.float()
    if ln_a is not None:
        A = F.layer_norm(A, (A.shape[1],), ln_a[0], ln_a[1], ln_a[2])
    v = F.linear(A, W, bias)
    if act == "relu":
        v = F.relu(v)
    elif act == "gelu":
        v = F.gelu(v)
    if res is not None:
        r = res.float()
        if ln_res is not None:
            r = F.layer_norm(r, (r.shape[1],), ln_res[0], ln_res[1], ln_res[2])
        v = v + r
    return v


def relu_live(pre, sacc, bias, c, ln_a):
    """Elements of a ReLU case that are compared: those whose pre-activation is farther from zero than its own
    bound c * 2^-23 * (sum_k |A' W| + |bias|) (+ 2^-8 * sum_k |A' W| with LN-on-load). Inside that band the
    kernel's pre-activation may have the other sign, and ReLU turns that into an error of |pre|, not of a rounding."""
    s = sacc if bias is None else sacc + bias.double().abs()
    band = c * 2.0 ** -23 * s + (2.0 ** -8 * sacc if ln_a else 0.0)
    return pre.abs() > band


def operands(M, K, N, seed=0, coherent=False):
    """Seeded CPU operands of one shape: A, W, res as bf16-representable float32; bias, gamma, beta float32.
    A and res carry a row offset and a row scale (LayerNorm has something to remove), W is nn.Linear-sized.
    coherent (the ReLU cases): A' is positive (A = |A|; gamma_a small around beta_a = 1) and each weight row has
    one sign, alternating by output column, so that every pre-activation is of the order of sum_k |A' W| -- far
    outside the band relu_live leaves out -- with both branches of the ReLU taken (test_infer_cpu.py checks it)."""
    g = torch.Generator().manual_seed(1000 * M + K + 7 * N + seed + (500000 if coherent else 0))

    def rnd(*s):
        return torch.randn(*s, generator=g)

    def bf(t):
        return t.bfloat16().float()

    t = types.SimpleNamespace(M=M, K=K, N=N)
    t.A = bf(rnd(M, K) * (0.5 + torch.rand(M, 1, generator=g)) + 0.3 * rnd(M, 1))
    t.W = bf(rnd(N, K) / math.sqrt(K))
    t.res = bf(rnd(M, N) * (0.5 + torch.rand(M, 1, generator=g)) + 0.3 * rnd(M, 1))
    t.bias = 0.2 * rnd(N)
    t.ga, t.ba = 1.0 + 0.2 * rnd(K), 0.1 * rnd(K)
    t.gr, t.br = 1.0 + 0.2 * rnd(N), 0.1 * rnd(N)
    if coherent:
        sign = torch.where(torch.arange(N) % 2 == 0, 1.0, -1.0)
        t.A, t.W = t.A.abs(), t.W.abs() * sign[:, None]
        t.ga, t.ba = 0.2 * rnd(K), 1.0 + 0.1 * rnd(K)
    return t


def case(M, K, N, f):
    """Operands of shape (M, K, N) under flags f: the coherent set for ReLU, the general one otherwise."""
    return operands(M, K, N, coherent=f.act == "relu")


def call_args(t, f):
    """Keyword arguments of skinny_ref / skinny_f32 for operands t under flags f."""
    return dict(bias=t.bias if f.bias else None, act=f.act, ln_a=(t.ga, t.ba, EPS_A) if f.ln_a else None,
                res=None if f.res == "none" else t.res, ln_res=(t.gr, t.br, EPS_R) if f.res == "ln" else None)
