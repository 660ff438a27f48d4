"""float64 restatement of fer_skinny_adapter (include/fervit.h) for tests/test_infer_prenorm_cpu.py and
tests/test_gpu_skinny_adapter.py, the float32 torch compositions, the seeded operands and the error bound.

    out = X + alpha * (H W2^T + b2),   H = GELU_erf(X W1^T + b1)

The reference works on the values the kernel is handed (X, W1, W2 already rounded to bf16 and widened; the fp32
b1, b2 and alpha) and leaves H unrounded.

The bound, per output element (m, n), in the form of DESIGN.md section 2.12:

    |got - ref| <= 2^-8 * |ref| + c * 2^-23 * scale + extra
    scale = |x| + |alpha| * (sum_r |H[m,r] W2[n,r]| + |b2[n]|)
    extra = |alpha| * (2^-8 * sum_r |H[m,r] W2[n,r]| + 1.13 * c * 2^-23 * sum_r s1[m,r] |W2[n,r]|)
    s1[m,r] = sum_k |X[m,k] W1[r,k]| + |b1[r]|

Derivation (nothing in it is measured on the code under test). The kernel computes, in this order,
  pre = fp32(X W1^T) + b1      products of bf16 values are exact in fp32, so the only error is the fp32
                               accumulation and the bias add: |pre_k - pre| <= c * 2^-23 * s1, with c the
                               constant of fp32 arithmetic on such a sum (below);
  Hf  = GELU(pre_k) in fp32    |GELU'| <= 1.13 everywhere (its maximum is 1.1289 at x = sqrt(2)), so the error of
                               pre is carried into Hf with at most that slope: 1.13 * c * 2^-23 * s1. The
                               evaluation of GELU itself adds a few units of 2^-23 * |pre| <= 2^-23 * s1, which
                               is inside the factor 4 that measure_c leaves between a measured fp32 error and c;
  Hb  = bf16(Hf)               one rounding, |Hb - Hf| <= 2^-9 * |Hf|; the bound takes 2^-8 (BF_ROUND), as
                               section 2.12 does for the matrix operand rounded on load;
  S   = fp32(Hb W2^T) + b2     every error of Hb above enters the output through |alpha| * |W2[n,r]|: that is
                               `extra`. The accumulation of S, the bias add and the final fused multiply-add
                               x + alpha * S are fp32 operations on terms whose magnitudes sum to `scale`:
                               c * 2^-23 * scale;
  out = bf16(x + alpha * S)    one rounding of the result: 2^-8 * |ref|.
c comes from elemwise.measure_c on the float32 torch composition of the same formula (adapter_f32) against this
reference, with the project's floor of 16 where it measures below it. GELU has no dead zone (it is smooth, unlike
ReLU), so no element is left out of the comparison. alpha = 0 makes scale = |x|, extra = 0 and ref = x, and the
kernel's fma(0, S, x) = x is exact: the test asks for X's bits there."""
import math
import types

import torch
import torch.nn.functional as F

MS = (1, 19, 37, 64)
DRS = ((192, 32), (384, 16), (768, 64), (64, 128))
ALPHAS = (0.1, 0.37, -1.5, 0.0)
GELU_SLOPE = 1.13


def alpha32(alpha):
    """The value the kernel reads: alpha (a Python float or a one-element tensor) as fp32, widened."""
    return float(torch.as_tensor(alpha, dtype=torch.float32).reshape(()))


def _gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))


def adapter_ref(X, W1, b1, W2, b2, alpha):
    """(ref, scale, sacc, carry) in float64: scale as in the module doc, sacc = sum_r |H W2|,
    carry = sum_r s1[m,r] |W2[n,r]|. alpha: a Python float or a one-element tensor, taken as fp32."""
    X, W1, W2, b1, b2 = X.double(), W1.double(), W2.double(), b1.double(), b2.double()
    a = alpha32(alpha)
    s1 = X.abs() @ W1.abs().t() + b1.abs()
    H = _gelu64(X @ W1.t() + b1)
    sacc = H.abs() @ W2.abs().t()
    ref = X + a * (H @ W2.t() + b2)
    scale = X.abs() + abs(a) * (sacc + b2.abs())
    carry = s1 @ W2.abs().t()
    return ref, scale, sacc, carry


def adapter_extra(alpha, sacc, carry, c):
    """The absolute term of the bound (module doc)."""
    a = abs(alpha32(alpha))
    return a * (2.0 ** -8 * sacc + GELU_SLOPE * c * 2.0 ** -23 * carry)


def adapter_f32(X, W1, b1, W2, b2, alpha, round_h=False, round_out=False):
    """The same formula as a float32 torch composition on the CPU: F.linear, F.gelu, F.linear, scale, add.
    round_h / round_out: with the kernel's two rounding points (H and the result to bf16)."""
    X = X.float()
    h = F.gelu(F.linear(X, W1.float(), b1))
    if round_h:
        h = h.bfloat16().float()
    v = X + alpha32(alpha) * F.linear(h, W2.float(), b2)
    return v.bfloat16().float() if round_out else v


def operands(M, D, R, seed=0):
    """Seeded CPU operands of one shape: X, W1, W2 as bf16-representable float32; b1, b2 float32. X carries a row
    offset and a row scale, W1 is nn.Linear-sized (the hidden pre-activations are O(1): both tails and the bend
    of GELU are visited), W2 likewise."""
    g = torch.Generator().manual_seed(7000 * M + D + 13 * R + seed)

    def rnd(*s):
        return torch.randn(*s, generator=g)

    def bf(t):
        return t.bfloat16().float()

    t = types.SimpleNamespace(M=M, D=D, R=R)
    t.X = bf(rnd(M, D) * (0.5 + torch.rand(M, 1, generator=g)) + 0.3 * rnd(M, 1))
    t.W1 = bf(rnd(R, D) / math.sqrt(D))
    t.b1 = 0.2 * rnd(R)
    t.W2 = bf(rnd(D, R) / math.sqrt(R))
    t.b2 = 0.2 * rnd(D)
    return t
