"""The attention error model (tests/attention_ref.py) checked without a GPU: a torch
emulation of the bf16 kernels' rounding points (fp32 scores, P and dS rounded to bf16, fp32 accumulation,
bf16 store) must pass the very checks tests/test_gpu_attention_elementwise.py runs on the kernels, and five
subtly wrong variants of it must fail them. So the bound is sound for a correct kernel and sharp enough to
catch a block-edge or keep-bit slip that a whole-tensor norm does not see."""
import math

import pytest
import torch

import attention_ref as R

B, H, DH = 1, 2, 64
CONFIGS = [(N, p, style) for N in (70, 197) for p in (0.0, 0.1) for style in ("normal", "peaked")]
# mutant -> needs dropout
MUTANTS = {"last_key_ignored": False, "keep_pair_swapped": True, "delta_undropped": True,
           "dk_last_block_missing": False, "out_drop_scale_twice": True}


def emulate(qkv, dout, N, scale, keep, ds, mutant=None):
    """bf16-path emulation; returns (out [B*N][D] bf16 values, lse [B*H*N], dqkv [B*N][3D] bf16 values)."""
    bf = R.bf_round
    q, k, v = R.split_heads(qkv, B, N, H, DH, 3)
    do = R.split_heads(dout, B, N, H, DH)
    last = 32 * ((N - 1) // 32)  # first row of the last 32-row block
    keepf = torch.ones(B, H, N, N) if keep is None else keep.float()
    if mutant == "keep_pair_swapped":
        idx = torch.arange(N) ^ 1
        idx[idx >= N] = N - 1
        keepf = keepf[..., idx]
    s = (q @ k.transpose(-1, -2)) * scale
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    if mutant == "last_key_ignored":
        e[..., last:, N - 1] = 0
    l = e.sum(-1, keepdim=True)
    o = (bf(e * keepf) @ v) * (ds / l)
    if mutant == "out_drop_scale_twice":
        o[..., 1, :] *= ds
    o = bf(o)
    lse = m + torch.log(l)
    P = torch.exp(s - lse)
    delta = (o * do).sum(-1, keepdim=True)
    if mutant == "delta_undropped":
        delta = ((P @ v) * do).sum(-1, keepdim=True)
    dS = P * ((do @ v.transpose(-1, -2)) * keepf * ds - delta)
    dSb = bf(dS)
    dv = bf((bf(P * keepf).transpose(-1, -2) @ do) * ds)
    dq = bf((dSb @ k) * scale)
    dSk = dSb.clone()
    if mutant == "dk_last_block_missing":
        dSk[..., last:, :] = 0
    dk = bf((dSk.transpose(-1, -2) @ q) * scale)
    return R.merge_heads(o), lse.reshape(-1), R.merge_heads(dq, dk, dv)


@pytest.fixture(scope="module")
def c():
    return R.c_table([(B, N, H, DH, style, p) for N, p, style in CONFIGS], "bf16")


def run_checks(N, p, style, c, mutant):
    qkv, dout = R.make_inputs(B, N, H, DH, style, 100 * N + int(10 * p))
    _, ds = R.drop_params(p)
    scale = R.f32(1.0 / math.sqrt(DH))
    keep = R.attn_keep(77 + N, B, N, H, p)
    out, lse, dqkv = emulate(qkv, dout, N, scale, keep, ds, mutant)
    r = R.Ref(qkv, dout, B, N, H, DH, scale, keep, ds)
    worst = {}
    R.check_forward(f"N={N} p={p} {style}", r, out, lse, c, "bf16", worst=worst)
    r.bwd(out)
    R.check_backward(f"N={N} p={p} {style}", r, dqkv, c, "bf16", worst=worst)
    # the column sums, once from fp32 accumulators' worth of precision and once from the stored bf16
    R.check_colsum(f"N={N} p={p} {style}", r, dqkv.double().sum(0), None, c, "bf16", sums_rounded=True, worst=worst)
    return worst


@pytest.mark.parametrize("N,p,style", CONFIGS)
def test_emulation_within_bound(N, p, style, c):
    worst = run_checks(N, p, style, c, None)
    print("worst err/bound", {k: round(v, 3) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values())


# a mutant of the dropout arithmetic equals the correct emulation at p = 0: it runs with dropout on only
@pytest.mark.parametrize("N,p,style,mutant", [(N, p, style, mu) for N, p, style in CONFIGS for mu in sorted(MUTANTS)
                                              if p > 0 or not MUTANTS[mu]])
def test_mutant_exceeds_bound(N, p, style, mutant, c):
    with pytest.raises(AssertionError, match="out of bound"):
        run_checks(N, p, style, c, mutant)
