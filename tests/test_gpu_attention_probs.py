"""fer_attention_probs (csrc/attn_probs.hip) on the GPU: the softmax probabilities of the fused
attention path against an fp64 softmax of the same rounded inputs, element-wise; row sums; the
agreement with the training forward's lse and output at p = 0; row selection, head averaging and
repeated calls bit for bit; guard words around the output; padded row strides; error paths.

Element gates = 4x the maxima measured on an MI355X over every shape below (printed by each run as
`probs-measure <dtype> N H dh <per-head max|d|> <head-avg max|d|>`): bf16 inputs are exact in the
reference, so both paths sit at fp32 rounding level, orders of magnitude below the 2e-2 / 1e-4 the
training forward's test allows for the same path.
  measured: bf16 per-head 8.7e-7, head-avg 4.3e-7; fp32 per-head 1.6e-6, head-avg 7.1e-7 (the fp32
  path's scores carry the rounding of a 64-term fp32 FMA chain; the MFMA sums bf16 products exactly)
"""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = [(19, 8, 64), (37, 12, 64), (197, 12, 64), (33, 3, 32), (64, 2, 64), (1, 2, 64), (257, 2, 64), (130, 3, 80),
          (19, 4, 128)]
DTYPES = ["bf16", "fp32"]
# 4 x measured (module docstring); caps: test_attention_fwd_bwd's 2e-2 (bf16) / 1e-4 (fp32)
GATE = {"bf16": 4 * 8.7e-7, "fp32": 4 * 1.6e-6}
CAP = {"bf16": 2e-2, "fp32": 1e-4}
FWD_TOL = {"bf16": 2e-2, "fp32": 1e-4}  # test_attention_fwd_bwd: output (relative L2) and lse (absolute)
SENTINEL = -7.5


def ops():
    from fervit import ops as o

    return o


def batch(N):
    return 3 if N < 64 else 2


def make_qkv(N, H, dh, dtype):
    g = torch.Generator().manual_seed(N * 1000 + H * 10 + dh)
    qkv = 2.0 * torch.randn(batch(N) * N, 3 * H * dh, generator=g)
    return qkv.to(DEV, torch.bfloat16 if dtype == "bf16" else torch.float32)


def split_heads(qd, B, N, H, dh):
    """q, k, v as [B, H, N, dh] fp64 on the CPU, from the device buffer's (rounded) values."""
    x = qd.double().cpu().view(B, N, 3, H, dh)
    return x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2), x[:, :, 2].transpose(1, 2)


@functools.lru_cache(maxsize=None)
def case(N, H, dh, dtype):
    """Inputs, the fp64 reference and the device results of one shape (computed once, read-only)."""
    o = ops()
    B = batch(N)
    qd = make_qkv(N, H, dh, dtype)
    q, k, v = split_heads(qd, B, N, H, dh)
    s = q @ k.transpose(-1, -2) / math.sqrt(dh)
    ref = torch.softmax(s, dim=-1)  # [B, H, N, N] fp64
    per_head = o.attention_probs(qd, B, N, H, dh, average_heads=False)
    avg = o.attention_probs(qd, B, N, H, dh, average_heads=True)
    torch.cuda.synchronize()
    return dict(B=B, qd=qd, s=s, v=v, ref=ref, per_head=per_head, avg=avg)


@pytest.mark.parametrize("N,H,dh", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_probs_match_fp64_softmax(N, H, dh, dtype):
    c = case(N, H, dh, dtype)
    B = c["B"]
    ph, pa = c["per_head"].cpu(), c["avg"].cpu()
    assert ph.shape == (B, H, N, N) and pa.shape == (B, N, N) and ph.dtype == torch.float32
    e_head = (ph.double() - c["ref"]).abs().max().item()
    e_avg = (pa.double() - c["ref"].mean(1)).abs().max().item()
    print(f"probs-measure {dtype} {N} {H} {dh} {e_head:.3e} {e_avg:.3e}")
    assert GATE[dtype] <= CAP[dtype]
    for p in (ph, pa):
        assert not torch.isnan(p).any()
        assert p.min().item() >= 0.0 and p.max().item() <= 1.0
        # a fixed-order fp32 sum of N terms
        assert (p.double().sum(-1) - 1.0).abs().max().item() <= 4 * N * 2.0 ** -23
    assert e_head <= GATE[dtype], e_head
    assert e_avg <= GATE[dtype], e_avg
    # the in-kernel head mean against torch.mean of the per-head result
    assert (pa - ph.mean(1)).abs().max().item() <= 1e-6


@pytest.mark.parametrize("N,H,dh", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_agrees_with_training_forward(N, H, dh, dtype):
    """At p = 0 the maps are the probabilities fer_attention_fwd used: its saved lse is the log of the
    normaliser the device probabilities imply (log Z = s - log p at each row's largest probability,
    s recomputed in fp64), and P V from the device's per-head probabilities is its output."""
    o = ops()
    c = case(N, H, dh, dtype)
    B, qd = c["B"], c["qd"]
    out = torch.empty(B * N, H * dh, device=DEV, dtype=qd.dtype)
    saved = o.attention_saved(qd, B, N, H, dh)
    o.attention_fwd(qd, out, saved, B, N, H, dh)
    lse = saved[:B * H * N].cpu().double().view(B, H, N)
    ph = c["per_head"].cpu().double()
    pmax, idx = ph.max(dim=-1, keepdim=True)
    implied = (c["s"].gather(-1, idx) - pmax.log()).squeeze(-1)
    e_lse = (implied - lse).abs().max().item()
    pv = (ph @ c["v"]).transpose(1, 2).reshape(B * N, H * dh)
    got = out.double().cpu()
    e_out = ((got - pv).norm() / (pv.norm() + 1e-12)).item()
    print(f"probs-fwd-measure {dtype} {N} {H} {dh} lse {e_lse:.3e} out {e_out:.3e}")
    assert e_lse < FWD_TOL[dtype], e_lse
    assert e_out < FWD_TOL[dtype], e_out


@pytest.mark.parametrize("N,H,dh", [(197, 12, 64), (33, 3, 32), (257, 2, 64)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_row_selection_and_repeat_are_bitwise(N, H, dh, dtype):
    """Single rows (first, a middle query block's, the last partial block's) carry the bits of the
    full call's rows in both head modes; a second full call repeats every bit."""
    o = ops()
    c = case(N, H, dh, dtype)
    B, qd = c["B"], c["qd"]
    for avg, full in ((False, c["per_head"]), (True, c["avg"])):
        for q0 in sorted({0, N // 2, N - 1}):
            one = o.attention_probs(qd, B, N, H, dh, average_heads=avg, q_start=q0, q_count=1)
            assert one.shape[-2:] == (1, N)
            assert torch.equal(one, full[..., q0:q0 + 1, :]), (avg, q0)
        mid = o.attention_probs(qd, B, N, H, dh, average_heads=avg, q_start=1, q_count=N - 1) if N > 1 else None
        if mid is not None:
            assert torch.equal(mid, full[..., 1:, :]), avg
        again = o.attention_probs(qd, B, N, H, dh, average_heads=avg)
        assert torch.equal(again, full), avg


@pytest.mark.parametrize("N,H,dh", [(33, 3, 32), (197, 12, 64)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_guard_words_stay_untouched(N, H, dh, dtype):
    """64 sentinel floats on each side of the output survive the full and the CLS-only calls."""
    o = ops()
    c = case(N, H, dh, dtype)
    B, qd = c["B"], c["qd"]
    for avg, full in ((False, c["per_head"]), (True, c["avg"])):
        for nq in (N, 1):
            shape = (B, nq, N) if avg else (B, H, nq, N)
            n = math.prod(shape)
            buf = torch.full((n + 128,), SENTINEL, device=DEV)
            o.attention_probs(qd, B, N, H, dh, average_heads=avg, q_start=0, q_count=nq, out=buf[64:64 + n].view(shape))
            assert (buf[:64] == SENTINEL).all() and (buf[64 + n:] == SENTINEL).all(), (avg, nq)
            assert torch.equal(buf[64:64 + n].view(shape), full[..., :nq, :]), (avg, nq)


@pytest.mark.parametrize("N,H,dh", [(37, 12, 64), (130, 3, 80)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_padded_row_stride_gives_the_same_bits(N, H, dh, dtype):
    o = ops()
    c = case(N, H, dh, dtype)
    B, qd = c["B"], c["qd"]
    D3 = 3 * H * dh
    wide = torch.full((B * N, D3 + 24), float("nan"), device=DEV, dtype=qd.dtype)
    wide[:, :D3] = qd
    view = wide[:, :D3]
    assert view.stride(0) == D3 + 24
    for avg, full in ((False, c["per_head"]), (True, c["avg"])):
        assert torch.equal(o.attention_probs(view, B, N, H, dh, average_heads=avg), full), avg


@pytest.mark.parametrize("dtype", DTYPES)
def test_error_paths_launch_nothing(dtype):
    """The C entry point refuses bad row ranges, a short output and an unsupported head width with a
    negative code and a message; the output keeps its sentinel."""
    from fervit._lib import lib

    o = ops()
    B, N, H, dh = 2, 33, 3, 32
    qd = make_qkv(N, H, dh, dtype)
    code = o.dcode(qd)
    buf = torch.full((B * H * N * N,), SENTINEL, device=DEV)
    L = lib()

    def call(dh_=dh, q0=0, nq=N, floats=buf.numel(), avg=0):
        rc = L.fer_attention_probs(code, qd.data_ptr(), qd.stride(0), B, N, H, dh_, 0.25, avg, q0, nq, buf.data_ptr(),
                                   floats, o.stream())
        return rc, L.fer_last_error().decode()

    bad = [call(q0=1, nq=N), call(q0=-1, nq=2), call(nq=0), call(floats=B * H * N * N - 1),
           call(floats=B * N * N - 1, avg=1)]
    if dtype == "bf16":
        bad += [call(dh_=20), call(dh_=136)]
    torch.cuda.synchronize()
    for rc, msg in bad:
        assert rc < 0 and "attention_probs" in msg, (rc, msg)
    assert (buf == SENTINEL).all()
    with pytest.raises(ValueError):
        o.attention_probs(qd, B, N, H, dh, q_start=N - 1, q_count=2)
    with pytest.raises(ValueError):
        o.attention_probs(qd, B, N, H, dh, out=torch.empty(B, N, N + 1, device=DEV))
    assert call()[0] == 0
    torch.cuda.synchronize()
    assert (buf != SENTINEL).all()
