"""Element-wise checks of the kernels at the two ends of every model (csrc/vit_edge.hip, csrc/wplus.hip): patch
im2col, token assembly and its gradient, the classification head, the w+ prologue (SemanticPE, LayerWiseNorm, LEAM), the
LatentDecomposer projection and the latent augmentation, on every dispatch branch, through the raw C ABI.

Conventions of tests/test_gpu_rowops.py (DESIGN.md sections 2.1 and 2.6):
  * every output is a view into a NaN-filled parent whose guards and padding must keep their bits;
  * where a kernel does at most one fp32 add, one fp32 multiply and one rounding per element the result
    is compared bit for bit with the same operations in fp32 torch on the CPU;
  * everything else: |got - ref| <= out_round * |ref| + c * 2^-23 * scale_i (+ a derived term), ref a
    float64 formula on the values the kernel was handed, scale_i defined next to each formula, c measured
    by running the SAME formula function in float32 torch on the CPU against the float64 run (times 4,
    floor 16, printed as `c-measure <op> <dtype> <value>`), never from the kernel.
Each *_formula function below is written once and evaluated in float64 (the reference) and in float32 (the
measurement)."""
import functools
import math

import numpy as np
import pytest
import torch

import dropmask
from abi_harness import (exact, f32v, last_error, nanflat, nanvec, nanview, ops, out_round, ptr, tdt, untouched,
                         untouched_flat, untouched_vec)
from abi_harness import lib as L
from dropmask import keep_mask, keep_mask_torch
from elemwise import U, assert_bits_equal, assert_close, measure_c

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
CAP = 8192 * 256  # element kernels launch at most 8192 blocks of 256 threads: beyond it the grid-stride loop
F64, F32 = torch.float64, torch.float32


def dcode(dtype):
    return 0 if dtype == "bf16" else 1


def stream():
    return ops().stream()


def dev(t):
    return None if t is None else t.to(DEV).contiguous()


def nanws(nbytes):
    """A NaN-filled workspace: a partial slab the kernel leaves unwritten poisons the reduced result."""
    return torch.full((max(1, nbytes // 4),), NAN, dtype=F32, device=DEV)


def drop(p):
    thr, sc = ops().drop_args(p)
    return thr, f32v(sc)


@functools.lru_cache(maxsize=64)
def host_keep(seed, n, p):
    return keep_mask(seed, (n,), p)


# ====================================================================== im2col
def im2col_ref(x, P, dt):
    """cols[(b, gy, gx)][(c, kh, kw)] = x[b][c][gy P + kh][gx P + kw], cast to dt (one rounding)."""
    B, C, H, W = x.shape
    gh, gw = H // P, W // P
    v = x[:, :, :gh * P, :gw * P].reshape(B, C, gh, P, gw, P).permute(0, 2, 4, 1, 3, 5)
    return v.reshape(B * gh * gw, C * P * P).to(dt)


def run_im2col(dtype, shape, ldc_pad, shift, seed=11):
    B, C, H, W, P = shape
    dt = tdt(dtype)
    K, rows = C * P * P, B * (H // P) * (W // P)
    x0 = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(seed))
    xv, xp = nanflat(x0.numel(), F32, x0, shift=shift)
    assert xv.data_ptr() % 16 == (4 * shift) % 16
    cols, cp = nanview(rows, K, ldc_pad, dt, align=(16 if (K + ldc_pad) % 4 == 0 else 2))
    rc = L().fer_im2col_patch(dcode(dtype), xv.data_ptr(), B, C, H, W, P, cols.data_ptr(), K + ldc_pad, stream())
    assert rc == 0, last_error()
    assert_bits_equal("im2col cols", cols.contiguous(), im2col_ref(x0, P, dt).to(DEV))
    untouched("im2col cols", cp, rows, K)
    untouched_flat("im2col x", xp, x0.numel(), shift=shift)


IM2COL_SHAPES = {
    "4wide": (2, 3, 16, 16, 4),
    "P3": (2, 3, 12, 12, 3),
    "W18": (2, 1, 16, 18, 4),
    "H18": (1, 2, 18, 16, 4),
}


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("ldc_pad", [0, 8, 2])
@pytest.mark.parametrize("shape", sorted(IM2COL_SHAPES))
def test_im2col_branches(dtype, shape, ldc_pad):
    """fer_im2col_patch, exact. 4wide with ldc = K or K + 8: im2col4_kernel (P, W, ldc multiples of 4, x
    16-byte aligned); ldc = K + 2 sends every shape to the scalar im2col_kernel. P3 (P % 4 != 0) and W18
    (W % 4 != 0; the last two image columns belong to no patch) are scalar at every ldc; H18 leaves two image
    rows beyond gh * P unread and stays 4-wide. The padding columns of cols keep their NaN bits."""
    run_im2col(dtype, IM2COL_SHAPES[shape], ldc_pad, 0)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_im2col_unaligned_x(dtype):
    """x one float into its parent (4-byte aligned): the 4-wide shape must take the scalar im2col_kernel, whose
    result is the same bits."""
    run_im2col(dtype, IM2COL_SHAPES["4wide"], 0, 1)
    run_im2col(dtype, IM2COL_SHAPES["4wide"], 8, 1)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("kind", ["im2col4", "scalar"])
def test_im2col_grid_stride(dtype, kind):
    """More work than 8192 blocks cover in one pass. im2col4_kernel: (3, 3, 976, 976, 16), total / 4 = 2,143,296
    > 8192 * 256. im2col_kernel: (1, 3, 976, 976, 16) at ldc = K + 2, total = 2,857,728."""
    shape, pad = ((3, 3, 976, 976, 16), 0) if kind == "im2col4" else ((1, 3, 976, 976, 16), 2)
    B, C, H, W, P = shape
    total = B * C * H * W
    assert (total // 4 if kind == "im2col4" else total) > CAP
    run_im2col(dtype, shape, pad, 0)


# ====================================================================== tokens forward
def tokens_fwd_ref(emb, cls, pos, B, n, D, keep, sc, dt):
    """fp32: (cls | emb) + pos, one add; kept elements times the fp32 dropout scale, one multiply; dropped
    ones +0.0; one rounding to dt."""
    v = torch.cat([cls.view(1, 1, D).expand(B, 1, D), emb.float().view(B, n, D)], 1) + pos.view(1, n + 1, D)
    if keep is not None:
        v = torch.where(keep.view(B, n + 1, D), v * torch.tensor(sc, dtype=F32), torch.zeros((), dtype=F32))
    return v.to(dt).reshape(-1)


def run_tokens_fwd(dtype, B, n, D, p, seed=4242, big=False):
    dt = tdt(dtype)
    N = n + 1
    g = torch.Generator().manual_seed(100 * D + B)
    emb0 = torch.randn(B * n, D, generator=g).to(dt)
    cls, pos = torch.randn(D, generator=g), torch.randn(N * D, generator=g)
    thr, sc = drop(p)
    total = B * N * D
    tv, tp = nanflat(total, dt)
    embd, clsd, posd = dev(emb0), dev(cls), dev(pos)
    rc = L().fer_tokens_fwd(dcode(dtype), embd.data_ptr(), clsd.data_ptr(), posd.data_ptr(), tv.data_ptr(), B, n, D,
                            thr, sc, seed, stream())
    assert rc == 0, last_error()
    if big:  # the keep mask of 17 M elements with integer arithmetic on the device; the values on the CPU
        keep = keep_mask_torch(seed, (total,), p)
        kept = tokens_fwd_ref(emb0, cls, pos, B, n, D, torch.ones(total, dtype=torch.bool), sc, dt).to(DEV)
        ref = torch.where(keep, kept, torch.zeros((), dtype=dt, device=DEV))
    else:
        keep = host_keep(seed, total, p) if p > 0 else None
        ref = tokens_fwd_ref(emb0, cls, pos, B, n, D, keep, sc, dt).to(DEV)
    assert_bits_equal("tokens_fwd t", tv.contiguous(), ref)
    if keep is not None:
        dropped = tv[~keep.to(DEV)]
        assert dropped.numel() > 0 or total < 64
        assert_bits_equal("tokens_fwd dropped elements are +0.0", dropped, torch.zeros_like(dropped))
    untouched_flat("tokens_fwd t", tp, total)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("B,n", [(1, 1), (3, 2), (4, 9)])
@pytest.mark.parametrize("dtype,D", [("bf16", 8), ("bf16", 12), ("fp32", 12), ("bf16", 6), ("fp32", 6), ("bf16", 768),
                                     ("fp32", 768)])
def test_tokens_fwd_branches(dtype, D, B, n, p):
    """fer_tokens_fwd, exact, with and without dropout. bf16 D = 8 and 768: tokens_fwd8_kernel (D % 8 == 0); D = 12
    (D % 4 == 0, D % 8 != 0) in bf16 and every D % 4 == 0 in fp32 (12, 768): tokens_fwd4_kernel<T>, fp32 with
    dropout included; D = 6: the scalar tokens_fwd_kernel<T>. (B, n) = (1, 1) is one CLS and one patch row."""
    run_tokens_fwd(dtype, B, n, D, p)


@pytest.mark.parametrize("dtype,B,n,D", [("bf16", 110, 199, 768), ("fp32", 55, 199, 768), ("fp32", 1750, 199, 6),
                                         ("bf16", 1750, 199, 6)])
def test_tokens_fwd_grid_stride(dtype, B, n, D):
    """Past the 8192-block cap, p = 0.1: tokens_fwd8_kernel at total / 8 = 2,112,000, tokens_fwd4_kernel<float>
    at total / 4 = 2,112,000, tokens_fwd_kernel<T> (D = 6) at total = 2,100,000."""
    total = B * (n + 1) * D
    per = 8 if (dtype == "bf16" and D % 8 == 0) else (4 if D % 4 == 0 else 1)
    assert total // per > CAP
    run_tokens_fwd(dtype, B, n, D, 0.1, big=True)


# ====================================================================== tokens backward
def tokens_bwd_formula(dtv, keep, sc, B, N, D, dt):
    """g = dt (kept: times the dropout scale; dropped: 0); demb = g[:, 1:]; dpos = sum_b g; dcls = dpos[0].
    scale of dpos / dcls: sum_b |g|."""
    g = dtv.to(dt).view(B, N, D)
    if keep is not None:
        g = torch.where(keep.view(B, N, D), g * torch.tensor(sc, dtype=dt), torch.zeros((), dtype=dt))
    return dict(g=g, dpos=g.sum(0).reshape(-1), s_dpos=g.abs().sum(0).reshape(-1))


TOK_OPTS = [dict(p=0.0, acc=0, null=None), dict(p=0.1, acc=1, null=None), dict(p=0.1, acc=0, null="demb"),
            dict(p=0.1, acc=0, null="dcls"), dict(p=0.0, acc=1, null="dpos")]


@pytest.mark.parametrize("B", [1, 3, 17, 41, 65])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("D,n", [(8, 1), (768, 9), (12, 1), (388, 9), (6, 1), (6, 9)])
def test_tokens_bwd_branches(dtype, D, n, B):
    """fer_tokens_bwd: demb exact, dpos / dcls within the measured bound (scale sum_b |g|). bf16 D = 8, 768:
    tokens_bwd8_kernel (16 batch chunks: B = 17 gives bchunk = 2 and empty chunks 9..15, B = 41 bchunk = 3, B = 65
    bchunk = 5); D = 12, 388 and fp32 D = 8, 768: tokens_bwd4_kernel<T> (64 chunks: B = 65 gives bchunk = 2 and
    empty chunks 33..63); D = 6: tokens_bwd_kernel<T>. The workspace is NaN-filled, so an empty chunk that does
    not write its zero slab shows in dpos. N D = 7680 (D = 768, n = 9) takes part_reduce_kernel<16>, the rest
    part_reduce_kernel<8>. Each case runs p in {0, 0.1}, accumulate in {0, 1} (outputs preset to random values)
    and demb / dcls / dpos null in turn."""
    dt = tdt(dtype)
    N = n + 1
    total = B * N * D
    g = torch.Generator().manual_seed(7 * D + B)
    dt0 = torch.randn(total, generator=g).to(dt)
    dtd = dev(dt0)
    for k, o in enumerate(TOK_OPTS):
        seed = 900 + k
        thr, sc = drop(o["p"])
        keep = host_keep(seed, total, o["p"]) if o["p"] > 0 else None
        r64 = tokens_bwd_formula(dt0.float(), keep, sc, B, N, D, F64)
        r32 = tokens_bwd_formula(dt0.float(), keep, sc, B, N, D, F32)
        c = measure_c("tokens_bwd.dpos", dtype, [(r32["dpos"], r64["dpos"], r64["s_dpos"])])
        init_pos, init_cls = torch.randn(N * D, generator=g) * 3, torch.randn(D, generator=g) * 3
        dembv, dembp = nanflat(B * n * D, dt)
        dposv, dposp = nanvec(N * D)
        dclsv, dclsp = nanvec(D)
        if o["acc"]:
            dposv.copy_(init_pos)
            dclsv.copy_(init_cls)
        ws = nanws(L().fer_tokens_bwd_ws(B, N, D))
        null = o["null"]
        rc = L().fer_tokens_bwd(dcode(dtype), dtd.data_ptr(), None if null == "demb" else dembv.data_ptr(),
                                None if null == "dcls" else dclsv.data_ptr(),
                                None if null == "dpos" else dposv.data_ptr(), o["acc"], B, n, D, thr, sc, seed,
                                ws.data_ptr(), ws.numel() * 4, stream())
        assert rc == 0, last_error()
        tag = f"tokens_bwd[{o}]"
        if null == "demb":
            assert torch.isnan(dembp).all().item(), tag + ": demb written though null"
        else:
            assert_bits_equal(tag + " demb", dembv.contiguous(), r32["g"][:, 1:].to(dt).reshape(-1).to(DEV))
        untouched_flat(tag + " demb", dembp, B * n * D)
        ref, sca = r64["dpos"], r64["s_dpos"]
        if o["acc"]:
            ref, sca = ref + init_pos.double(), sca + init_pos.double().abs()
        if null == "dpos":
            assert_bits_equal(tag + " dpos kept", dposv, (init_pos if o["acc"] else torch.full((N * D,), NAN)).to(DEV))
        else:
            assert_close(tag + " dpos", dposv, ref, sca, c, 0.0)
        refc, scac = r64["dpos"][:D], r64["s_dpos"][:D]
        if o["acc"]:
            refc, scac = refc + init_cls.double(), scac + init_cls.double().abs()
        if null == "dcls":
            assert torch.isnan(dclsp).all().item(), tag + ": dcls written though null"
        else:
            assert_close(tag + " dcls", dclsv, refc, scac, c, 0.0)
        untouched_vec(tag + " dpos", dposp, N * D)
        untouched_vec(tag + " dcls", dclsp, D)


# ====================================================================== head
def head_fwd_formula(x, lw, lb, W, bias, eps, keep, sc, dt, stats=None):
    """LayerNorm of the CLS rows, dropout, Linear. Scales: mean: mean|x|; rstd: rstd; h (the LayerNorm output,
    as in DESIGN.md 2.1): (|x| + |mu|) rstd |lw| + |lb|; logits: sum_d s_h sc keep |W| + |bias| (the error of
    each h carried through the product, and the products the dot sums)."""
    x, lw, lb, W, bias = (t.to(dt) for t in (x, lw, lb, W, bias))
    D = x.shape[1]
    if stats is None:
        mu = x.mean(1, keepdim=True)
        rs = (((x - mu) ** 2).mean(1, keepdim=True) + eps) ** -0.5
    else:
        mu, rs = stats[:, 0:1].to(dt), stats[:, 1:2].to(dt)
    xh = (x - mu) * rs
    s_xh = (x.abs() + mu.abs()) * rs
    h = xh * lw + lb
    s_h = s_xh * lw.abs() + lb.abs()
    k = torch.ones_like(h) if keep is None else keep.to(dt) * sc
    hd, s_hd = h * k, s_h * k
    return dict(mu=mu[:, 0], rs=rs[:, 0], xh=xh, s_xh=s_xh, hd=hd, s_hd=s_hd, k=k, logits=hd @ W.t() + bias,
                s_logits=s_hd @ W.abs().t() + bias.abs(), s_mu=x.abs().mean(1))


def head_bwd_formula(x, lw, lb, W, dl, stats, keep, sc, dt):
    """Backward from the fp32 mean / rstd the kernel is handed. g = (dl W) keep sc; dln_w = sum_b g xh;
    dln_b = sum_b g; dt = rstd (g lw - mean(g lw) - xh mean(g lw xh)); dW = sum_b dl hd; dbias = sum_b dl.
    Scales: the same expressions on magnitudes, with s_xh = (|x| + |mu|) rstd in place of |xh| and
    s_g = (|dl| |W|) keep sc in place of |g|."""
    f = head_fwd_formula(x, lw, lb, W, torch.zeros(W.shape[0]), 0.0, keep, sc, dt, stats=stats)
    dl, W, lw = dl.to(dt), W.to(dt), lw.to(dt)
    rs = f["rs"][:, None]
    g, s_g = (dl @ W) * f["k"], (dl.abs() @ W.abs()) * f["k"]
    gg, s_gg = g * lw, s_g * lw.abs()
    xh, s_xh = f["xh"], f["s_xh"]
    dtv = rs * (gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True))
    s_dt = rs * (s_gg + s_gg.mean(1, keepdim=True) + s_xh * (s_gg * s_xh).mean(1, keepdim=True))
    return dict(dt=dtv, s_dt=s_dt, dW=dl.t() @ f["hd"], s_dW=dl.abs().t() @ f["s_hd"], dbias=dl.sum(0),
                s_dbias=dl.abs().sum(0), dln_w=(g * xh).sum(0), s_dln_w=(s_g * s_xh).sum(0), dln_b=g.sum(0),
                s_dln_b=s_g.sum(0))


HEAD_GRADS = ("dln_w", "dln_b", "dW", "dbias")
HEAD_CASES = {
    "D4_C255": dict(D=4, C=255, B=5, N=5, pad=0, zero=1),
    "D6_C256_zero_rows": dict(D=6, C=256, B=37, N=5, pad=0, zero=1, p=0.1, acc=1),
    "D4_C257_N1": dict(D=4, C=257, B=5, N=1, pad=8, zero=1, eps=1e-6),
    "D6_C300_B1_ld2": dict(D=6, C=300, B=1, N=5, pad=2, zero=0, p=0.1),
    "D8_C300_acc": dict(D=8, C=300, B=5, N=5, pad=8, zero=1, p=0.1, acc=1),
    "D252_C7": dict(D=252, C=7, B=37, N=5, pad=8, zero=1, p=0.1),
    "D768_ld2_zero_rows": dict(D=768, C=7, B=5, N=5, pad=2, zero=1, acc=1, eps=1e-6),
    "D1000_C1_no_dW": dict(D=1000, C=1, B=5, N=5, pad=0, zero=0, null="dW"),
    "D1024_N1_no_dbias": dict(D=1024, C=7, B=37, N=1, pad=8, zero=1, p=0.1, null="dbias"),
    "D1024_B1_no_dln_w": dict(D=1024, C=1, B=1, N=5, pad=0, zero=1, null="dln_w"),
    "D768_no_dln_b_acc": dict(D=768, C=7, B=5, N=5, pad=0, zero=0, acc=1, null="dln_b", p=0.1),
}


def call_head_fwd(dtype, t, rs_, lw, lb, eps, W, bias, logits, stats, B, D, C, thr, sc, seed):
    return L().fer_head_fwd(dcode(dtype), t.data_ptr(), rs_, lw.data_ptr(), lb.data_ptr(), eps, W.data_ptr(),
                            bias.data_ptr(), logits.data_ptr(), stats.data_ptr(), B, D, C, thr, sc, seed, stream())


def call_head_bwd(dtype, t, rs_, lw, lb, W, stats, dl, dtv, zero, rows, D_ld, grads, acc, B, D, C, thr, sc, seed):
    ws = nanws(L().fer_head_bwd_ws(B, D, C))
    return L().fer_head_bwd(dcode(dtype), t.data_ptr(), rs_, lw.data_ptr(), lb.data_ptr(), W.data_ptr(),
                            stats.data_ptr(), dl.data_ptr(), dtv.data_ptr(), zero, rows, D_ld, ptr(grads["dln_w"]),
                            ptr(grads["dln_b"]), ptr(grads["dW"]), ptr(grads["dbias"]), acc, B, D, C, thr, sc, seed,
                            ws.data_ptr(), ws.numel() * 4, stream())


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("case", sorted(HEAD_CASES))
def test_head_elementwise(dtype, case):
    """fer_head_fwd / fer_head_bwd: logits, stats, dt, dW, dbias, dln_w, dln_b per element. head_fwd_kernel<T> and
    head_bwd_kernel<T> walk D in strides of 256 (D = 4, 6, 8: one partial trip; 252: one; 768: three; 1000: a
    partial fourth; 1024: four full) and C in strides of 4 waves; C = 255, 256, 257, 300 at D <= 8 reach the
    per-sample dbias partial beyond thread 255 (C > 256 was never written before the store looped over C).
    The CLS rows sit at row_stride = N D_ld inside a [B N][D_ld] parent, D_ld = D, D + 8 or D + 2; the other
    rows of the input are NaN (never read). zero = 1: the other rows of dt are exactly zero, by
    zero_rows4_kernel<T> (D and D_ld multiples of 4) or zero_rows_kernel<T> (D = 6, or D_ld = D + 2); padding
    columns keep their NaN. zero = 0: the other rows keep their NaN. N = 1: no other rows. Sample 1 is a
    constant row (variance 0, rstd = eps^-1/2), sample 2 has a common offset of 100. null: that gradient
    output is a null pointer (part_reduce with null outputs, or skipped)."""
    o = dict(dict(p=0.0, acc=0, eps=1e-5, null=None), **HEAD_CASES[case])
    D, C, B, N, pad, zero = o["D"], o["C"], o["B"], o["N"], o["pad"], o["zero"]
    dt, oround = tdt(dtype), out_round(dtype)
    D_ld, seed, eps = D + pad, 31337 + D, f32v(o["eps"])
    g = torch.Generator().manual_seed(13 * D + C)
    x0 = torch.randn(B, D, generator=g) * 2 + 0.5
    if B >= 5:
        x0[1] = 0.75
        x0[2] = x0[2] * 0.5 + 100.0
    lw, lb = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    W, bias = torch.randn(C, D, generator=g) / math.sqrt(D), torch.randn(C, generator=g)
    dl = torch.randn(B, C, generator=g)
    tin, _ = nanview(B * N, D, pad, dt, guard=0, align=2)
    tin[::N] = x0.to(DEV).to(dt)
    x = exact(tin[::N])
    thr, sc = drop(o["p"])
    keep = keep_mask(seed, (B, D), o["p"]) if o["p"] > 0 else None
    lwd, lbd, Wd, bd, dld = dev(lw), dev(lb), dev(W), dev(bias), dev(dl)

    logits, lp = nanvec(B * C)
    stats, sp = nanvec(2 * B)
    rc = call_head_fwd(dtype, tin, N * D_ld, lwd, lbd, eps, Wd, bd, logits, stats, B, D, C, thr, sc, seed)
    assert rc == 0, last_error()
    f64 = head_fwd_formula(x, lw, lb, W, bias, eps, keep, sc, F64)
    f32 = head_fwd_formula(x, lw, lb, W, bias, eps, keep, sc, F32)
    c_l = measure_c("head.logits", dtype, [(f32["logits"], f64["logits"], f64["s_logits"])])
    c_m = measure_c("head.mean", dtype, [(f32["mu"], f64["mu"], f64["s_mu"])])
    c_r = measure_c("head.rstd", dtype, [(f32["rs"], f64["rs"], f64["rs"])])
    assert_close("head logits", logits, f64["logits"], f64["s_logits"], c_l, 0.0)
    st = stats.view(B, 2)
    assert_close("head mean", st[:, 0], f64["mu"], f64["s_mu"], c_m, 0.0)
    assert_close("head rstd", st[:, 1], f64["rs"], f64["rs"], c_r, 0.0)
    untouched_vec("head logits", lp, B * C)
    untouched_vec("head stats", sp, 2 * B)

    # ---- backward, from the statistics the forward kernel wrote
    st_in = st.cpu().double()
    b64 = head_bwd_formula(x, lw, lb, W, dl, st_in, keep, sc, F64)
    b32 = head_bwd_formula(x, lw, lb, W, dl, st_in, keep, sc, F32)
    shapes = dict(dln_w=(D,), dln_b=(D,), dW=(C, D), dbias=(C,))
    init = {k: torch.randn(*shapes[k], generator=g) * 3 for k in HEAD_GRADS}
    grads, gpar = {}, {}
    for k in HEAD_GRADS:
        v, gpar[k] = nanvec(int(np.prod(shapes[k])))
        if o["acc"]:
            v.copy_(init[k].reshape(-1))
        grads[k] = None if o["null"] == k else v
    dtv, dtp = nanview(B * N, D, pad, dt, guard=2, align=2)
    rc = call_head_bwd(dtype, tin, N * D_ld, lwd, lbd, Wd, stats, dld, dtv, zero, B * N, D_ld, grads, o["acc"], B, D,
                       C, thr, sc, seed)
    assert rc == 0, last_error()
    c_dt = measure_c("head.dt", dtype, [(b32["dt"], b64["dt"], b64["s_dt"])])
    assert_close("head dt", dtv[::N], b64["dt"], b64["s_dt"], c_dt, oround)
    if N > 1:
        rest = torch.ones(B * N, dtype=torch.bool)
        rest[::N] = False
        others = dtv[rest.to(DEV)]
        want = torch.zeros_like(others) if zero else torch.full_like(others, NAN)
        assert_bits_equal(f"head dt rows other than CLS (zero_rest = {zero})", others, want)
    untouched("head dt", dtp, B * N, D, guard=2)
    for k in HEAD_GRADS:
        n_k = int(np.prod(shapes[k]))
        if grads[k] is None:
            want = init[k].reshape(-1) if o["acc"] else torch.full((n_k,), NAN)
            assert_bits_equal(f"head {k} (null output) left alone", gpar[k][4:4 + n_k], want.to(DEV))
        else:
            c_k = measure_c(f"head.{k}", dtype, [(b32[k], b64[k], b64["s_" + k])])
            ref, sca = b64[k], b64["s_" + k]
            if o["acc"]:
                ref, sca = ref + init[k].double(), sca + init[k].double().abs()
            assert_close(f"head {k}", grads[k], ref, sca, c_k, 0.0)
        untouched_vec(f"head {k}", gpar[k], n_k)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_head_too_wide_is_an_error(dtype):
    """D = 1028 > 1024 (the LDS row of head_fwd_kernel / head_bwd_kernel): both entry points return non-zero
    with their message and launch nothing."""
    B, D, C, dt = 3, 1028, 7, tdt(dtype)
    t = torch.ones(B, D, dtype=dt, device=DEV)
    w = torch.ones(D, device=DEV)
    W, bias = torch.ones(C, D, device=DEV), torch.ones(C, device=DEV)
    logits, lp = nanvec(B * C)
    stats, sp = nanvec(2 * B)
    rc = call_head_fwd(dtype, t, D, w, w, 1e-5, W, bias, logits, stats, B, D, C, 0, 1.0, 0)
    assert rc != 0 and "head_fwd: D <= 1024" in last_error()
    grads = {k: torch.full((n_k,), NAN, device=DEV) for k, n_k in (("dln_w", D), ("dln_b", D), ("dW", C * D), ("dbias", C))}
    dtv = torch.full((B, D), NAN, dtype=dt, device=DEV)
    st_in = torch.ones(2 * B, device=DEV)
    rc = call_head_bwd(dtype, t, D, w, w, W, st_in, torch.ones(B, C, device=DEV), dtv, 1, B, D, grads, 0, B, D, C, 0,
                       1.0, 0)
    assert rc != 0 and "head_bwd: D <= 1024" in last_error()
    torch.cuda.synchronize()
    for name, v in dict(grads, logits=lp, stats=sp, dt=dtv).items():
        assert torch.isnan(v).all().item(), f"{name} written by a rejected call"


# ====================================================================== w+ prologue
def sig_err(x):
    """Derived, not measured: the kernels form sigmoid(x) = 1 / (1 + __expf(-x)), __expf being
    v_exp_f32 of x log2(e); the rounding of that product is carried through the exponent (|x| 2^-24) and the
    instruction, the add and the division add a few 2^-24 more: relative error <= (|x| + 4) 2^-23."""
    return (x.abs() + 4.0) * U


def wplus_formula(x, dy, P, eps, saved, dt):
    """x [B][L][D]; P: sg [3][D], sl [L][D], grp [L], lw, lb [L][D], gate [L], lm [L] (each pair / scalar may
    be None). Forward: a = x + sg[grp] + sl; n = LN_l(a); u = a + s(gate) (n - a) | n | a; y = u s(lm).
    Backward from `saved` (the fp32 mean / rstd handed to the kernel; None: the formula's own).
    Scales: s_a = |x| + |sg| + |sl|, s_xh = (s_a + |mu|) rstd, s_n = s_xh |lw| + |lb|, s_u = s_a + s(gate)
    (s_n + s_a) | s_n | s_a, s_y = s_u s(lm); the gradients' scales are their own expressions on these
    magnitudes. e_*: the derived relative terms of the two sigmoids (sig_err), for 1 - s scaled by s / (1 - s);
    x_<output>: the absolute term they give, each e on the magnitude its factor multiplies and no other: in dx
    (and its sums d_sl, d_sg) e_leam + e_gate on the LayerNorm part (dn = dy s(lm) s(gate)) and e_leam +
    e_(1-gate) on |dy| s(lm) (1 - s(gate)); d_lw, d_lb: e_leam + e_gate; d_gate: e_leam (in du) + e_gate +
    e_(1-gate) (the factor s (1 - s)); d_leam: e_gate (in u) + e_leam + e_(1-leam)."""
    B, Lr, D = x.shape
    c = lambda t: None if t is None else t.to(dt)
    x, dy = c(x), c(dy)
    sg, sl, lw, lb, gate, lm = (c(P[k]) for k in ("sg", "sl", "lw", "lb", "gate", "lm"))
    grp = P["grp"]
    zero, one = torch.zeros(Lr, dtype=dt), torch.ones(Lr, dtype=dt)
    a, s_a = x, x.abs()
    if sg is not None:
        a = x + (sg[grp] + sl)
        s_a = x.abs() + sg[grp].abs() + sl.abs()
    sgate = torch.sigmoid(gate) if gate is not None else zero
    slm = torch.sigmoid(lm) if lm is not None else one
    e_g = sig_err(gate.double()) if gate is not None else zero.double()
    e_g1 = e_g * (sgate / (1 - sgate)).double() if gate is not None else zero.double()
    e_l = sig_err(lm.double()) if lm is not None else zero.double()
    e_l1 = e_l * (slm / (1 - slm)).double() if lm is not None else zero.double()
    G, S = sgate.view(1, Lr, 1), slm.view(1, Lr, 1)
    EL, EG, EG1 = e_l.view(1, Lr, 1), e_g.view(1, Lr, 1), e_g1.view(1, Lr, 1)
    r = dict()
    if lw is not None:
        if saved is None:
            mu = a.mean(2, keepdim=True)
            rs = (((a - mu) ** 2).mean(2, keepdim=True) + eps) ** -0.5
        else:
            mu, rs = saved[..., 0:1].to(dt), saved[..., 1:2].to(dt)
        xh, s_xh = (a - mu) * rs, (s_a + mu.abs()) * rs
        n, s_n = xh * lw + lb, s_xh * lw.abs() + lb.abs()
        u, s_u = (a + G * (n - a), s_a + G * (s_n + s_a)) if gate is not None else (n, s_n)
        r.update(mu=mu[..., 0], rs=rs[..., 0], s_mu=s_a.mean(2))
        r["x_y"] = (e_g.view(1, Lr, 1) * (G * (n - a)).abs().double() * S.double() if gate is not None else 0.0)
    else:
        u, s_u = a, s_a
        r["x_y"] = 0.0
    r.update(y=u * S, s_y=s_u * S)
    r["x_y"] = r["x_y"] + e_l.view(1, Lr, 1) * r["y"].abs().double()
    if dy is None:
        return r
    du, s_du = dy * S, dy.abs() * S
    al, s_al = (dy * u).sum(2), (dy.abs() * s_u).sum(2)
    if lw is not None:
        dn, s_dn = (du * G, s_du * G) if gate is not None else (du, s_du)
        gg, s_gg = dn * lw, s_dn * lw.abs()
        dv = rs * (gg - gg.mean(2, keepdim=True) - xh * (gg * xh).mean(2, keepdim=True))
        s_dv = rs * (s_gg + s_gg.mean(2, keepdim=True) + s_xh * (s_gg * s_xh).mean(2, keepdim=True))
        x_dv = (EL + EG) * s_dv.double()
        if gate is not None:
            dv, s_dv = dv + du * (1 - G), s_dv + s_du * (1 - G)
            x_dv = x_dv + (EL + EG1) * (s_du * (1 - G)).double()
            ag, s_ag = (du * (n - a)).sum(2), (s_du * (s_n + s_a)).sum(2)
            r.update(d_gate=ag.sum(0) * sgate * (1 - sgate), s_d_gate=s_ag.sum(0) * sgate * (1 - sgate))
            r["x_d_gate"] = (e_l + e_g + e_g1) * r["s_d_gate"].double()
        r.update(d_lw=(dn * xh).sum(0), s_d_lw=(s_dn * s_xh).sum(0), d_lb=dn.sum(0), s_d_lb=s_dn.sum(0))
        r.update(x_d_lw=(e_l + e_g).view(Lr, 1) * r["s_d_lw"].double(), x_d_lb=(e_l + e_g).view(Lr, 1) * r["s_d_lb"].double())
    else:
        dv, s_dv = du, s_du
        x_dv = EL * s_du.double()
    r.update(dx=dv, s_dx=s_dv, x_dx=x_dv)
    if sg is not None:
        dsl, s_dsl = dv.sum(0), s_dv.sum(0)
        onehot = torch.nn.functional.one_hot(grp, 3).to(dt)  # [L][3]
        r.update(d_sl=dsl, s_d_sl=s_dsl, d_sg=onehot.t() @ dsl, s_d_sg=onehot.t() @ s_dsl, x_d_sl=x_dv.sum(0),
                 x_d_sg=onehot.t().double() @ x_dv.sum(0))
    if lm is not None:
        r.update(d_leam=al.sum(0) * slm * (1 - slm), s_d_leam=s_al.sum(0) * slm * (1 - slm))
        r["x_d_leam"] = (e_g + e_l + e_l1) * r["s_d_leam"].double()
    return r


WPLUS_COMBOS = [(spe, lwn, leam) for spe in (0, 1) for lwn in ("none", "lwn", "gate") for leam in (0, 1)]
WPLUS_CONFIGS = [dict(D=4, Lr=1, B=1), dict(D=255, Lr=18, B=3), dict(D=256, Lr=18, B=33, acc=1),
                 dict(D=257, Lr=1, B=70), dict(D=512, Lr=18, B=3, nulls=True), dict(D=1000, Lr=18, B=1),
                 dict(D=1024, Lr=18, B=3, acc=1)]
WPLUS_OUT = ("d_sg", "d_sl", "d_lw", "d_lb", "d_gate", "d_leam")
LOGITS = [0.0, -4.0, 4.0, -3.5, 3.5, -3.0, 3.0, -2.5, 2.5, -2.0, 2.0, -1.5, 1.5, -1.0, 1.0, -0.5, 0.5, 0.25]


def wplus_params(combo, Lr, D, g):
    spe, lwn, leam = combo
    P = dict(sg=None, sl=None, grp=None, lw=None, lb=None, gate=None, lm=None)
    if spe:
        P.update(sg=torch.randn(3, D, generator=g), sl=torch.randn(Lr, D, generator=g),
                 grp=(torch.arange(Lr) * 3 // max(Lr, 3)) if Lr > 1 else torch.tensor([2]))
    if lwn != "none":
        P.update(lw=1 + 0.1 * torch.randn(Lr, D, generator=g), lb=0.1 * torch.randn(Lr, D, generator=g))
    if lwn == "gate":
        P["gate"] = torch.tensor(LOGITS[:Lr])
    if leam:
        P["lm"] = torch.tensor(LOGITS[:Lr][::-1]) if Lr > 1 else torch.tensor([0.0])
    return P


def call_wplus_fwd(x, y, B, Lr, D, Pd, eps, saved):
    return L().fer_wplus_fwd(x.data_ptr(), y.data_ptr(), B, Lr, D, ptr(Pd["sg"]), ptr(Pd["sl"]), ptr(Pd["grp"]),
                             ptr(Pd["lw"]), ptr(Pd["lb"]), ptr(Pd["gate"]), ptr(Pd["lm"]), eps, ptr(saved), stream())


def call_wplus_bwd(x, saved, dy, dx, B, Lr, D, Pd, eps, outs, acc):
    ws = nanws(L().fer_wplus_ws(B, Lr, D))
    return L().fer_wplus_bwd(x.data_ptr(), ptr(saved), dy.data_ptr(), dx.data_ptr(), B, Lr, D, ptr(Pd["sg"]),
                             ptr(Pd["sl"]), ptr(Pd["grp"]), ptr(Pd["lw"]), ptr(Pd["lb"]), ptr(Pd["gate"]),
                             ptr(Pd["lm"]), eps, ptr(outs["d_sg"]), ptr(outs["d_sl"]), ptr(outs["d_lw"]),
                             ptr(outs["d_lb"]), ptr(outs["d_gate"]), ptr(outs["d_leam"]), acc, ws.data_ptr(),
                             ws.numel() * 4, stream())


def run_wplus(combo, D, Lr, B, acc=0, null=None, tag="wplus"):
    spe, lwn, leam = combo
    g = torch.Generator().manual_seed(1000 * D + 10 * B + Lr)
    x0, dy0 = torch.randn(B, Lr, D, generator=g) * 1.5 + 0.3, torch.randn(B, Lr, D, generator=g)
    P = wplus_params(combo, Lr, D, g)
    Pd = {k: dev(v) for k, v in P.items()}
    eps = f32v(1e-5)
    xd, dyd = dev(x0), dev(dy0)
    n = B * Lr * D
    yv, yp = nanflat(n, F32)
    sv, sp = nanvec(2 * B * Lr)
    assert call_wplus_fwd(xd, yv, B, Lr, D, Pd, eps, sv) == 0, last_error()
    f64 = wplus_formula(x0, None, P, eps, None, F64)
    f32 = wplus_formula(x0, None, P, eps, None, F32)
    c_y = measure_c(f"{tag}.y", "fp32", [(f32["y"], f64["y"], f64["s_y"])])
    assert_close(f"{tag} y", yv, f64["y"], f64["s_y"], c_y, 0.0, extra=f64["x_y"])
    untouched_flat(f"{tag} y", yp, n)
    saved = sv.view(B, Lr, 2)
    if lwn != "none":
        c_m = measure_c(f"{tag}.mean", "fp32", [(f32["mu"], f64["mu"], f64["s_mu"])])
        c_r = measure_c(f"{tag}.rstd", "fp32", [(f32["rs"], f64["rs"], f64["rs"])])
        assert_close(f"{tag} saved mean", saved[..., 0], f64["mu"], f64["s_mu"], c_m, 0.0)
        assert_close(f"{tag} saved rstd", saved[..., 1], f64["rs"], f64["rs"], c_r, 0.0)
    else:
        assert_bits_equal(f"{tag} saved without LWN is (0, 0)", sv, torch.zeros_like(sv))
    untouched_vec(f"{tag} saved", sp, 2 * B * Lr)
    y2 = torch.full((n,), NAN, device=DEV)
    assert call_wplus_fwd(xd, y2, B, Lr, D, Pd, eps, None) == 0, last_error()
    assert_bits_equal(f"{tag} y with saved null", y2, yv.contiguous())

    # ---- backward from the saved statistics of the forward kernel
    st = saved.cpu().double() if lwn != "none" else None
    b64 = wplus_formula(x0, dy0, P, eps, st, F64)
    b32 = wplus_formula(x0, dy0, P, eps, st, F32)
    shapes = dict(d_sg=(3, D), d_sl=(Lr, D), d_lw=(Lr, D), d_lb=(Lr, D), d_gate=(Lr,), d_leam=(Lr,))
    live = dict(d_sg=spe, d_sl=spe, d_lw=lwn != "none", d_lb=lwn != "none", d_gate=lwn == "gate", d_leam=leam)
    init = {k: torch.randn(*shapes[k], generator=g) * 3 for k in WPLUS_OUT}
    outs, par = {}, {}
    for k in WPLUS_OUT:
        v, par[k] = nanvec(int(np.prod(shapes[k])))
        if acc:
            v.copy_(init[k].reshape(-1))
        outs[k] = v if (live[k] and k != null) else None
    dxv, dxp = nanflat(n, F32)
    rc = call_wplus_bwd(xd, sv if lwn != "none" else None, dyd, dxv, B, Lr, D, Pd, eps, outs, acc)
    assert rc == 0, last_error()
    c_dx = measure_c(f"{tag}.dx", "fp32", [(b32["dx"], b64["dx"], b64["s_dx"])])
    assert_close(f"{tag} dx", dxv, b64["dx"], b64["s_dx"], c_dx, 0.0, extra=b64["x_dx"])
    untouched_flat(f"{tag} dx", dxp, n)
    for k in WPLUS_OUT:
        n_k = int(np.prod(shapes[k]))
        if outs[k] is None:
            want = init[k].reshape(-1) if acc else torch.full((n_k,), NAN)
            assert_bits_equal(f"{tag} {k} (null output) left alone", par[k][4:4 + n_k], want.to(DEV))
        else:
            c_k = measure_c(f"{tag}.{k}", "fp32", [(b32[k], b64[k], b64["s_" + k])])
            ref, sca = b64[k], b64["s_" + k]
            ext = b64["x_" + k]
            if acc:
                ref, sca = ref + init[k].double(), sca + init[k].double().abs()
            assert_close(f"{tag} {k}", outs[k], ref, sca, c_k, 0.0, extra=ext)
        untouched_vec(f"{tag} {k}", par[k], n_k)


@pytest.mark.parametrize("cfg", range(len(WPLUS_CONFIGS)))
@pytest.mark.parametrize("combo", WPLUS_COMBOS, ids=lambda c: f"spe{c[0]}-{c[1]}-leam{c[2]}")
def test_wplus_options(combo, cfg):
    """fer_wplus_fwd / fer_wplus_bwd in all 12 option combinations (SPE on / off x {no LWN, LWN, LWN + gate} x LEAM
    on / off; an absent stage is a null pointer), each at every listed D, L, B and accumulate value: y, saved, dx
    and the six parameter gradients per element. wplus_fwd_kernel / wplus_bwd_kernel hold 4 x 256 columns per row:
    D = 4 (one partial trip), 255, 256, 257 (the second trip with one column), 512, 1000, 1024 (all four full).
    L = 18: group indices 0, 1, 2 (six layers each); L = 1: group 2. wplus_bwd_kernel runs min(B, 32) batch
    chunks: B = 33 gives bchunk = 2 and leaves chunks 17..31 empty (they must write zero partials into the
    NaN-filled workspace), B = 70 gives bchunk = 3 with chunks 24..31 empty. Gate and LEAM logits cover
    [-4, 4] and 0. The D = 512 configuration also nulls each gradient output in turn."""
    o = dict(dict(acc=0, nulls=False), **WPLUS_CONFIGS[cfg])
    run_wplus(combo, o["D"], o["Lr"], o["B"], acc=o["acc"])
    if o["nulls"]:
        for k in WPLUS_OUT:
            run_wplus(combo, o["D"], o["Lr"], o["B"], acc=0, null=k, tag=f"wplus.null.{k}")


def test_wplus_too_wide_is_an_error():
    """D = 1028 > 1024 columns per row: fer_wplus_fwd and fer_wplus_bwd both return non-zero with their
    message and write nothing (the backward kernel would leave dx[:, 1024:] unwritten and drop those columns
    from every reduction)."""
    B, Lr, D = 2, 3, 1028
    x = torch.ones(B, Lr, D, device=DEV)
    P = dict(sg=torch.ones(3, D), sl=torch.ones(Lr, D), grp=torch.tensor([0, 1, 2]), lw=torch.ones(Lr, D),
             lb=torch.ones(Lr, D), gate=torch.zeros(Lr), lm=torch.zeros(Lr))
    Pd = {k: dev(v) for k, v in P.items()}
    y = torch.full((B, Lr, D), NAN, device=DEV)
    saved = torch.full((B * Lr * 2,), NAN, device=DEV)
    assert call_wplus_fwd(x, y, B, Lr, D, Pd, 1e-5, saved) != 0 and "wplus_fwd: D <= 1024" in last_error()
    outs = {k: torch.full(s, NAN, device=DEV) for k, s in
            dict(d_sg=(3, D), d_sl=(Lr, D), d_lw=(Lr, D), d_lb=(Lr, D), d_gate=(Lr,), d_leam=(Lr,)).items()}
    dx = torch.full((B, Lr, D), NAN, device=DEV)
    st_in = torch.ones(B * Lr * 2, device=DEV)
    rc = call_wplus_bwd(x, st_in, x, dx, B, Lr, D, Pd, 1e-5, outs, 0)
    assert rc != 0 and "wplus_bwd: D <= 1024" in last_error(), (rc, last_error())
    torch.cuda.synchronize()
    for name, v in dict(outs, y=y, saved=saved, dx=dx).items():
        assert torch.isnan(v).all().item(), f"{name} written by a rejected call"


# ====================================================================== decomposer
def decomp_formula(w, dirs, omode, alpha, dmode, dt):
    """scores = w dirs^T (scale sum |w| |dirs|). e = scores dirs, or scores[best] dirs[best] with best the
    FIRST index of max |scores| (torch.argmax's rule, which the LatentDecomposer module follows); the kernel
    forms e from its own fp32 scores, so an element of e carries sum_c s_score[c] |dirs[c][i]|. id = w - e
    (|w| + s_e); enhanced = id + alpha e (|w| + s_e + |alpha| s_e); concat = (e, id)."""
    w, dirs = w.to(dt), dirs.to(dt)
    # one reduction per (b, c) over identical products in identical order: equal rows give equal bits (the tie test)
    sc, s_sc = (w[:, None, :] * dirs[None]).sum(2), (w[:, None, :] * dirs[None]).abs().sum(2)
    if dmode == 0:
        e, s_e = sc @ dirs, s_sc @ dirs.abs()
    else:
        top = sc.abs() == sc.abs().max(1, keepdim=True).values
        best = torch.where(top, torch.arange(sc.shape[1]), sc.shape[1]).min(1).values  # first maximal index
        e = sc.gather(1, best[:, None]) * dirs[best]
        s_e = s_sc.gather(1, best[:, None]) * dirs[best].abs()
    idv, s_id = w - e, w.abs() + s_e
    y, s_y = {0: (e, s_e), 1: (idv, s_id), 2: (idv + alpha * e, s_id + abs(alpha) * s_e),
              3: (torch.cat([e, idv], 1), torch.cat([s_e, s_id], 1))}[omode]
    return dict(scores=sc, s_scores=s_sc, y=y, s_y=s_y)


def decomp_inputs(B, C, LD, dmode, base_seed):
    """Inputs whose float64 top-two |scores| gap exceeds twice the score bound in every row (max_class): the
    fp32 argmax then cannot legitimately differ from the float64 one. The seed is searched on the CPU and the
    property asserted; no row is skipped."""
    for seed in range(base_seed, base_seed + 64):
        g = torch.Generator().manual_seed(seed)
        w = torch.randn(B, LD, generator=g)
        dirs = torch.randn(C, LD, generator=g) * (torch.rand(C, 1, generator=g) + 0.5) / math.sqrt(LD)
        if dmode == 0 or C == 1:
            return w, dirs
        r64 = decomp_formula(w, dirs, 0, 1.0, 0, F64)
        r32 = decomp_formula(w, dirs, 0, 1.0, 0, F32)
        c = max(16.0, 4.0 * ((r32["scores"].double() - r64["scores"]).abs() / (U * r64["s_scores"])).max().item())
        top = r64["scores"].abs().topk(2, dim=1)
        bound = c * U * r64["s_scores"].gather(1, top.indices)
        if ((top.values[:, 0] - top.values[:, 1]) > 2 * bound.sum(1)).all():
            return w, dirs
    raise AssertionError("no seed with a clear max_class winner in every row")


def run_decompose(B, C, LD, omode, alpha, dmode, w, dirs, scores_only=False, tie=False, tag="decompose"):
    alpha = f32v(alpha)
    wd, dd = dev(w), dev(dirs)
    sv, sp = nanvec(B * C)
    ny = B * LD * (2 if omode == 3 else 1)
    yv, yp = nanflat(ny, F32)
    rc = L().fer_decompose(wd.data_ptr(), dd.data_ptr(), B, C, LD, omode, alpha, dmode,
                           None if scores_only else yv.data_ptr(), sv.data_ptr(), stream())
    assert rc == 0, last_error()
    r64 = decomp_formula(w, dirs, omode, alpha, dmode, F64)
    r32 = decomp_formula(w, dirs, omode, alpha, dmode, F32)
    c_s = measure_c(f"{tag}.scores", "fp32", [(r32["scores"], r64["scores"], r64["s_scores"])])
    assert_close(f"{tag} scores", sv, r64["scores"], r64["s_scores"], c_s, 0.0)
    untouched_vec(f"{tag} scores", sp, B * C)
    if scores_only:
        assert torch.isnan(yp).all().item()
        return
    if dmode == 1 and C > 1 and not tie:  # the clear-winner property the comparison of y rests on
        top = r64["scores"].abs().topk(2, dim=1)
        bound = (c_s * U * r64["s_scores"].gather(1, top.indices)).sum(1)
        assert ((top.values[:, 0] - top.values[:, 1]) > 2 * bound).all()
    c_y = measure_c(f"{tag}.y", "fp32", [(r32["y"], r64["y"], r64["s_y"])])
    assert_close(f"{tag} y", yv, r64["y"], r64["s_y"], max(c_y, c_s), 0.0)
    untouched_flat(f"{tag} y", yp, ny)


@pytest.mark.parametrize("dmode", [0, 1])
@pytest.mark.parametrize("omode", [0, 1, 2, 3])
@pytest.mark.parametrize("C", [1, 7, 16])
@pytest.mark.parametrize("LD", [1, 255, 256, 257, 9216])
def test_decompose_elementwise(LD, C, omode, dmode):
    """fer_decompose: scores and y per element, both decompose modes (0 all_classes, 1 max_class) and the four
    output modes (expr_only, id_only, enhanced, concat). decomp_scores_kernel strides LD by 256 threads with C
    accumulators (LD = 1: one thread; 255 / 256 / 257: the edge of the first trip; 9216 = 18 x 512: 36 trips);
    decomp_out_kernel runs ceil(LD / 256) blocks per sample. B = 1 with alpha = 2.0 and B = 3 with alpha = 0.5;
    y null (scores only) on the first output mode."""
    for B, alpha in ((1, 2.0), (3, 0.5)):
        w, dirs = decomp_inputs(B, C, LD, dmode, 50 * LD + C)
        run_decompose(B, C, LD, omode, alpha, dmode, w, dirs)
        if omode == 0:
            run_decompose(B, C, LD, omode, alpha, dmode, w, dirs, scores_only=True)


def test_decompose_exact_tie_takes_first():
    """max_class with two directions of exactly equal |score|, both above all others. torch.argmax, which the
    LatentDecomposer module applies to |coeff|, returns the first maximal index, and so must
    decomp_out_kernel's `>`. (a) dirs[5] = -dirs[2] with w close to 3 dirs[2]: scores[5] = -scores[2] bit for
    bit (negating every product negates the sum). scores[5] dirs[5] is then the same vector as scores[2]
    dirs[2], so (b) makes the choice visible: dirs[5] = dirs[2] where w is non-zero and 9.0 where w is zero, so
    the two scores are the same sum of the same products while e differs in the tail."""
    B, C, LD = 3, 7, 300
    g = torch.Generator().manual_seed(77)
    dirs = torch.randn(C, LD, generator=g) / math.sqrt(LD)
    dirs[5] = -dirs[2]
    w = 3.0 * dirs[2].expand(B, LD) + 0.01 * torch.randn(B, LD, generator=g)
    r = decomp_formula(w, dirs, 0, 1.0, 1, F64)
    assert (r["scores"][:, 2] == -r["scores"][:, 5]).all() and r["scores"].abs().argmax(1).eq(2).all()
    run_decompose(B, C, LD, 0, 1.0, 1, w, dirs, tie=True, tag="decompose.tie")
    w2 = w.clone()
    w2[:, 200:] = 0.0
    dirs2 = dirs.clone()
    dirs2[5] = dirs[2]
    dirs2[5, 200:] = 9.0
    r2 = decomp_formula(w2, dirs2, 0, 1.0, 1, F64)
    assert (r2["scores"][:, 2] == r2["scores"][:, 5]).all() and r2["scores"].abs().argmax(1).eq(2).all()
    for omode in (0, 3):
        run_decompose(B, C, LD, omode, 1.0, 1, w2, dirs2, tie=True, tag="decompose.tie")


def test_decompose_too_many_directions_is_an_error():
    """C = 17 > 16 accumulators of decomp_scores_kernel: an error, nothing written."""
    B, C, LD = 2, 17, 64
    w, dirs = torch.ones(B, LD, device=DEV), torch.ones(C, LD, device=DEV)
    y, sc = torch.full((B * LD,), NAN, device=DEV), torch.full((B * C,), NAN, device=DEV)
    rc = L().fer_decompose(w.data_ptr(), dirs.data_ptr(), B, C, LD, 0, 1.0, 0, y.data_ptr(), sc.data_ptr(), stream())
    assert rc != 0 and "decompose: at most 16 directions" in last_error()
    torch.cuda.synchronize()
    assert torch.isnan(y).all().item() and torch.isnan(sc).all().item()


# ====================================================================== latent augmentation
def noise_formula(u1, u2, ft):
    """Box-Muller in ft arithmetic from the float32 uniforms: r = sqrt(-2 ln u1), z = r cos(2 pi u2)."""
    u1, u2 = u1.astype(ft), u2.astype(ft)
    r = np.sqrt(ft(-2.0) * np.log(u1))
    return r, r * np.cos(ft(2.0 * math.pi) * u2)


def run_augment(B, LD, noise_std, lo, hi, mask_prob, seed=20240607, zero_x=False):
    n = B * LD
    noise_std, lo, hi, mask_prob = (np.float32(v) for v in (noise_std, lo, hi, mask_prob))
    g = torch.Generator().manual_seed(LD + B)
    x0 = torch.zeros(n) if zero_x else torch.randn(n, generator=g)
    xv, xp = nanflat(n, F32, x0)
    rc = L().fer_latent_augment(xv.data_ptr(), B, LD, float(noise_std), float(lo), float(hi), float(mask_prob), seed,
                                stream())
    assert rc == 0, last_error()
    got = xv.cpu()
    untouched_flat("augment x", xp, n)
    do_noise, do_scale, do_mask = noise_std > 0, (hi > lo or lo != 1), mask_prob > 0
    u1, u2, um, us = dropmask.augment_draws(seed, n, B)
    keep = torch.from_numpy(um > mask_prob) if do_mask else torch.ones(n, dtype=torch.bool)
    if do_mask:  # the zero pattern is exact: dropped elements are +0.0
        assert_bits_equal("augment dropped elements are +0.0", got[~keep], torch.zeros(int((~keep).sum())))
        assert 0 < int((~keep).sum()) < n or n < 8
    if not (do_noise or do_scale):
        assert_bits_equal("augment: elements no stage touches keep their bits", got[keep], x0[keep])
        return
    x64 = x0.double()
    v, bound = x64, torch.zeros(n, dtype=F64)
    if do_noise:
        r64, z64 = noise_formula(u1, u2, np.float64)
        _, z32 = noise_formula(u1, u2, np.float32)
        s_noise = float(noise_std) * (r64 + np.abs(z64))
        c = measure_c("augment.noise", "fp32", [(float(noise_std) * z32.astype(np.float64), float(noise_std) * z64,
                                                 s_noise)])
        v = x64 + float(noise_std) * torch.from_numpy(z64)
        # the issue's scale for the noise, and one rounding (half an ulp) of the sum x + noise
        bound = c * U * torch.from_numpy(s_noise) + 0.5 * U * v.abs()
    if do_scale:
        s32 = (lo + (hi - lo) * us).astype(np.float32)  # float32 host value of the per-sample scale
        s = torch.from_numpy(s32.astype(np.float64)).repeat_interleave(LD)
        ulp = torch.from_numpy(np.spacing(s32).astype(np.float64)).repeat_interleave(LD)
        # the kernel's scale within 2 ulps of s32 (the multiply-add may be contracted), one product rounding
        bound = bound * s + v.abs() * 2 * ulp + U * (v * s).abs()
        v = v * s
    assert_close("augment x", got[keep], v[keep], torch.zeros(int(keep.sum())), 0.0, 0.0, extra=bound[keep])


AUG_STAGES = {"noise": (0.05, 1.0, 1.0, 0.0), "scale": (0.0, 0.8, 1.2, 0.0), "mask": (0.0, 1.0, 1.0, 0.1),
              "all": (0.05, 0.8, 1.2, 0.1), "none": (0.0, 1.0, 1.0, 0.0)}


@pytest.mark.parametrize("stage", sorted(AUG_STAGES))
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("LD", [1, 512, 9216])
def test_latent_augment_stages(LD, B, stage):
    """fer_latent_augment against the host replica of its draws (dropmask.u01 / sub_seeds / augment_draws), each
    stage alone, all three, and none (noise_std = 0, scale_lo = scale_hi = 1, mask_prob = 0: x keeps its bits).
    noise: x + noise_std r cos(2 pi u2), bound c 2^-23 noise_std (r + |z|) + 2^-24 |ref| (the one rounding of the
    sum), c measured from the float32 numpy evaluation of the formula (with x = 0 as well); scale: the per-sample factor
    within 2 fp32 ulps of the float32 host value; mask: the zero pattern exact, survivors untouched."""
    run_augment(B, LD, *AUG_STAGES[stage])
    if stage == "noise":
        run_augment(B, LD, *AUG_STAGES[stage], zero_x=True)


def test_latent_augment_grid_stride():
    """n = 228 x 9216 = 2,101,248 > 8192 x 256 elements: latent_augment_kernel's grid-stride loop, all stages."""
    assert 228 * 9216 > CAP
    run_augment(228, 9216, *AUG_STAGES["all"])
