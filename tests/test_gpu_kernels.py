"""Kernel-level parity on the GPU: every libfervit op vs a plain fp32 torch reference of
the same op on the same inputs (bf16 path with bf16-appropriate tolerances; the fp32 path
tight). Dropout masks are rebuilt on the host from the kernel's hash (tests/dropmask.py),
so dropout paths are checked element-exactly too."""
import math

import numpy as np

import pytest
import torch

from dropmask import keep_mask

pytestmark = pytest.mark.gpu

DEV = "cuda"


def ops():
    from fervit import ops as o

    return o


def rel_err(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def bf(t):
    return t.to(DEV, torch.bfloat16)


# ---------------------------------------------------------------------- GEMM
GEMM_SHAPES = [(64, 64, 64), (300, 136, 200), (1000, 768, 768), (512, 2304, 768), (4864, 512, 2048),
               (777, 3072, 776)]


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_linear_fwd_dgrad_wgrad(M, N, K, dtype):
    o = ops()
    g = torch.Generator().manual_seed(M * 7 + N)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    dy = torch.randn(M, N, generator=g)
    cast = bf if dtype == "bf16" else (lambda t: t.to(DEV))
    xr, wr, dyr = (cast(t).float().cpu().double() for t in (x, w, dy))
    tol = 1e-2 if dtype == "bf16" else 1e-5
    y = o.linear_fwd(cast(x), cast(w))
    assert rel_err(y.cpu(), xr @ wr.t()) < tol
    dx = o.linear_dgrad(cast(dy), cast(w))
    assert rel_err(dx.cpu(), dyr @ wr) < tol
    gw = torch.zeros(N, K, device=DEV)
    o.linear_wgrad(cast(dy), cast(x), gw)
    assert rel_err(gw.cpu(), dyr.t() @ xr) < tol
    o.linear_wgrad(cast(dy), cast(x), gw, accumulate=True)
    assert rel_err(gw.cpu(), 2 * (dyr.t() @ xr)) < tol


@pytest.mark.parametrize("M,N,K", [(20000, 3000, 520), (9000, 2048, 40), (70000, 768, 136), (25500, 768, 768)])
def test_gemm_persistent_many_tiles(M, N, K):
    """More 256x256 tiles than CUs: each persistent workgroup walks several tiles, prefetching the
    next tile's first K-tile during the epilogue (plain kind) or not, plus the fused column sums
    and the residual kind with dropout (exact keep pattern). fp32 torch matmul on the GPU as
    reference."""
    o = ops()
    g = torch.Generator(device=DEV).manual_seed(M + K)
    x = torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, device=DEV, generator=g) / math.sqrt(K)).to(torch.bfloat16)
    b = torch.randn(N, device=DEV, generator=g)
    res = torch.randn(M, N, device=DEV, generator=g).to(torch.bfloat16)
    ref = x.float() @ w.float().t()
    y = o.linear_fwd(x, w)
    assert rel_err(y, ref) < 1e-2
    pre = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
    cs = torch.zeros(N, device=DEV)
    y2 = o.linear_fwd(x, w, b, pre=pre, act="gelu", colsum=cs)
    assert rel_err(pre, ref + b) < 1e-2
    gl = torch.nn.functional.gelu(ref + b)
    assert rel_err(y2, gl) < 1e-2
    assert rel_err(cs, y2.float().sum(0)) < 1e-3
    y3 = o.linear_fwd(x, w, b, res=res)
    assert rel_err(y3, ref + b + res.float()) < 1e-2
    # deterministic across calls
    assert torch.equal(o.linear_fwd(x, w), y)
    # dropout keep bits (hashed inside the main loop): exact pattern against the host replica,
    # on a strictly positive pre-activation so that an output is 0 iff it was dropped
    xp, wp = x.abs() + 0.01, (w.abs() + 0.01).to(torch.bfloat16)
    xp = xp.to(torch.bfloat16)
    yd = o.linear_fwd(xp, wp, act="relu", dropout=0.1, seed=77)
    keep = keep_mask(77, (M, N), 0.1).to(DEV)
    assert torch.equal(yd != 0, keep)
    # the residual kind with dropout (out-proj / fc2 forward): drop(acc + b) + res
    rz = torch.zeros(M, N, device=DEV, dtype=torch.bfloat16)
    bp = b.abs() + 0.01
    yr = o.linear_fwd(xp, wp, bp, res=rz, dropout=0.1, seed=78)
    keep = keep_mask(78, (M, N), 0.1).to(DEV)
    assert torch.equal(yr != 0, keep)
    refp = (xp.float() @ wp.float().t() + bp) / 0.9
    assert rel_err(torch.where(keep, yr.float(), refp), refp) < 1e-2


@pytest.mark.parametrize("K", [768, 2048])
def test_gemm_last_round_split(K):
    """300 tiles of 256x256 on the persistent grid (two whole rounds and a last round under half full,
    the shape class of every N = 768 ViT-B linear): the fixed kinds -- GELU gate with dropout,
    residual with dropout, gate multiply with column sums -- against fp32 torch on the GPU with the
    host-rebuilt keep masks, and bit-identical across calls. (Splitting the last round along K in the
    launch passed this test and was not kept: DESIGN.md section 9.)"""
    o = ops()
    M, N, p = 25600, 768, 0.1
    g = torch.Generator(device=DEV).manual_seed(K)
    x = torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, device=DEV, generator=g) / math.sqrt(K)).to(torch.bfloat16)
    b = torch.randn(N, device=DEV, generator=g)
    h = x.float() @ w.float().t() + b
    keep = keep_mask(91, (M, N), p).to(DEV)
    # GELU gate (fc1 forward)
    gate = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
    y = o.linear_fwd(x, w, b, pre=gate, pre_gate=True, act="gelu", dropout=p, seed=91)
    hr = h.clone().requires_grad_(True)
    a = torch.nn.functional.gelu(hr)
    a.backward(torch.ones_like(a))
    assert rel_err(y, torch.where(keep, a.detach() / (1 - p), torch.zeros((), device=DEV))) < 1e-2
    assert rel_err(gate, torch.where(keep, hr.grad / (1 - p), torch.zeros((), device=DEV))) < 1e-2
    y2 = o.linear_fwd(x, w, b, pre=torch.empty_like(gate), pre_gate=True, act="gelu", dropout=p, seed=91)
    assert torch.equal(y, y2)
    # residual with dropout (out-proj / fc2 forward)
    res = torch.randn(M, N, device=DEV, generator=g).to(torch.bfloat16)
    yr = o.linear_fwd(x, w, b, res=res, dropout=p, seed=91)
    ref = torch.where(keep, h / (1 - p), torch.zeros((), device=DEV)) + res.float()
    assert rel_err(yr, ref) < 1e-2
    assert torch.equal(o.linear_fwd(x, w, b, res=res, dropout=p, seed=91), yr)
    # gate multiply with fused column sums (fc2 input gradient)
    cs = torch.zeros(N, device=DEV)
    ym = o.linear_fwd(x, w, aux=gate, aux_act="mul", colsum=cs)
    refm = (x.float() @ w.float().t()) * gate.float()
    assert rel_err(ym, refm) < 1e-2
    assert rel_err(cs, ym.float().sum(0)) < 1e-3


@pytest.mark.parametrize("cfg", [3, 5, 8, 11])
def test_gemm_every_tile_config(cfg):
    """Each bf16 kernel configuration (forced through fer_gemm_set_config) on ragged shapes,
    all three operand layouts, split-K, and the fused epilogue."""
    from fervit._lib import lib

    o = ops()
    lib().fer_gemm_set_config(cfg)
    try:
        # (K = 24: a single K-step; the ring kernel's K loop runs two K-steps per trip, odd counts included)
        for M, N, K in [(300, 136, 200), (777, 520, 1096), (2056, 264, 520), (130, 72, 24)]:
            g = torch.Generator().manual_seed(M + cfg)
            x = torch.randn(M, K, generator=g)
            w = torch.randn(N, K, generator=g) / math.sqrt(K)
            dy = torch.randn(M, N, generator=g)
            b = torch.randn(N, generator=g)
            xr, wr, dyr = (bf(t).float().cpu().double() for t in (x, w, dy))
            y = o.linear_fwd(bf(x), bf(w), b.to(DEV), act="relu")
            assert rel_err(y.cpu(), torch.relu(xr @ wr.t() + b.double())) < 1e-2, (cfg, M, N, K)
            assert rel_err(o.linear_dgrad(bf(dy), bf(w)).cpu(), dyr @ wr) < 1e-2, (cfg, M, N, K)
            gw = torch.zeros(N, K, device=DEV)
            o.linear_wgrad(bf(dy), bf(x), gw)
            assert rel_err(gw.cpu(), dyr.t() @ xr) < 1e-2, (cfg, M, N, K)
    finally:
        lib().fer_gemm_set_config(-1)


@pytest.mark.parametrize("act", ["gelu", "relu"])
def test_gemm_epilogue_bias_act_dropout_residual(act):
    o = ops()
    M, N, K, p, seed = 1030, 640, 384, 0.1, 12345
    g = torch.Generator().manual_seed(1)
    x, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / math.sqrt(K)
    b, r = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    pre = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
    y = o.linear_fwd(bf(x), bf(w), b.to(DEV), pre=pre, act=act, dropout=p, seed=seed, res=bf(r))
    xr, wr, rr = (bf(t).float().cpu() for t in (x, w, r))
    h = xr @ wr.t() + b
    a = torch.nn.functional.gelu(h) if act == "gelu" else torch.relu(h)
    keep = keep_mask(seed, (M, N), p)
    ref = torch.where(keep, a / (1 - p), torch.zeros(())) + rr
    assert rel_err(pre.cpu(), h) < 1e-2
    assert rel_err(y.cpu(), ref) < 1e-2
    # dgrad through dropout + activation derivative (aux), as in the FFN backward
    dy = torch.randn(M, K, generator=g)
    w2 = torch.randn(K, N, generator=g) / math.sqrt(N)  # [out=K, in=N]
    cs = torch.zeros(N, device=DEV)  # fused linear1.bias gradient (column sums of dF)
    dF = o.linear_dgrad(bf(dy), bf(w2), dropout=p, seed=seed, drop_ld=N, aux=pre, aux_act=act, colsum=cs)
    dyr, w2r, hr = bf(dy).float().cpu(), bf(w2).float().cpu(), pre.float().cpu()
    hh = hr.clone().requires_grad_(True)
    aa = torch.nn.functional.gelu(hh) if act == "gelu" else torch.relu(hh)
    dG = dyr @ w2r
    aa.backward(torch.where(keep, dG / (1 - p), torch.zeros(())))
    assert rel_err(dF.cpu(), hh.grad) < 2e-2
    assert rel_err(cs.cpu(), hh.grad.sum(0)) < 2e-2


@pytest.mark.parametrize("drop_ld", [640, 644])
@pytest.mark.parametrize("kind", ["gate", "res"])
def test_gemm_epilogue_keep_bits_exact(kind, drop_ld):
    """Every keep decision of the fused epilogues, element for element: the fixed kinds hash 8-element
    pieces with keep8a when drop_ld % 8 == 0 (640); 644 takes the generic epilogue (csrc/gemm.hip
    epi_kind). GATE: the output is exactly 0 where dropped and non-zero where kept (GELU of a
    continuous pre-activation); RES: y - res isolates the dropped term (exactly 0 where dropped)."""
    o = ops()
    M, N, K, p, seed = 1030, 640, 384, 0.1, 0x1234_5678_9ABC
    g = torch.Generator().manual_seed(11)
    x, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / math.sqrt(K)
    b = torch.randn(N, generator=g)
    keep = keep_mask(seed, (M, drop_ld), p)[:, :N]
    h = bf(x).float().cpu() @ bf(w).float().cpu().t() + b
    live = h.abs() < 4  # GELU's fp32 tail below about -5.3 rounds to exactly 0: not a keep decision
    assert live.float().mean() > 0.99
    if kind == "gate":
        gate = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
        y = o.linear_fwd(bf(x), bf(w), b.to(DEV), pre=gate, pre_gate=True, act="gelu", dropout=p, seed=seed,
                         drop_ld=drop_ld).float().cpu()
        got = y != 0
    else:
        res = torch.zeros(M, N, device=DEV, dtype=torch.bfloat16)  # y = drop(xW^T + b) exactly
        y = o.linear_fwd(bf(x), bf(w), b.to(DEV), res=res, dropout=p, seed=seed, drop_ld=drop_ld).float().cpu()
        got = y != 0
    assert torch.equal(got[live], keep[live]), int((got != keep)[live].sum())


@pytest.mark.parametrize("act", ["gelu", "relu"])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_gemm_pre_gate_and_mul(act, dtype, p):
    """pre_gate: `pre` receives act'(h) * keep / (1 - p) (the same keep bits as the output's
    dropout); the FFN input-gradient GEMM then multiplies by it (aux_act="mul") -- equal to the
    dropout + act' epilogue of test_gemm_epilogue_bias_act_dropout_residual (csrc/gemm.hip)."""
    o = ops()
    M, N, K, seed = 1030, 640, 384, 2468
    g = torch.Generator().manual_seed(7)
    x, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / math.sqrt(K)
    b = torch.randn(N, generator=g)
    cast = bf if dtype == "bf16" else (lambda t: t.to(DEV))
    tol = 1e-2 if dtype == "bf16" else 1e-5
    gate = torch.empty(M, N, device=DEV, dtype=cast(x).dtype)
    y = o.linear_fwd(cast(x), cast(w), b.to(DEV), pre=gate, pre_gate=True, act=act, dropout=p, seed=seed)
    xr, wr = cast(x).float().cpu(), cast(w).float().cpu()
    hh = (xr @ wr.t() + b).requires_grad_(True)
    a = torch.nn.functional.gelu(hh) if act == "gelu" else torch.relu(hh)
    keep = keep_mask(seed, (M, N), p) if p > 0 else torch.ones(M, N, dtype=torch.bool)
    assert rel_err(y.cpu(), torch.where(keep, a / (1 - p), torch.zeros(()))) < tol
    a.backward(torch.ones_like(a))
    assert rel_err(gate.cpu(), torch.where(keep, hh.grad / (1 - p), torch.zeros(()))) < tol
    dy = torch.randn(M, K, generator=g)
    w2 = torch.randn(K, N, generator=g) / math.sqrt(N)
    cs = torch.zeros(N, device=DEV)
    dF = o.linear_dgrad(cast(dy), cast(w2), aux=gate, aux_act="mul", colsum=cs)
    ref = (cast(dy).float().cpu() @ cast(w2).float().cpu()) * gate.float().cpu()
    assert rel_err(dF.cpu(), ref) < 2 * tol
    assert rel_err(cs.cpu(), ref.sum(0)) < 2 * tol


@pytest.mark.parametrize("cfg", [8, 3, 11])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_gemm_8phase_epilogue_kinds(p, cfg):
    """The 8-phase kernel's fixed-flag epilogues (csrc/gemm.hip epi_kind: EPI_STORE, EPI_GATE,
    EPI_RES2, EPI_MUL2; and the 128^2 / 128x64 kernels', cfg 3 / 11), forced through fer_gemm_set_config on a ragged shape (partial last
    tile row and column, K tail): the calls the post-norm layer makes (fervit/layers.py
    PostNormLayerFn), each against an fp32 torch reference with the host-rebuilt keep mask."""
    from fervit._lib import lib

    o = ops()
    M, N, K, seed = 1100, 520, 200, 4321
    g = torch.Generator().manual_seed(11)
    x, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / math.sqrt(K)
    b, r = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    xr, wr, rr = (bf(t).float().cpu() for t in (x, w, r))
    h = xr @ wr.t() + b
    keep = keep_mask(seed, (M, N), p) if p > 0 else torch.ones(M, N, dtype=torch.bool)
    lib().fer_gemm_set_config(cfg)
    try:
        # EPI_STORE: bias only (qkv fwd), and no epilogue at all (out-proj dgrad)
        assert rel_err(o.linear_fwd(bf(x), bf(w), b.to(DEV)).cpu(), h) < 1e-2
        assert rel_err(o.linear_fwd(bf(x), bf(w)).cpu(), xr @ wr.t()) < 1e-2
        # EPI_GATE: fc1 fwd, GELU + dropout, pre = GELU'(h) * keep / (1 - p)
        gate = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
        y = o.linear_fwd(bf(x), bf(w), b.to(DEV), pre=gate, pre_gate=True, act="gelu", dropout=p, seed=seed,
                         drop_ld=N)
        hh = h.clone().requires_grad_(True)
        a = torch.nn.functional.gelu(hh)
        a.backward(torch.ones_like(a))
        assert rel_err(y.cpu(), torch.where(keep, a.detach() / (1 - p), torch.zeros(()))) < 1e-2
        assert rel_err(gate.cpu(), torch.where(keep, hh.grad / (1 - p), torch.zeros(()))) < 1e-2
        # EPI_GATER: fc1 fwd of the ReLU encoders (LatentViT), pre = (h > 0) * keep / (1 - p)
        gr = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
        yr = o.linear_fwd(bf(x), bf(w), b.to(DEV), pre=gr, pre_gate=True, act="relu", dropout=p, seed=seed,
                          drop_ld=N)
        assert rel_err(yr.cpu(), torch.where(keep, torch.relu(h) / (1 - p), torch.zeros(()))) < 1e-2
        gref = torch.where(keep & (h > 0), torch.full_like(h, 1 / (1 - p)), torch.zeros(())).to(torch.bfloat16)
        assert (gr.cpu() != gref).float().mean().item() < 1e-3  # sign flips of |h| ~ 0 only
        # EPI_RES2: out-proj / fc2 fwd, bias + dropout + residual (and the residual-only dgrad form)
        z = o.linear_fwd(bf(x), bf(w), b.to(DEV), res=bf(r), dropout=p, seed=seed, drop_ld=N)
        assert rel_err(z.cpu(), torch.where(keep, h / (1 - p), torch.zeros(())) + rr) < 1e-2
        z2 = o.linear_fwd(bf(x), bf(w), res=bf(r))
        assert rel_err(z2.cpu(), xr @ wr.t() + rr) < 1e-2
        # EPI_MUL2: fc2 dgrad through the gate, with the fused bias-gradient column sums
        cs = torch.zeros(N, device=DEV)
        dF = o.linear_fwd(bf(x), bf(w), aux=gate, aux_act="mul", colsum=cs)
        ref = (xr @ wr.t()) * gate.float().cpu()
        assert rel_err(dF.cpu(), ref) < 1e-2
        assert rel_err(cs.cpu(), ref.sum(0)) < 2e-2
    finally:
        lib().fer_gemm_set_config(-1)


def test_gemm_keep_rate():
    o = ops()
    M, N, K = 512, 1024, 64
    x = torch.ones(M, K, device=DEV, dtype=torch.bfloat16)
    w = torch.full((N, K), 1.0 / K, device=DEV, dtype=torch.bfloat16)
    y = o.linear_fwd(x, w, dropout=0.1, seed=99).float()
    frac = (y != 0).float().mean().item()
    assert abs(frac - 0.9) < 0.005
    assert torch.allclose(y[y != 0], torch.full_like(y[y != 0], 1 / 0.9), rtol=1e-2)


# ---------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("D", [128, 384, 512, 768, 1024])
def test_layernorm_fwd_bwd(dtype, D):
    o = ops()
    M = 1000
    g = torch.Generator().manual_seed(D)
    x = torch.randn(M, D, generator=g) * 2 + 0.5
    w, b = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    dy, res = torch.randn(M, D, generator=g), torch.randn(M, D, generator=g)
    cast = bf if dtype == "bf16" else (lambda t: t.to(DEV))
    tol = 1e-2 if dtype == "bf16" else 1e-5
    xd = cast(x)
    mean = torch.empty(M, device=DEV)
    rstd = torch.empty(M, device=DEV)
    y = o.layernorm_fwd(xd, w.to(DEV), b.to(DEV), 1e-5, mean=mean, rstd=rstd)
    xr = xd.float().cpu().requires_grad_(True)
    wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    yr = torch.nn.functional.layer_norm(xr, (D,), wr, br, 1e-5)
    assert rel_err(y.cpu(), yr) < tol
    p, seed = 0.1, 777
    dyd = cast(dy)
    gw = torch.zeros(D, device=DEV)
    gb = torch.zeros(D, device=DEV)
    gbias = torch.zeros(D, device=DEV)
    dxd = torch.empty_like(xd)
    dx = o.layernorm_bwd(dyd, xd, mean, rstd, w.to(DEV), res=cast(res), dx_drop=dxd, dropout=p, seed=seed, dgamma=gw,
                         dbeta=gb, dbias=gbias)
    yr.backward(dyd.float().cpu())
    dx_ref = xr.grad + cast(res).float().cpu()
    assert rel_err(dx.cpu(), dx_ref) < tol
    keep = keep_mask(seed, (M, D), p)
    dxd_ref = torch.where(keep, dx_ref / (1 - p), torch.zeros(()))
    assert rel_err(dxd.cpu(), dxd_ref) < tol
    assert rel_err(gw.cpu(), wr.grad) < 1e-4 + tol
    assert rel_err(gb.cpu(), br.grad) < 1e-4 + tol
    # kernel sums the fp32 values before the bf16 rounding of dx_drop
    assert rel_err(gbias.cpu(), dxd.float().cpu().sum(0)) < (5e-3 if dtype == "bf16" else 1e-5)


# ---------------------------------------------------------------------- attention
def attn_ref(qkv, B, N, H, dh, keep=None, p=0.0):
    D = H * dh
    q, k, v = qkv.view(B, N, 3, H, dh).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) / math.sqrt(dh)
    P = torch.softmax(s, -1)
    lse = torch.logsumexp(s, -1)
    Pd = P if keep is None else torch.where(keep, P / (1 - p), torch.zeros(()))
    out = (Pd @ v).permute(0, 2, 1, 3).reshape(B * N, D)
    return out, lse


@pytest.mark.parametrize("splits", [0, 1, 2, 3])
def test_wgrad_group(splits):
    """One grouped launch of several weight gradients sharing the token count (csrc/gemm.hip
    gemm_wgrad_group_kernel): ragged tiles (N, K not multiples of 128), padded row strides,
    accumulate on / off, K split 1-3 with the in-launch ordered reduction; against fp32 torch,
    bit-identical on a repeat (the split reduction's order does not depend on arrival)."""
    o = ops()
    M = 1000
    g = torch.Generator(device=DEV).manual_seed(11 + splits)
    shapes = [(256, 128, False), (136, 200, True), (384, 512, False), (64, 8, True), (520, 264, False)]
    items, refs = [], []
    for N, K, acc in shapes:
        dy = torch.randn(M, N + 8, device=DEV, generator=g).to(torch.bfloat16)[:, :N]  # row stride N + 8
        x = torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16)
        out = torch.randn(N, K, device=DEV, generator=g) if acc else torch.full((N, K), float("nan"), device=DEV)
        ref = dy.float().t() @ x.float() + (out if acc else 0)
        items.append((dy, x, out, acc))
        refs.append(ref)
    init = [it[2].clone() for it in items]
    o.linear_wgrad_group(items, splits=splits)
    torch.cuda.synchronize()
    for (dy, x, out, acc), ref in zip(items, refs):
        assert rel_err(out, ref) < 1e-5, (dy.shape, x.shape, acc)
    first = [it[2].clone() for it in items]
    for it, i0 in zip(items, init):
        it[2].copy_(i0)
    o.linear_wgrad_group(items, splits=splits)
    for it, f in zip(items, first):
        assert torch.equal(it[2], f)


@pytest.mark.parametrize("N,H,dh", [(10, 8, 48), (19, 8, 64), (37, 12, 64), (197, 12, 64), (19, 6, 64), (100, 4, 64),
                                    (150, 3, 32), (250, 2, 64),
                                    # general path (csrc/attention.hip attn_*_gen): dh > 64 or N > 256
                                    (19, 4, 128), (37, 8, 96), (257, 12, 64), (300, 2, 128), (130, 3, 80)])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_attention_fwd_bwd(N, H, dh, dtype, p):
    o = ops()
    B = 3 if N >= 197 else 8
    D = H * dh
    seed = 4242
    g = torch.Generator().manual_seed(N * 100 + dh)
    qkv = torch.randn(B * N, 3 * D, generator=g)
    dout = torch.randn(B * N, D, generator=g)
    cast = bf if dtype == "bf16" else (lambda t: t.to(DEV))
    tol = 2e-2 if dtype == "bf16" else 1e-4
    qd = cast(qkv)
    out = torch.empty(B * N, D, device=DEV, dtype=qd.dtype)
    saved = o.attention_saved(qd, B, N, H, dh, dropout=p)
    lse = saved[:B * H * N]
    o.attention_fwd(qd, out, saved, B, N, H, dh, dropout=p, seed=seed)
    # attention dropout index: (bh*N + q)*NP + k, NP = N rounded up to even (csrc/attention.hip)
    keep = keep_mask(seed, (B, H, N, N + (N & 1)), p)[..., :N] if p > 0 else None
    qr = qd.float().cpu().requires_grad_(True)
    ref, lse_ref = attn_ref(qr, B, N, H, dh, keep, p)
    assert rel_err(out.cpu(), ref) < tol
    assert (lse.cpu() - lse_ref.reshape(-1)).abs().max().item() < (2e-2 if dtype == "bf16" else 1e-4)
    nb = (N + 31) // 32
    if p > 0 and saved.numel() > B * H * N + 63:
        # persistent bf16 path: keep bits stored for the backward, word (kb, qb, j) = bits over the
        # 32 queries of block qb for key kb*32 + j (csrc/attention.hip attn_fwd_pers)
        off = (B * H * N + 63) // 64 * 64
        words = saved[off:off + B * H * nb * nb * 32].view(torch.int32).cpu().numpy().view(np.uint32)
        words = words.reshape(B * H, nb, nb, 32).astype(np.uint64)
        bits = (words[..., None] >> np.arange(32, dtype=np.uint64)) & np.uint64(1)  # [bh][kb][qb][j][qi]
        got = torch.from_numpy(bits.transpose(0, 2, 4, 1, 3).reshape(B * H, nb * 32, nb * 32).astype(bool))
        want = keep.reshape(B * H, N, N)
        assert torch.equal(got[:, :N, :N], want)
    dd = cast(dout)
    dqkv = torch.empty_like(qd)
    cs = torch.full((3 * D,), 0.5, device=DEV)  # fused in_proj.bias gradient, accumulated
    o.attention_bwd(qd, out, dd, saved, dqkv, B, N, H, dh, dropout=p, seed=seed, colsum=cs, colsum_accumulate=True)
    ref.backward(dd.float().cpu())
    assert rel_err(cs.cpu() - 0.5, qr.grad.sum(0)) < 2 * tol
    for j, name in enumerate("qkv"):
        a = dqkv.cpu().float()[:, j * D:(j + 1) * D]
        b = qr.grad[:, j * D:(j + 1) * D]
        assert rel_err(a, b) < 2 * tol, name
    # deterministic: a second backward reproduces every bit (fixed-order dQ / bias sums)
    dqkv2 = torch.empty_like(qd)
    cs2 = torch.full((3 * D,), 0.5, device=DEV)
    o.attention_bwd(qd, out, dd, saved, dqkv2, B, N, H, dh, dropout=p, seed=seed, colsum=cs2, colsum_accumulate=True)
    assert torch.equal(dqkv2, dqkv) and torch.equal(cs2, cs)


@pytest.mark.parametrize("N,H,dh,B", [(197, 12, 64, 64), (19, 8, 64, 512)])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_attention_persistent_multi_unit(N, H, dh, B, p):
    """The headline configuration's persistent attention path with several (batch, head) units per
    workgroup: B*H = 768 units on 256 workgroups (N = 197) / 4096 units on CUs x occupancy <= 1024
    workgroups (N = 19: several one-wave workgroups per CU), so every workgroup walks >= 3 units
    (next-unit K/V prefetch into the second LDS buffer, work-queue claims). Forward output, lse,
    the stored keep bits, dQ/dK/dV and the fused in_proj bias gradient against a torch fp32
    reference on the GPU, under the work queue (mode 0) and the fixed stride (mode 1), which must
    also agree bit for bit (csrc/attention.hip attn_fwd_pers / attn_bwd_pers)."""
    from dropmask import keep_mask_torch
    from fervit._lib import lib

    o = ops()
    D = H * dh
    seed = 777 + N
    g = torch.Generator(device=DEV).manual_seed(B * N + H)
    qkv = torch.randn(B * N, 3 * D, device=DEV, generator=g).to(torch.bfloat16)
    dout = torch.randn(B * N, D, device=DEV, generator=g).to(torch.bfloat16)
    keep = keep_mask_torch(seed, (B, H, N, N + (N & 1)), p)[..., :N] if p > 0 else None
    qr = qkv.float().requires_grad_(True)
    ref, lse_ref = attn_ref(qr, B, N, H, dh, keep, p)
    ref.backward(dout.float())
    results = []
    for mode in (0, 1):
        lib().fer_set_persistent_mode(mode)
        try:
            out = torch.empty(B * N, D, device=DEV, dtype=torch.bfloat16)
            saved = o.attention_saved(qkv, B, N, H, dh, dropout=p)
            o.attention_fwd(qkv, out, saved, B, N, H, dh, dropout=p, seed=seed)
            dqkv = torch.empty_like(qkv)
            cs = torch.zeros(3 * D, device=DEV)
            o.attention_bwd(qkv, out, dout, saved, dqkv, B, N, H, dh, dropout=p, seed=seed, colsum=cs)
            torch.cuda.synchronize()
        finally:
            lib().fer_set_persistent_mode(0)
        assert rel_err(out, ref) < 2e-2, mode
        assert (saved[:B * H * N] - lse_ref.reshape(-1)).abs().max().item() < 2e-2, mode
        if p > 0:
            nb = (N + 31) // 32
            off = (B * H * N + 63) // 64 * 64
            words = saved[off:off + B * H * nb * nb * 32].view(torch.int32).view(B * H, nb, nb, 32).to(torch.int64)
            words &= 0xFFFFFFFF
            bits = (words[..., None] >> torch.arange(32, device=DEV)) & 1  # [bh][kb][qb][j][qi]
            got = bits.permute(0, 2, 4, 1, 3).reshape(B * H, nb * 32, nb * 32).bool()[:, :N, :N]
            assert torch.equal(got, keep.reshape(B * H, N, N)), mode
        for j, name in enumerate("qkv"):
            assert rel_err(dqkv[:, j * D:(j + 1) * D], qr.grad[:, j * D:(j + 1) * D]) < 4e-2, (mode, name)
        assert rel_err(cs, qr.grad.sum(0)) < 4e-2, mode
        # the saved state's alignment padding is never written: compare lse and the keep words only
        nw = B * H * ((N + 31) // 32) ** 2 * 32 if p > 0 else 0
        off = (B * H * N + 63) // 64 * 64
        # (the keep words compared as integers: as floats most of them are NaN bit patterns)
        results.append((out, saved[:B * H * N], saved[off:off + nw].view(torch.int32), dqkv, cs))
    for a, b in zip(*results):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_head_dropout_keep_mask(dtype):
    """Classification head with train-mode dropout between its LayerNorm and Linear (the hybrid
    head `hybrid_latent_vit.py:110-114`: LayerNorm -> Dropout(0.1) -> Linear) through
    fer_head_fwd / fer_head_bwd, against torch with the host-rebuilt keep mask (element index
    b*D + d): logits, d(CLS rows), zeroed other rows, and the LN / Linear parameter gradients."""
    o = ops()
    B, N, D, C, p, seed = 37, 5, 768, 7, 0.1, 31337
    g = torch.Generator().manual_seed(3)
    cast = bf if dtype == "bf16" else (lambda t: t.to(DEV))
    t = cast(torch.randn(B * N, D, generator=g))
    lnw, lnb = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    W, b = torch.randn(C, D, generator=g) / math.sqrt(D), torch.randn(C, generator=g)
    dl = torch.randn(B, C, generator=g)
    logits, stats = o.head_fwd(t, N, lnw.to(DEV), lnb.to(DEV), 1e-5, W.to(DEV), b.to(DEV), B, dropout=p, seed=seed)
    keep = keep_mask(seed, (B, D), p)
    tr = t.float().cpu().requires_grad_(True)
    P = [x.clone().requires_grad_(True) for x in (lnw, lnb, W, b)]
    cls = tr.view(B, N, D)[:, 0]
    h = torch.nn.functional.layer_norm(cls, (D,), P[0], P[1], 1e-5)
    hd = torch.where(keep, h / (1 - p), torch.zeros(()))
    ref = hd @ P[2].t() + P[3]
    tol = 1e-2 if dtype == "bf16" else 1e-5
    assert rel_err(logits.cpu(), ref) < tol
    ref.backward(dl)
    grads = [torch.zeros_like(x, device=DEV) for x in (lnw, lnb, W, b)]
    dt = o.head_bwd(t, N, lnw.to(DEV), lnb.to(DEV), W.to(DEV), stats, dl.to(DEV), B, grads, False, dropout=p,
                    seed=seed)
    assert rel_err(dt.float().cpu(), tr.grad) < tol
    assert torch.count_nonzero(dt.view(B, N, D)[:, 1:]).item() == 0
    for got, want in zip(grads, P):
        assert rel_err(got.cpu(), want.grad) < tol
    # a dropped feature of sample b passes no gradient to its LN output: d(ln_b) restricted to one
    # sample (B = 1 launch) is zero exactly where that sample's feature was dropped
    g1 = [torch.zeros_like(x, device=DEV) for x in (lnw, lnb, W, b)]
    _, st1 = o.head_fwd(t[:N], N, lnw.to(DEV), lnb.to(DEV), 1e-5, W.to(DEV), b.to(DEV), 1, dropout=p, seed=seed)
    o.head_bwd(t[:N], N, lnw.to(DEV), lnb.to(DEV), W.to(DEV), st1, dl[:1].to(DEV), 1, g1, False, dropout=p, seed=seed)
    assert torch.equal(g1[1].cpu() != 0, keep[0])


# ---------------------------------------------------------------------- misc
def test_colsum_and_tokens_and_head():
    o = ops()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3001, 768, generator=g)
    out = torch.zeros(768, device=DEV)
    o.colsum(bf(x), out)
    assert rel_err(out.cpu(), bf(x).float().cpu().sum(0)) < 1e-4
    B, n, D = 4, 9, 384
    emb = torch.randn(B * n, D, generator=g)
    cls, pos = torch.randn(1, 1, D, generator=g), torch.randn(1, n + 1, D, generator=g)
    t = o.tokens_fwd(emb.to(DEV), cls.to(DEV), pos.to(DEV), B, n, D)
    ref = torch.cat([cls.expand(B, -1, -1), emb.view(B, n, D)], 1) + pos
    assert torch.allclose(t.cpu().view(B, n + 1, D), ref, atol=1e-6)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("D,B", [(384, 5), (6, 5), (388, 5), (768, 41)])
def test_tokens_bwd_dropout(dtype, D, B):
    """Gradient of the token assembly (cat(cls, patches) + pos, dropout): d(patches), d(cls) and
    d(pos) against the host keep mask; bf16 with D % 8 == 0 takes the 8-column kernel (B = 41: 16 batch
    chunks of 3, the last ones short or empty), other D % 4 == 0 the 4-column one, D = 6 the per-element
    one (csrc/vit_edge.hip tokens_bwd8_kernel / tokens_bwd4_kernel / tokens_bwd_kernel)."""
    o = ops()
    n, p, seed = 9, 0.1, 777
    N = n + 1
    g = torch.Generator().manual_seed(21)
    cast = bf if dtype == "bf16" else (lambda t: t.to(DEV))
    dt = cast(torch.randn(B * N, D, generator=g))
    dcls, dpos = torch.zeros(D, device=DEV), torch.zeros(N * D, device=DEV)
    demb = o.tokens_bwd(dt, B, n, D, dcls, dpos, False, dropout=p, seed=seed)
    keep = keep_mask(seed, (B, N * D), p).view(B, N, D)
    gref = torch.where(keep, dt.float().cpu().view(B, N, D) / (1 - p), torch.zeros(()))
    tol = 1e-2 if dtype == "bf16" else 1e-5
    assert rel_err(demb.float().cpu().view(B, n, D), gref[:, 1:]) < tol
    assert rel_err(dpos.cpu().view(N, D), gref.sum(0)) < tol
    assert rel_err(dcls.cpu(), gref[:, 0].sum(0)) < tol


def test_cross_entropy_matches_torch():
    o = ops()
    g = torch.Generator().manual_seed(9)
    logits = torch.randn(256, 7, generator=g)
    y = torch.randint(0, 7, (256,), generator=g)
    w = torch.rand(7, generator=g) + 0.5
    for ls in (0.0, 0.1):
        for wt in (None, w):
            lg = logits.clone().requires_grad_(True)
            ref = torch.nn.functional.cross_entropy(lg, y, weight=wt, label_smoothing=ls)
            ref.backward()
            loss, dl = o.cross_entropy(logits.to(DEV), y.to(DEV), None if wt is None else wt.to(DEV), ls)
            assert abs(loss.item() - ref.item()) < 1e-5
            assert (dl.cpu() - lg.grad).abs().max().item() < 1e-6


@pytest.mark.gpu
def test_transposed_bf16_shadow():
    """FlatParams.half_t_view == W^T of the bf16 shadow for ragged 2-D shapes, and it follows
    in-place parameter updates (cast path) and the fused optimizer's refresh."""
    from fervit.runtime import FlatParams

    g = torch.Generator().manual_seed(5)
    shapes = [(70, 130), (3072, 768), (1, 5), (7,), (65, 64), (2, 3, 4), (129, 1)]
    ps = [torch.nn.Parameter(torch.randn(*s, generator=g).cuda()) for s in shapes]
    flat = FlatParams(ps)
    for p in ps:
        if p.dim() == 2:
            assert torch.equal(flat.half_t_view(p), flat.half_view(p).t().contiguous())
    with torch.no_grad():
        ps[1].mul_(-2.0)
    t = flat.half_t_view(ps[1])
    assert torch.equal(t, ps[1].data.to(torch.bfloat16).t().contiguous())
    with pytest.raises(ValueError):
        flat.half_t_view(ps[3])


def test_persistent_work_queue_streams_and_capture():
    """The persistent GEMM / attention kernels claim tiles from per-stream device counters whose
    launch-start values the host tracks (common.h wq_*): many back-to-back launches on one stream,
    launches alternating with a second stream that runs concurrently, and a graph-captured launch
    (fixed stride under capture) replayed between eager ones must all give the first launch's bits."""
    o = ops()
    g = torch.Generator(device=DEV).manual_seed(3)
    M, N, K = 256 * 70, 1024, 192  # 280 tiles of 256x256: 8-phase persistent kernel
    x = torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, device=DEV, generator=g) / math.sqrt(K)).to(torch.bfloat16)
    ref = o.linear_fwd(x, w)
    assert rel_err(ref, x.float() @ w.float().t()) < 1e-2
    B, Nt, H, dh = 48, 197, 12, 64  # 576 (batch, head) units
    qkv = torch.randn(B * Nt, 3 * H * dh, device=DEV, generator=g).to(torch.bfloat16)
    dout = torch.randn(B * Nt, H * dh, device=DEV, generator=g).to(torch.bfloat16)
    sv = o.attention_saved(qkv, B, Nt, H, dh, dropout=0.1)
    ao = torch.empty(B * Nt, H * dh, device=DEV, dtype=torch.bfloat16)
    dq = torch.empty_like(qkv)
    o.attention_fwd(qkv, ao, sv, B, Nt, H, dh, dropout=0.1, seed=4)
    o.attention_bwd(qkv, ao, dout, sv, dq, B, Nt, H, dh, dropout=0.1, seed=4)
    ao_ref, dq_ref = ao.clone(), dq.clone()
    side = torch.cuda.Stream()
    outs = []
    for i in range(40):
        st = side if i % 3 == 1 else torch.cuda.current_stream()
        with torch.cuda.stream(st):
            outs.append(o.linear_fwd(x, w))
    torch.cuda.synchronize()
    for y in outs:
        assert torch.equal(y, ref)
    for _ in range(6):
        o.attention_fwd(qkv, ao, sv, B, Nt, H, dh, dropout=0.1, seed=4)
        o.attention_bwd(qkv, ao, dout, sv, dq, B, Nt, H, dh, dropout=0.1, seed=4)
        assert torch.equal(ao, ao_ref) and torch.equal(dq, dq_ref)
    # captured launch (fixed stride) between eager launches on the capture stream's queue
    cap_out = torch.empty_like(ref)
    gr = torch.cuda.CUDAGraph()
    s2 = torch.cuda.Stream()
    s2.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s2):
        o.linear_fwd(x, w, out=cap_out)
        with torch.cuda.graph(gr, stream=s2):
            o.linear_fwd(x, w, out=cap_out)
    torch.cuda.current_stream().wait_stream(s2)
    for _ in range(3):
        cap_out.zero_()
        gr.replay()
        assert torch.equal(o.linear_fwd(x, w), ref)
        torch.cuda.synchronize()
        assert torch.equal(cap_out, ref)


@pytest.mark.parametrize("N,H,dh,B", [(197, 12, 64, 64), (19, 8, 64, 256), (37, 12, 64, 48), (10, 6, 64, 64),
                                      (100, 4, 32, 16)])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_attention_fwd_occupancy_form_bit_exact(N, H, dh, B, p):
    """The occupancy form of the forward (fer_attention_set_fwd_kernel(2): one workgroup per (batch,
    head), two per CU) runs the persistent kernel's arithmetic in the same order: output, lse and the
    stored keep bits must agree bit for bit with it (fer_attention_set_fwd_kernel(1)), and the backward
    fed from either gives identical gradients."""
    from fervit._lib import lib

    o = ops()
    D = H * dh
    g = torch.Generator(device=DEV).manual_seed(B * N + H + int(p * 10))
    qkv = torch.randn(B * N, 3 * D, device=DEV, generator=g).to(torch.bfloat16)
    dout = torch.randn(B * N, D, device=DEV, generator=g).to(torch.bfloat16)
    res = []
    try:
        for k in (1, 2):
            assert lib().fer_attention_set_fwd_kernel(k) == 0
            out = torch.full((B * N, D), float("nan"), device=DEV, dtype=torch.bfloat16)
            saved = o.attention_saved(qkv, B, N, H, dh, dropout=p)
            saved.fill_(float("nan"))
            o.attention_fwd(qkv, out, saved, B, N, H, dh, dropout=p, seed=99 + N)
            dqkv = torch.empty_like(qkv)
            o.attention_bwd(qkv, out, dout, saved, dqkv, B, N, H, dh, dropout=p, seed=99 + N)
            torch.cuda.synchronize()
            res.append((out, saved[:B * H * N].clone(), saved[B * H * N:].clone(), dqkv))
    finally:
        lib().fer_attention_set_fwd_kernel(0)
    (o1, l1, m1, d1), (o2, l2, m2, d2) = res
    assert torch.isfinite(o1.float()).all()
    assert torch.equal(o1.view(torch.int16), o2.view(torch.int16))
    assert torch.equal(l1.view(torch.int32), l2.view(torch.int32))
    if p > 0:  # keep-bit words (the padding words after lse are never written by either kernel)
        nb = (N + 31) // 32
        off = (B * H * N + 63) // 64 * 64 - B * H * N
        w1 = m1[off:off + B * H * nb * nb * 32].view(torch.int32).view(B * H, nb, nb, 32)
        w2 = m2[off:off + B * H * nb * nb * 32].view(torch.int32).view(B * H, nb, nb, 32)
        # words of padding keys (kb*32 + j >= N) are unspecified: the occupancy form skips their hashing
        # when the last key block holds <= 8 keys; the backward reads them but its results cannot depend
        # on them (the dqkv comparison below)
        real = (torch.arange(nb, device=DEV)[:, None] * 32 + torch.arange(32, device=DEV)[None, :]) < N
        real = real[None, :, None, :].expand_as(w1)
        assert torch.equal(w1[real], w2[real])
    assert torch.equal(d1.view(torch.int16), d2.view(torch.int16))


def test_gemm_work_queue_every_tile_written():
    """Work-queue claims of the pipelined plain-kind GEMM (the next tile's claim is an inline-asm atomic
    whose result is read after the main loop): a NaN-prefilled output must come back finite and equal
    to torch's product over the whole matrix in every one of several back-to-back launches on one
    stream (counter bases carried across launches), i.e. no tile skipped or left half-written. The
    plain kind's arithmetic is idempotent per tile, so a tile processed twice shows up only as the
    claim count going off, which the next launches would then see as skipped tiles."""
    from fervit._lib import lib

    o = ops()
    assert lib().fer_set_persistent_mode(0) == 0
    g = torch.Generator(device=DEV).manual_seed(17)
    M, N, K = 50432, 2304, 768
    x = torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, device=DEV, generator=g) / math.sqrt(K)).to(torch.bfloat16)
    b = torch.randn(N, device=DEV, generator=g)
    ref = x.float() @ w.float().t() + b
    for _ in range(4):
        y = torch.full((M, N), float("nan"), device=DEV, dtype=torch.bfloat16)
        o.linear_fwd(x, w, b, out=y)
        torch.cuda.synchronize()
        assert torch.isfinite(y.float()).all()
        assert rel_err(y, ref) < 1e-2


@pytest.mark.parametrize("D", [768, 388])
def test_tokens_fwd_bf16_dropout(D):
    """Token assembly t = dropout(cat(cls, patches) + pos) on the bf16 path: D % 8 == 0 takes the 8-column
    kernel (csrc/vit_edge.hip tokens_fwd8_kernel), D = 388 the 4-column one; values and keep bits against the
    host keep mask (the same element index row * D + d in both kernels)."""
    o = ops()
    B, n, p, seed = 6, 13, 0.1, 4242
    N = n + 1
    g = torch.Generator().manual_seed(D)
    emb = torch.randn(B * n, D, generator=g)
    cls, pos = torch.randn(1, 1, D, generator=g), torch.randn(1, N, D, generator=g)
    t = o.tokens_fwd(bf(emb), cls.to(DEV), pos.to(DEV), B, n, D, dropout=p, seed=seed)
    ref = torch.cat([cls.expand(B, -1, -1), bf(emb).float().cpu().view(B, n, D)], 1) + pos
    keep = keep_mask(seed, (B * N, D), p).view(B, N, D)
    want = torch.where(keep, ref / (1 - p), torch.zeros(()))
    got = t.float().cpu().view(B, N, D)
    assert torch.equal(got != 0, keep)
    assert rel_err(got, want) < 1e-2
