"""Element-wise checks of the row kernels (csrc/layernorm.hip) and the small element / reduction
kernels (csrc/optim.hip, csrc/reduce.hip, csrc/vit_edge.hip) against plain float64 formulas on the CPU, on every dispatch branch.

Every comparison is per element: |got - ref| <= out_round * |ref| + c * 2^-23 * scale_i.
  * ref is float64 torch on the CPU, computed from the exact values the kernel was handed (bf16
    inputs are cast to bf16 first and then widened; the backward uses the fp32 mean / rstd it was
    given; eps and the dropout scale are the fp32 values of the ABI).
  * out_round is 2^-8 for a bf16 output (one RNE rounding is <= 2^-9 relative, doubled for a value
    that sits on a rounding boundary after the fp32 error) and 0 for an fp32 output.
  * scale_i is the magnitude fp32 arithmetic handled for this element (see the *_ref functions).
  * c is measured inside each test against the same reference, never against the kernel: the same
    op in float32 torch on the CPU (native_layer_norm, autograd, sum), its worst element error in
    scale_i units, times 4 (the kernels sum in butterfly order, torch sequentially / pairwise),
    floor 16. Every measurement is printed as `c-measure <op> <dtype> <value>` (DESIGN.md section 2
    has the table).
A failure names the worst element: index, got, ref, bound."""
import functools
import math

import numpy as np
import pytest
import torch

from abi_harness import f32v, last_error, nanview, ops, ptr, tdt, untouched
from abi_harness import lib as L
from dropmask import keep_mask
from elemwise import BF_ROUND, U, assert_bits_equal, assert_close, measure_c  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda"
BIG = 8192 * 256 + 3  # past the 8192-block grid cap of the element kernels: grid-stride loop


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---------------------------------------------------------------------- LayerNorm references
def ln_fwd_ref(x, G, Bt, eps):
    """float64 forward. x [M][D]; G, Bt the gamma / beta row of every row, [M][D] or [D]."""
    mu = x.mean(1, keepdim=True)
    var = ((x - mu) ** 2).mean(1, keepdim=True)
    rstd = (var + eps) ** -0.5
    y = (x - mu) * rstd * G + Bt
    return dict(y=y, mean=mu[:, 0], rstd=rstd[:, 0],
                s_y=(x.abs() + mu.abs()) * rstd * G.abs() + Bt.abs(), s_mean=x.abs().mean(1), s_rstd=rstd[:, 0])


def ln_bwd_ref(x, dy, G, res, mean, rstd, keep, dscale):
    """float64 backward from the formula, with the mean / rstd given. keep: host mask or None."""
    mu, rs = mean[:, None], rstd[:, None]
    xh = (x - mu) * rs
    gy = G * dy
    s1 = gy.mean(1, keepdim=True)
    s2 = (gy * xh).mean(1, keepdim=True)
    dx = rs * (gy - s1 - xh * s2)
    s_dx = rs * (gy.abs() + gy.abs().mean(1, keepdim=True) + xh.abs() * (gy * xh).abs().mean(1, keepdim=True))
    if res is not None:
        dx = dx + res
        s_dx = s_dx + res.abs()
    r = dict(dx=dx, s_dx=s_dx, dgamma=(dy * xh).sum(0), s_dgamma=(dy * xh).abs().sum(0), dbeta=dy.sum(0),
             s_dbeta=dy.abs().sum(0))
    if keep is not None:
        r["dxd"] = torch.where(keep, dx * dscale, torch.zeros((), dtype=torch.float64))
        r["s_dxd"] = s_dx * dscale
        last = r["dxd"]
    else:
        last = dx
    r["dbias"], r["s_dbias"] = last.sum(0), last.abs().sum(0)
    return r


def ln_f32(x, gam, bet, gi, eps, dy, res, keep, dscale):
    """The same op in float32 torch on the CPU: native_layer_norm and its autograd."""
    D = x.shape[1]
    x32 = x.float().requires_grad_(True)
    w32, b32 = gam.detach().clone().float().requires_grad_(True), bet.detach().clone().float().requires_grad_(True)
    xh, mean, rstd = torch.native_layer_norm(x32, (D,), None, None, eps)
    y = xh * w32[gi] + b32[gi]
    y.backward(dy.float())
    dx = x32.grad if res is None else x32.grad + res.float()
    r = dict(y=y.detach(), mean=mean.detach().reshape(-1), rstd=rstd.detach().reshape(-1), dx=dx,
             dgamma=w32.grad.sum(0), dbeta=b32.grad.sum(0))
    last = dx
    if keep is not None:
        r["dxd"] = last = torch.where(keep, dx * torch.tensor(dscale, dtype=torch.float32), torch.zeros(()))
    r["dbias"] = last.sum(0)
    return r


def gamma_index(M, Lr, row_div):
    return (torch.arange(M) // row_div) % Lr


@functools.lru_cache(maxsize=4)
def ln_inputs(M, D, Lr, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, D, generator=g) * 2 + 0.5
    gam, bet = 1 + 0.1 * torch.randn(Lr, D, generator=g), 0.1 * torch.randn(Lr, D, generator=g)
    dy, res = torch.randn(M, D, generator=g), torch.randn(M, D, generator=g)
    return x, gam, bet, dy, res


def call_ln_fwd(x, gam, bet, Lr, row_div, y, mean, rstd, M, D, eps):
    o = ops()
    return L().fer_layernorm_fwd(o.dcode(x), x.data_ptr(), x.stride(0), gam.data_ptr(), bet.data_ptr(), Lr, row_div,
                                 y.data_ptr(), y.stride(0), ptr(mean), ptr(rstd), M, D, eps, o.stream())


def call_ln_bwd(dy, x, mean, rstd, gam, Lr, row_div, res, dx, dxd, thr, sc, seed, dgamma, dbeta, dbias, accumulate,
                M, D):
    o = ops()
    ws = torch.empty(max(1, L().fer_layernorm_bwd_ws(M, D) // 4), dtype=torch.float32, device=DEV)
    return L().fer_layernorm_bwd(o.dcode(x), dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), mean.data_ptr(),
                                 rstd.data_ptr(), gam.data_ptr(), Lr, row_div, ptr(res),
                                 res.stride(0) if res is not None else D, dx.data_ptr(), dx.stride(0), ptr(dxd), thr,
                                 sc, seed, ptr(dgamma), ptr(dbeta), ptr(dbias), int(accumulate), ws.data_ptr(),
                                 ws.numel() * 4, M, D, o.stream())


GRADS = ("dgamma", "dbeta", "dbias")


def run_ln(dtype, M, D, *, Lr=1, row_div=1, eps=1e-5, pads=None, use_res=True, p=0.1, use_dxd=True, want=GRADS,
           accumulate=False, want_stats=True, inputs=None, seed=777, keep_check=True, tag="ln"):
    """Forward and backward through the C ABI on padded views, every output checked per element.
    Returns the device outputs for further assertions."""
    o = ops()
    dt = tdt(dtype)
    out_round = BF_ROUND if dtype == "bf16" else 0.0
    pads = dict(dict(x=0, y=0, dy=0, res=0, dx=0), **(pads or {}))
    x0, gam, bet, dy0, res0 = inputs if inputs is not None else ln_inputs(M, D, Lr, 1000 * D + M)
    eps = f32v(eps)
    xd, _ = nanview(M, D, pads["x"], dt, x0, guard=0)
    dyd, _ = nanview(M, D, pads["dy"], dt, dy0, guard=0)
    resd = nanview(M, D, pads["res"], dt, res0, guard=0)[0] if use_res else None
    gd, bd = gam.to(DEV).contiguous(), bet.to(DEV).contiguous()
    # the exact values the kernels see
    x, dy = xd.float().cpu().double(), dyd.float().cpu().double()
    res = resd.float().cpu().double() if use_res else None
    gi = gamma_index(M, Lr, row_div)
    G, Bt = gam.double()[gi], bet.double()[gi]

    # ---- forward
    yd, yp = nanview(M, D, pads["y"], dt, guard=0)
    mean = torch.full((M,), float("nan"), device=DEV)
    rstd = torch.full((M,), float("nan"), device=DEV)
    rc = call_ln_fwd(xd, gd, bd, Lr, row_div, yd, mean if want_stats else None, rstd if want_stats else None, M, D,
                     eps)
    assert rc == 0, last_error()
    fr = ln_fwd_ref(x, G, Bt, eps)
    thr, sc = o.drop_args(p)
    sc = f32v(sc)
    keep = keep_mask(seed, (M, D), p) if (use_dxd and p > 0) else (torch.ones(M, D, dtype=torch.bool) if use_dxd else None)
    t32 = ln_f32(x, gam, bet, gi, eps, dy, res, keep, sc)
    c_y = measure_c(f"{tag}.y", dtype, [(t32["y"], fr["y"], fr["s_y"])])
    c_mean = measure_c(f"{tag}.mean", dtype, [(t32["mean"], fr["mean"], fr["s_mean"])])
    c_rstd = measure_c(f"{tag}.rstd", dtype, [(t32["rstd"], fr["rstd"], fr["s_rstd"])])
    assert_close(f"{tag}.y", yd, fr["y"], fr["s_y"], c_y, out_round)
    untouched(f"{tag}.y", yp, M, D, guard=0)
    if want_stats:
        assert_close(f"{tag}.mean", mean, fr["mean"], fr["s_mean"], c_mean, 0.0)
        assert_close(f"{tag}.rstd", rstd, fr["rstd"], fr["s_rstd"], c_rstd, 0.0)
    else:
        # the statistics the backward needs, from a second forward that does save them
        assert torch.isnan(mean).all().item() and torch.isnan(rstd).all().item()
        y2 = torch.empty(M, D, dtype=dt, device=DEV)
        assert call_ln_fwd(xd, gd, bd, Lr, row_div, y2, mean, rstd, M, D, eps) == 0, last_error()
        assert_bits_equal(f"{tag}.y with / without saved statistics", y2, yd.contiguous())

    # ---- backward
    dxv, dxp = nanview(M, D, pads["dx"], dt, guard=0)
    dxdv, dxdp = nanview(M, D, pads["dx"], dt, guard=0) if use_dxd else (None, None)
    g0 = torch.Generator().manual_seed(5)
    init = {k: (torch.randn(D, generator=g0) * 3 if accumulate else torch.full((D,), float("nan"))) for k in GRADS}
    gout = {k: (init[k].clone().to(DEV) if k in want else None) for k in GRADS}
    rc = call_ln_bwd(dyd, xd, mean, rstd, gd, Lr, row_div, resd, dxv, dxdv, thr, sc, seed, gout["dgamma"],
                     gout["dbeta"], gout["dbias"], accumulate, M, D)
    assert rc == 0, last_error()
    m_in, r_in = mean.cpu().double(), rstd.cpu().double()
    br = ln_bwd_ref(x, dy, G, res, m_in, r_in, keep, sc)
    # c: fp32 torch against the float64 formula on the statistics torch itself saw (the exact ones)
    bx = ln_bwd_ref(x, dy, G, res, fr["mean"], fr["rstd"], keep, sc)
    c_dx = measure_c(f"{tag}.dx", dtype, [(t32["dx"], bx["dx"], bx["s_dx"])])
    assert_close(f"{tag}.dx", dxv, br["dx"], br["s_dx"], c_dx, out_round)
    untouched(f"{tag}.dx", dxp, M, D, guard=0)
    if use_dxd:
        c_dxd = measure_c(f"{tag}.dx_drop", dtype, [(t32["dxd"], bx["dxd"], bx["s_dxd"])])
        assert_close(f"{tag}.dx_drop", dxdv, br["dxd"], br["s_dxd"], c_dxd, out_round)
        untouched(f"{tag}.dx_drop", dxdp, M, D, guard=0)
        if p == 0:
            assert_bits_equal(f"{tag}.dx_drop at p = 0 vs dx", dxdv.contiguous(), dxv.contiguous())
        elif keep_check:
            # keep decisions: zero exactly where the host mask drops, on the elements that are not
            # themselves (nearly) zero
            live = br["dx"].abs() > 2.0 ** -20 * br["dx"].abs().max()
            assert live.double().mean().item() >= 0.999, f"{tag}: live set {live.double().mean().item():.5f}"
            nz = dxdv.float().cpu() != 0
            wrong = (nz != keep) & live
            assert not wrong.any().item(), \
                f"{tag}: {int(wrong.sum())} keep decisions differ from the host mask, first at {wrong.nonzero()[0].tolist()}"
    if Lr == 1:
        for k in GRADS:
            if k not in want:
                continue
            c_k = measure_c(f"{tag}.{k}", dtype, [(t32[k], bx[k], bx["s_" + k])])
            ref, scale = br[k], br["s_" + k]
            if accumulate:
                ref, scale = ref + init[k].double(), scale + init[k].double().abs()
            assert_close(f"{tag}.{k}", gout[k], ref, scale, c_k, 0.0)
    return dict(y=yd, mean=mean, rstd=rstd, dx=dxv, dxd=dxdv, grads=gout, fwd_ref=fr, bwd_ref=br)


# ---------------------------------------------------------------------- LayerNorm cases
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("D", [4, 8, 12, 252, 256, 260, 264, 388, 1020, 1024])
def test_layernorm_dispatch(dtype, D):
    """Every (D + 255) / 256 instantiation at M = 37 (three 8-wide blocks, ten 4-wide ones). bf16 with
    D % 8 == 0 (8, 256, 264, 1024): ln_fwd8_kernel<1..4> and ln_bwd8_kernel<1..4, true>; bf16 with
    D % 8 == 4 (4, 12, 252, 260, 388, 1020): ln_fwd_kernel<bf16> and ln_bwd_kernel<bf16, 1..4>; fp32:
    ln_fwd_kernel<float>, ln_bwd_kernel<float, 1..4>. 260 and 264 leave the last chunk nearly empty."""
    run_ln(dtype, 37, D, tag="ln.dispatch")


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("D,msg", [(1028, "multiple of 4 and <= 1024"), (6, "multiple of 4 and <= 1024")])
def test_layernorm_bad_width_is_an_error(dtype, D, msg):
    """Host checks of fer_layernorm_fwd / fer_layernorm_bwd: D > 1024 or D % 4 != 0 returns non-zero with a
    fer_last_error text and launches nothing (the NaN-filled outputs stay NaN)."""
    M, dt = 8, tdt(dtype)
    x = torch.ones(M, D, dtype=dt, device=DEV)
    w = torch.ones(D, device=DEV)
    y = torch.full((M, D), float("nan"), dtype=dt, device=DEV)
    st = torch.full((M,), float("nan"), device=DEV)
    rc = call_ln_fwd(x, w, w, 1, 1, y, st, st, M, D, 1e-5)
    assert rc != 0 and msg in last_error() and "layernorm_fwd" in last_error()
    one = torch.ones(M, device=DEV)
    rc = call_ln_bwd(x, x, one, one, w, 1, 1, None, y, None, 0, 1.0, 0, None, None, None, False, M, D)
    assert rc != 0 and msg in last_error() and "layernorm_bwd" in last_error()
    torch.cuda.synchronize()
    assert torch.isnan(y).all().item() and torch.isnan(st).all().item()


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("pad", [8, 4])
@pytest.mark.parametrize("D", [768, 136])
@pytest.mark.parametrize("which", ["x", "y", "dy", "res", "dx", "all"])
def test_layernorm_row_strides(dtype, pad, D, which):
    """Row stride D + pad on x / y / dy / res / dx (dx_drop shares dx's stride) one at a time and all together,
    as column-0 views of NaN-filled wider tensors: a read of the padding poisons the row sums, a write to it
    clears a NaN. bf16, pad 8: ln_fwd8_kernel / ln_bwd8_kernel<C, true> with ld != D; bf16, pad 4: a single
    stride that is no multiple of 8 sends the call to ln_fwd_kernel<bf16> (x, y) / ln_bwd_kernel<bf16, VPL>
    (x, dy, res, dx); fp32: the 4-wide kernels either way."""
    names = ("x", "y", "dy", "res", "dx")
    pads = {k: (pad if which in (k, "all") else 0) for k in names}
    run_ln(dtype, 37, D, pads=pads, tag="ln.stride")


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("D", [512, 388])
@pytest.mark.parametrize("Lr", [2, 18])
@pytest.mark.parametrize("row_div", [1, 3])
def test_layernorm_row_groups(dtype, D, Lr, row_div):
    """gamma_rows = L > 1 (LayerWiseNorm): row r uses gamma / beta row (r / row_div) % L; M = 5 L row_div + 1, so
    the index wraps five times and the last group has one row. bf16 D = 512: ln_fwd8_kernel and
    ln_bwd8_kernel<2, false> (gamma loaded per row); bf16 D = 388 and fp32: the `gr` arithmetic of
    ln_fwd_kernel / ln_bwd_kernel. Parameter gradients need a shared gamma: asking for dgamma is the
    documented error."""
    M = Lr * row_div * 5 + 1
    r = run_ln(dtype, M, D, Lr=Lr, row_div=row_div, want=(), tag="ln.groups")
    dg = torch.full((Lr, D), float("nan"), device=DEV)
    x = torch.ones(M, D, dtype=tdt(dtype), device=DEV)
    w = torch.ones(Lr, D, device=DEV)
    dx = torch.full((M, D), float("nan"), dtype=tdt(dtype), device=DEV)
    rc = call_ln_bwd(x, x, r["mean"], r["rstd"], w, Lr, row_div, None, dx, None, 0, 1.0, 0, dg, None, None, False, M, D)
    assert rc != 0 and "parameter grads need shared gamma" in last_error()
    torch.cuda.synchronize()
    assert torch.isnan(dg).all().item() and torch.isnan(dx).all().item()


OPTIONS = {
    "no_res": dict(use_res=False),
    "dbias_of_dx": dict(use_dxd=False),
    "only_dgamma": dict(want=("dgamma",)),
    "only_dbeta": dict(want=("dbeta",)),
    "only_dbias": dict(want=("dbias",)),
    "no_param_grads": dict(want=()),
    "accumulate": dict(accumulate=True),
    "no_saved_stats": dict(want_stats=False),
    "p0_dx_drop": dict(p=0.0),
}


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("opt", sorted(OPTIONS))
def test_layernorm_options(dtype, opt):
    """Option combinations of fer_layernorm_bwd / _fwd at M = 1000, D = 768 (bf16: ln_fwd8_kernel<3>,
    ln_bwd8_kernel<3, true>; fp32: ln_fwd_kernel<float>, ln_bwd_kernel<float, 3>): res null; dbias without
    dx_drop (column sums of dx); one of dgamma / dbeta / dbias alone (part_reduce with null outputs) or none
    (want_part == 0, no partials written); accumulate onto non-zero gradients (init + sum); forward with
    mean / rstd null; dx_drop at dropout 0 (bit-identical to dx)."""
    run_ln(dtype, 1000, 768, inputs=ln_inputs(1000, 768, 1, 31), tag=f"ln.opt.{opt}", **OPTIONS[opt])


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("D", [768, 388])
@pytest.mark.parametrize("M", [1, 7, 9, 17])
def test_layernorm_few_rows(dtype, D, M):
    """M below one block or just past it (8 rows per 8-wide block, 4 per 4-wide one; the backward grid is
    ceil(M / 16)): half-waves / waves without a row still write zero column partials for dgamma / dbeta /
    dbias, and the prefetch of the 'next' row must not be read. bf16 D = 768: the 8-wide kernels; D = 388
    and fp32: the 4-wide ones."""
    run_ln(dtype, M, D, tag="ln.fewrows")


def _capped_rows(kind):
    return 64 * cu_count() + 37 if kind == "fwd_cap" else 32 * cu_count() + 5


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("D", [128, 768])
@pytest.mark.parametrize("kind", ["fwd_cap", "bwd_cap"])
def test_layernorm_capped_grid(dtype, D, kind):
    """Beyond the grid caps (forward 4 x CUs blocks, backward 2 x CUs): M = 64 CUs + 37 makes every half-wave of
    ln_fwd8_kernel walk 2 - 3 rows (the double-buffered loop takes its second trip, with an odd and an even
    tail) and of ln_bwd8_kernel 4 - 5 rows; M = 32 CUs + 5 gives 1 - 2 and 2 - 3. fp32: ln_bwd_kernel's paired
    two-register-set row loop at the same counts."""
    run_ln(dtype, _capped_rows(kind), D, tag="ln.capped")


def _stat_rows(kind, D, M=64):
    g = torch.Generator().manual_seed(41)
    if kind == "constant":
        v = torch.randn(M, 1, generator=g)
        v[0] = 0.0
        x = v.expand(M, D).clone()
    elif kind == "offset":
        x = 100 + 0.1 * torch.randn(M, D, generator=g)
    else:
        x = 1e-3 * torch.randn(M, D, generator=g)
    gam, bet = 1 + 0.1 * torch.randn(1, D, generator=g), 0.1 * torch.randn(1, D, generator=g)
    return x, gam, bet, torch.randn(M, D, generator=g), torch.randn(M, D, generator=g)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("eps", [1e-5, 1e-6])
def test_layernorm_constant_rows(dtype, eps):
    """Rows of one repeated value (row 0 all zero), D = 768, M = 64: variance 0, so the reference is y = beta,
    rstd = eps^-1/2 and dx from the formula with xhat = 0 (both passes of ln_fwd8_kernel / ln_fwd_kernel:
    a mean that is off by an ulp must not turn into a variance)."""
    inp = _stat_rows("constant", 768)
    r = run_ln(dtype, 64, 768, eps=eps, inputs=inp, tag="ln.constant")
    fr = r["fwd_ref"]
    assert torch.equal(fr["y"], inp[2].double().expand(64, 768))
    assert torch.allclose(fr["rstd"], torch.full((64,), f32v(eps) ** -0.5, dtype=torch.float64), rtol=1e-15)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("eps", [1e-5, 1e-6])
def test_layernorm_large_offset_rows(dtype, eps):
    """Rows with mean 100 and std 0.1, D = 768, M = 64. This is the case a one-pass variance
    E[x^2] - mean^2 fails: 1e4 * 2^-24 per term is the size of the variance itself, while the two-pass
    form of ln_fwd8_kernel / ln_fwd_kernel keeps rstd to a few ulp."""
    run_ln(dtype, 64, 768, eps=eps, inputs=_stat_rows("offset", 768), tag="ln.offset")


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("eps", [1e-5, 1e-6])
def test_layernorm_tiny_std_rows(dtype, eps):
    """Rows with std 1e-3 (variance 1e-6, the size of timm's eps = 1e-6 and a tenth of nn.LayerNorm's):
    eps decides rstd, in ln_fwd8_kernel / ln_fwd_kernel and through the saved rstd in the backward."""
    run_ln(dtype, 64, 768, eps=eps, inputs=_stat_rows("tiny", 768), tag="ln.tinystd")


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("M", [1000, "capped"])
def test_layernorm_bwd_deterministic(dtype, M):
    """One backward with dgamma, dbeta and dbias, twice: bit-identical dx, dx_drop and gradients (fixed-order
    column partials in ln_bwd8_kernel / ln_bwd_kernel and part_reduce), also with the capped grid where
    each block sums several rows."""
    o = ops()
    M = _capped_rows("fwd_cap") if M == "capped" else M
    D, dt = 768, tdt(dtype)
    x0, gam, bet, dy0, res0 = ln_inputs(M, D, 1, 1000 * D + M)
    xd, dyd, resd = x0.to(DEV, dt), dy0.to(DEV, dt), res0.to(DEV, dt)
    gd = gam.to(DEV)
    mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    o.layernorm_fwd(xd, gd, bet.to(DEV), 1e-5, mean=mean, rstd=rstd)
    runs = []
    for _ in range(2):
        outs = [torch.full((M, D), float("nan"), dtype=dt, device=DEV) for _ in range(2)]
        gr = [torch.full((D,), float("nan"), device=DEV) for _ in range(3)]
        o.layernorm_bwd(dyd, xd, mean, rstd, gd, dx=outs[0], res=resd, dx_drop=outs[1], dropout=0.1, seed=99,
                        dgamma=gr[0], dbeta=gr[1], dbias=gr[2])
        runs.append(outs + gr)
    for name, a, b in zip(("dx", "dx_drop") + GRADS, *runs):
        assert not torch.isnan(a.float()).any().item(), name
        assert_bits_equal(f"ln.determinism {name}", a, b)


# ---------------------------------------------------------------------- casts
def _special_f32():
    bits = [
        0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,  # exact ties: to even down / up, both signs
        0x3F808001, 0x3F807FFF, 0x3F818001, 0x3F817FFF,  # one fp32 ulp either side of a tie
        0x00000000, 0x80000000, 0x7F800000, 0xFF800000,  # +-0, +-inf
        0x7FC00000, 0xFFC00001, 0x7F800001,  # NaN (quiet, negative with payload, signalling)
        0x00000001, 0x007FFFFF, 0x00008000, 0x00018000, 0x80008000, 0x80018001, 0x00010000,  # fp32 denormals
        0x7F7FFFFF, 0x7F7F8000, 0xFF7FFFFF, 0x7F7F7FFF,  # round up to +-inf / stay the largest finite
        0x00800000, 0x007F8000,  # smallest normal; a denormal that rounds up to it
    ]
    return torch.from_numpy(np.array(bits, dtype=np.uint32).view(np.float32).copy())


def _with_specials(n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g) * torch.exp(4 * torch.randn(n, generator=g))
    sp = _special_f32()
    k = min(n, sp.numel())
    x[:k] = sp[:k]
    if n >= 2 * sp.numel():
        x[-sp.numel():] = sp
    return x


@pytest.mark.parametrize("n", [1, 255, 257, BIG])
def test_cast_f32_to_bf16_bit_exact(n):
    """fer_cast_f32_bf16 (cast_f32_bf16_kernel; the DDP wire format and the bf16 weight shadow) against
    tensor.to(bfloat16): round to nearest even on exact ties in both directions, +-0, +-inf, NaN, fp32
    denormals, values that round up to inf; n = 8192 * 256 + 3 takes the grid-stride loop's second trip."""
    x = _with_specials(n, 3)
    got = ops().cast_bf16(x.to(DEV)).cpu()
    ref = x.to(torch.bfloat16)
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan)
    assert_bits_equal("cast_bf16", torch.where(nan, torch.zeros_like(got), got), torch.where(nan, torch.zeros_like(ref), ref))


@pytest.mark.parametrize("n", [1, 255, 257, BIG])
def test_cast_bf16_to_f32_bit_exact(n):
    """fer_cast_bf16_f32 (cast_bf16_f32_kernel) against tensor.float(): an exact widening, including bf16
    denormals, +-0, +-inf and NaN; all sizes of the cast above."""
    xb = _with_specials(n, 4).to(torch.bfloat16)
    got = ops().cast_f32(xb.to(DEV)).cpu()
    ref = xb.float()
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan)
    assert_bits_equal("cast_f32", torch.where(nan, torch.zeros_like(got), got), torch.where(nan, torch.zeros_like(ref), ref))


# ---------------------------------------------------------------------- axpy
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("n", [1, 255, 257, BIG])
def test_axpy(dtype, n):
    """fer_axpy (axpy_kernel<T>): y = x + a t with a read from device memory, against float64. fp32: 1 ulp
    (the compiler may or may not fuse the multiply-add), taken at the larger of |y| and the product |a t|
    that an unfused form rounds; bf16: 2^-8 relative on top of that. n past the grid cap included."""
    g = torch.Generator().manual_seed(n % 1000)
    dt = tdt(dtype)
    x, t = torch.randn(n, generator=g).to(dt), torch.randn(n, generator=g).to(dt)
    a = torch.tensor([0.37], dtype=torch.float32)
    got = ops().axpy(x.to(DEV), t.to(DEV), a.to(DEV))
    at = a.double() * t.double()
    ref = x.double() + at
    assert_close(f"axpy {dtype}", got.float(), ref, torch.maximum(ref.abs(), at.abs()), 1.0,
                 BF_ROUND if dtype == "bf16" else 0.0)


# ---------------------------------------------------------------------- dot / sumsq
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("with_b", [True, False])
@pytest.mark.parametrize("n", [1, 1023, 1025, 1024 * 1024 + 7])
def test_dot(dtype, with_b, n):
    """fer_dot (dot_part_kernel<T> + sum_final_kernel): sum a_i b_i, or sum a_i^2 with b null, with and without
    accumulate onto a non-zero value, against float64 with the column-sum bound c 2^-23 sum |a_i b_i|;
    1023 / 1025 sit either side of one block's 1024 elements, 1024^2 + 7 uses all 1024 partials and the
    grid-stride loop. Two calls are bit-identical (fixed-order sums)."""
    g = torch.Generator().manual_seed(n % 997)
    dt = tdt(dtype)
    a = torch.randn(n, generator=g).to(dt)
    b = torch.randn(n, generator=g).to(dt) if with_b else None
    prod = a.double() * (b.double() if with_b else a.double())
    ref, scale = prod.sum(), prod.abs().sum()
    f32 = (a.float() * (b.float() if with_b else a.float())).sum()
    c = measure_c("dot" if with_b else "dot.sq", dtype, [(f32, ref, scale)])
    ad, bd = a.to(DEV), (b.to(DEV) if with_b else None)
    outs = []
    for _ in range(2):
        out = torch.full((1,), float("nan"), device=DEV)
        ops().dot(ad, bd, out)
        outs.append(out.cpu())
    assert_close(f"dot {dtype}", outs[0], ref.reshape(1), scale.reshape(1), c, 0.0)
    assert_bits_equal("dot twice", outs[0], outs[1])
    acc = torch.tensor([-3.25], device=DEV)
    ops().dot(ad, bd, acc, accumulate=True)
    assert_close(f"dot {dtype} accumulate", acc, (ref - 3.25).reshape(1), (scale + 3.25).reshape(1), c, 0.0)


@pytest.mark.parametrize("n", [1, 1023, 1025, 1024 * 1024 + 7])
def test_sumsq(n):
    """fer_sumsq (the gradient-norm reduction: dot_part_kernel<float> with b null, no accumulate: the output is
    overwritten) against float64 sum x_i^2, bit-identical across two calls."""
    o = ops()
    g = torch.Generator().manual_seed(n % 991)
    x = torch.randn(n, generator=g)
    ref, f32 = (x.double() ** 2).sum(), (x * x).sum()
    c = measure_c("sumsq", "fp32", [(f32, ref, ref)])
    xd = x.to(DEV)
    ws = torch.empty(1024, device=DEV)
    outs = []
    for _ in range(2):
        out = torch.full((1,), 123.0, device=DEV)
        assert L().fer_sumsq(xd.data_ptr(), n, out.data_ptr(), ws.data_ptr(), ws.numel() * 4, o.stream()) == 0, last_error()
        outs.append(out.cpu())
    assert_close("sumsq", outs[0], ref.reshape(1), ref.reshape(1), c, 0.0)
    assert_bits_equal("sumsq twice", outs[0], outs[1])


@pytest.mark.parametrize("sq_scale", [1.0, 0.25])
@pytest.mark.parametrize("sumsq", [0.0, 1e-12, 1.0, 1e8])
def test_clip_coef(sumsq, sq_scale):
    """fer_clip_coef (clip_coef_kernel): min(1, max_norm / (sqrt(sumsq * sq_scale) + 1e-6)) in float64, relative
    error 1e-6; sumsq = 0 and 1e-12 take the min(1, .) branch, 1e8 the clipping one."""
    o = ops()
    s = torch.tensor([sumsq], dtype=torch.float32, device=DEV)
    coef = torch.full((1,), float("nan"), device=DEV)
    max_norm = 1.0
    assert L().fer_clip_coef(s.data_ptr(), sq_scale, max_norm, coef.data_ptr(), o.stream()) == 0, last_error()
    ref = min(1.0, max_norm / (math.sqrt(float(s.item()) * sq_scale) + 1e-6))
    got = coef.item()
    assert abs(got - ref) <= 1e-6 * abs(ref), f"clip_coef({sumsq}, {sq_scale}): got {got!r} ref {ref!r}"


# ---------------------------------------------------------------------- dropout
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("n", [1, 255, 257, BIG])
def test_dropout(dtype, n):
    """fer_dropout (dropout_kernel<T>) on strictly positive input: zero exactly where the host keep mask
    (tests/dropmask.py, element index = linear index) drops, kept values x / (1 - p) to one fp32 rounding
    (bf16: plus the output rounding), including the grid-stride loop past the grid cap; p = 0 returns x bit
    for bit."""
    o = ops()
    g = torch.Generator().manual_seed(n % 983)
    x = (torch.rand(n, generator=g) + 0.5).to(tdt(dtype))
    p, seed = 0.1, 4242
    xd = x.to(DEV)
    got = o.dropout(xd, p, seed).cpu()
    keep = keep_mask(seed, (n,), p)
    wrong = (got != 0) != keep
    assert not wrong.any().item(), f"dropout: {int(wrong.sum())} keep decisions differ, first at {int(wrong.nonzero()[0])}"
    sc = f32v(1.0 / (1.0 - p))
    ref = torch.where(keep, x.double() * sc, torch.zeros((), dtype=torch.float64))
    assert_close(f"dropout {dtype}", got.float(), ref, ref.abs(), 1.0, BF_ROUND if dtype == "bf16" else 0.0)
    assert_bits_equal("dropout p = 0", o.dropout(xd, 0.0, seed).cpu(), x)


# ---------------------------------------------------------------------- colsum
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("N", [4, 252, 768])
@pytest.mark.parametrize("M", [1, 31, 33, 8193, 3001])
def test_colsum(dtype, M, N):
    """fer_colsum (colsum_part_kernel<T> + part_reduce_kernel<8>) with row stride N + 4 (NaN padding): plain, and
    with accumulate onto a non-zero `out` and a device `scale`; part_reduce multiplies the column sum by
    *scale before it is added, so the reference is out0 + scale * sum. M = 1, 31, 33: one row block and
    just past it (32 rows per block), phases without a row; 3001: 94 blocks of 32 rows, the last short
    (the `r < r1` tail); 8193: the 256-block cap, 33 rows per block, trailing blocks empty. N = 4: one
    live lane per block; 252, 768: one and three column blocks."""
    o = ops()
    g = torch.Generator().manual_seed(M * 1000 + N)
    xv, _ = nanview(M, N, 4, tdt(dtype), torch.randn(M, N, generator=g), guard=0)
    x = xv.float().cpu().double()
    ref, scale = x.sum(0), x.abs().sum(0)
    f32 = xv.float().cpu().sum(0)
    c = measure_c("colsum", dtype, [(f32, ref, scale)])
    out = torch.full((N,), float("nan"), device=DEV)
    o.colsum(xv, out)
    assert_close(f"colsum {dtype}", out, ref, scale, c, 0.0)
    init = torch.randn(N, generator=g) * 5
    s = torch.tensor([-0.75], dtype=torch.float32)
    out = init.to(DEV)
    o.colsum(xv, out, accumulate=True, scale=s.to(DEV))
    ref2, scale2 = init.double() + s.double() * ref, init.double().abs() + 0.75 * scale
    c2 = measure_c("colsum.acc_scale", dtype, [(init + s * f32, ref2, scale2)])
    assert_close(f"colsum {dtype} accumulate + scale", out, ref2, scale2, c2, 0.0)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("N", [4084, 8192])
@pytest.mark.parametrize("M", [33, 3001])
def test_colsum_wide(dtype, M, N):
    """fer_colsum above 4080 columns: part_reduce_kernel<16> (16 columns x 16 row phases per block; N = 4084:
    the first width that takes it, the last block with 4 live columns). test_colsum's two forms on randn
    inputs, and the same two on integer inputs ({-3..3} * 4, integer start values, scale -0.75), where every
    partial, total and scaled total is exact in fp32 in any order: got == the float64 result."""
    o = ops()
    g = torch.Generator().manual_seed(M * 1000 + N)
    xv, _ = nanview(M, N, 4, tdt(dtype), torch.randn(M, N, generator=g), guard=0)
    x = xv.float().cpu().double()
    ref, scale = x.sum(0), x.abs().sum(0)
    f32 = xv.float().cpu().sum(0)
    c = measure_c("colsum.wide", dtype, [(f32, ref, scale)])
    out = torch.full((N + 16,), float("nan"), device=DEV)
    o.colsum(xv, out[:N])
    assert_close(f"colsum {dtype}", out[:N], ref, scale, c, 0.0)
    assert torch.isnan(out[N:]).all().item(), "colsum wrote past its N columns"
    init = torch.randn(N, generator=g) * 5
    s = torch.tensor([-0.75], dtype=torch.float32)
    out = init.to(DEV)
    o.colsum(xv, out, accumulate=True, scale=s.to(DEV))
    ref2, scale2 = init.double() + s.double() * ref, init.double().abs() + 0.75 * scale
    c2 = measure_c("colsum.wide.acc_scale", dtype, [(init + s * f32, ref2, scale2)])
    assert_close(f"colsum {dtype} accumulate + scale", out, ref2, scale2, c2, 0.0)
    xi = torch.randint(-3, 4, (M, N), generator=g).float() * 4
    xiv, _ = nanview(M, N, 4, tdt(dtype), xi, guard=0)
    refi = xi.double().sum(0)
    out = torch.full((N + 16,), float("nan"), device=DEV)
    o.colsum(xiv, out[:N])
    assert torch.equal(out[:N].cpu().double(), refi), "integer inputs: the column sums are not exact"
    assert torch.isnan(out[N:]).all().item(), "colsum wrote past its N columns"
    initi = torch.randint(-5, 6, (N,), generator=g).float()
    out = initi.to(DEV)
    o.colsum(xiv, out, accumulate=True, scale=s.to(DEV))
    assert torch.equal(out.cpu().double(), initi.double() - 0.75 * refi), "integer inputs: accumulate + scale is not exact"


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_colsum_bad_width_is_an_error(dtype):
    """fer_colsum's host check: N = 6 (no multiple of 4) returns the library's error and writes nothing."""
    o = ops()
    x = torch.ones(16, 6, dtype=tdt(dtype), device=DEV)
    out = torch.full((6,), float("nan"), device=DEV)
    ws = torch.empty(4096, device=DEV)
    rc = L().fer_colsum(o.dcode(x), x.data_ptr(), 6, 16, 6, out.data_ptr(), 0, None, ws.data_ptr(), ws.numel() * 4,
                        o.stream())
    assert rc != 0 and "colsum: N and ld must be multiples of 4" in last_error()
    torch.cuda.synchronize()
    assert torch.isnan(out).all().item()


# ---------------------------------------------------------------------- cross entropy
@pytest.mark.parametrize("zscale", [1.0, 1e4])
@pytest.mark.parametrize("C", [2, 7, 100])
@pytest.mark.parametrize("B", [1, 255, 257, 600])
def test_cross_entropy(B, C, zscale):
    """fer_cross_entropy (ce_kernel, one block): B = 257 and 600 take the `b += 256` loop's second and third
    trips, B = 1 and 255 leave threads idle; logits at scale 1e4 overflow expf without the max
    subtraction; row 0 has all-equal logits; class weights on / off, label smoothing 0 / 0.1, grad_scale
    1/4; want_grad = False passes a null dlogits and still writes the loss. Reference: float64
    torch.nn.functional.cross_entropy and its gradient; bound c 2^-23 |loss| for the loss and c 2^-23 / B
    for a gradient entry, c measured from fp32 torch on the CPU."""
    o = ops()
    g = torch.Generator().manual_seed(B * 101 + C)
    logits = torch.randn(B, C, generator=g) * zscale
    logits[0] = logits[0, 0]
    y = torch.randint(0, C, (B,), generator=g)
    w = torch.rand(C, generator=g) + 0.5
    F = torch.nn.functional
    ld, yd, wd = logits.to(DEV), y.to(DEV), w.to(DEV)
    for ls in (0.0, 0.1):
        for wt in (None, w):
            name = f"cross_entropy B={B} C={C} scale={zscale:g} ls={ls} weight={'on' if wt is not None else 'off'}"
            res = {}
            for prec in (torch.float64, torch.float32):
                lg = logits.clone().to(prec).requires_grad_(True)
                loss = F.cross_entropy(lg, y, weight=None if wt is None else wt.to(prec), label_smoothing=ls)
                loss.backward()
                res[prec] = (loss.detach(), lg.grad * 0.25)
            rl, rg = res[torch.float64]
            s_loss, s_grad = rl.abs().reshape(1), torch.full((B, C), 1.0 / B, dtype=torch.float64)
            c_l = measure_c("cross_entropy.loss", "fp32", [(res[torch.float32][0].reshape(1), rl.reshape(1), s_loss)])
            c_g = measure_c("cross_entropy.grad", "fp32", [(res[torch.float32][1], rg, s_grad)])
            loss, dl = o.cross_entropy(ld, yd, None if wt is None else wd, ls, grad_scale=0.25)
            assert_close(name + " loss", loss.reshape(1), rl.reshape(1), s_loss, c_l, 0.0)
            assert_close(name + " dlogits", dl, rg, s_grad, c_g, 0.0)
            loss2, none = o.cross_entropy(ld, yd, None if wt is None else wd, ls, grad_scale=0.25, want_grad=False)
            assert none is None
            assert_bits_equal(name + " loss without dlogits", loss2.reshape(1).cpu(), loss.reshape(1).cpu())
