"""Element-wise checks of the LatentCNN kernels (csrc/convbn.hip) through the C ABI against
tests/cnn_ref.py in float64 on the CPU, computed from the exact values handed to the kernel.

Bound: |got - ref| <= out_round * |ref| + c * 2^-23 * scale_i, out_round 2^-8 for
a bf16 output and 0 for fp32; c is measured per case from the same formulas in float32 torch on the CPU
(x 4, floor 16, printed as `c-measure` lines), never from the kernel. Outputs are views into NaN-filled
parents with guard rows and, in the padded run, padded strides; everything outside the view must stay
bit-unchanged. Inputs are padded views as well in the padded run.

BatchNorm: M x C over {2, 18, 36, 37, 4608} x {8, 24, 384, 512}, inputs {randn, constant columns,
mean 100 / std 0.1}, epilogues {BN -> ReLU -> dropout (conv block and res-block conv1), BN -> + residual
-> ReLU (res-block conv2), plain}, p in {0, 0.3}, tight and padded: the full cross for every shape. The
references of one (dtype, M, C, input kind) are computed once and shared by its paddings (and, for the
forward, by its p values), so a case stays within seconds. Dropped elements must be exactly 0 (host
mask, tests/dropmask.py).
Elements whose pre-ReLU value lies within its own bound of 0 are left out (the gate may fall either
way), in the backward together with their column's sums; the reference must leave out <= 0.1 %."""
import functools

import pytest
import torch

import cnn_ref as R
from abi_harness import all_nan, exact, f32v, last_error, nanview, ops, ptr, tdt, untouched
from abi_harness import lib as L
from dropmask import keep_mask
from elemwise import BF_ROUND, U, assert_bits_equal, assert_close, measure_c

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 2
F64 = torch.float64


# ---------------------------------------------------------------------- conv1d im2col
COLS_SHAPES = [(2, 18, 8), (1, 1, 8), (3, 2, 24), (5, 18, 512)]


def call_cols(x, cols, B, Ls, C):
    o = ops()
    return L().fer_conv1d_cols(o.dcode(x), x.data_ptr(), x.stride(0), cols.data_ptr(), cols.stride(0), B, Ls, C,
                               o.stream())


def call_cols_bwd(dcols, res, dx, B, Ls, C):
    o = ops()
    return L().fer_conv1d_cols_bwd(o.dcode(dcols), dcols.data_ptr(), dcols.stride(0), ptr(res),
                                   C if res is None else res.stride(0), dx.data_ptr(), dx.stride(0), B, Ls, C,
                                   o.stream())


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("shape", COLS_SHAPES)
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_conv1d_cols_forward_is_a_bit_exact_gather(dtype, shape, pad):
    B, Ls, C = shape
    dt = tdt(dtype)
    g = torch.Generator().manual_seed(B * 100 + C)
    xd, _ = nanview(B * Ls, C, pad, dt, torch.randn(B * Ls, C, generator=g))
    cd, cp = nanview(B * Ls, 3 * C, pad, dt)
    assert call_cols(xd, cd, B, Ls, C) == 0, last_error()
    want = R.conv1d_cols(xd.cpu().contiguous(), B, Ls)
    assert_bits_equal("cols", cd.cpu().contiguous(), want)
    untouched("cols", cp, B * Ls, 3 * C)
    if B > 1:  # the second sample's first row must not see the first sample's last row
        c4 = cd.cpu().float().reshape(B, Ls, C, 3)
        assert (c4[1, 0, :, 0] == 0).all() and (c4[0, Ls - 1, :, 2] == 0).all()


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("use_res", [False, True])
@pytest.mark.parametrize("shape", COLS_SHAPES)
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_conv1d_cols_backward(dtype, shape, use_res, pad):
    B, Ls, C = shape
    dt = tdt(dtype)
    M = B * Ls
    g = torch.Generator().manual_seed(B * 100 + C + 7)
    dd, _ = nanview(M, 3 * C, pad, dt, torch.randn(M, 3 * C, generator=g))
    rd = nanview(M, C, pad, dt, torch.randn(M, C, generator=g))[0] if use_res else None
    xd, xp = nanview(M, C, pad, dt)
    assert call_cols_bwd(dd, rd, xd, B, Ls, C) == 0, last_error()
    d64, r64 = exact(dd), exact(rd) if use_res else None
    ref = R.conv1d_cols_bwd(d64, B, Ls, r64)
    scale = R.conv1d_cols_bwd(d64.abs(), B, Ls, None if r64 is None else r64.abs())
    f32 = R.conv1d_cols_bwd(d64.float(), B, Ls, None if r64 is None else r64.float())
    c = measure_c("conv1d_cols_bwd", dtype, [(f32, ref, scale)])
    assert_close("conv1d_cols_bwd", xd, ref, scale, c, BF_ROUND if dtype == "bf16" else 0.0)
    untouched("conv1d_cols_bwd", xp, M, C)
    if B > 1 and not use_res:  # sample 1's first row: no term from sample 0's last row
        only = d64.reshape(B, Ls, C, 3)
        want = only[1, 0, :, 1] + (only[1, 1, :, 0] if Ls > 1 else 0)
        assert_close("cols_bwd boundary", xd[Ls], want, scale[Ls], c, BF_ROUND if dtype == "bf16" else 0.0)


# ---------------------------------------------------------------------- BatchNorm
BN_M = [2, 18, 36, 37, 4608]
BN_C = [8, 24, 384, 512]
KINDS = ["randn", "const", "shift"]
EPIS = {"relu_drop": dict(relu=True, res=False), "res_relu": dict(relu=True, res=True),
        "plain": dict(relu=False, res=False)}


@functools.lru_cache(maxsize=2)
def bn_inputs(M, C, kind):
    g = torch.Generator().manual_seed(M * 1000 + C + KINDS.index(kind))
    x = torch.randn(M, C, generator=g)
    if kind == "const":
        x[:, ::3] = x[0, ::3]
    elif kind == "shift":
        x = 100.0 + 0.1 * x
    bet = 0.1 * torch.randn(C, generator=g)
    # keep the pre-ReLU values of the ill-conditioned inputs away from the gate, so that the elements the
    # reference must leave out stay below 0.1 %: a constant column's value is beta itself, and a mean-100
    # column carries an absolute error of ~1e-4 per unit of c (the randn input exercises the gate)
    res = torch.randn(M, C, generator=g)
    if kind == "const":  # (rstd = eps^-1/2 = 316 there: the bound of such an element is ~1e-3 |x|)
        bet[::3] = bet[::3].abs() + 0.3
        res[:, ::3] = res[:, ::3].abs()
    elif kind == "shift":
        bet = bet + 4.0
    return dict(x=x, gam=1 + 0.1 * torch.randn(C, generator=g), bet=bet,
                res=res, dy=torch.randn(M, C, generator=g),
                rm=0.1 * torch.randn(C, generator=g), rv=0.5 + torch.rand(C, generator=g))


def call_bn_fwd(x, gam, bet, rm, rv, nbt, train, mom, eps, res, relu, thr, sc, seed, y, mean, rstd, M, C):
    o = ops()
    return L().fer_batchnorm_fwd(o.dcode(x), x.data_ptr(), x.stride(0), ptr(gam), ptr(bet), ptr(rm), ptr(rv), ptr(nbt),
                                 int(train), mom, eps, ptr(res), C if res is None else res.stride(0), int(relu), thr,
                                 sc, seed, y.data_ptr(), y.stride(0), ptr(mean), ptr(rstd), M, C, o.stream())


def call_bn_bwd(dy, x, mean, rstd, gam, bet, res, relu, thr, sc, seed, train, dx, dres, dgam, dbet, acc, M, C):
    o = ops()
    return L().fer_batchnorm_bwd(o.dcode(x), dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), ptr(mean),
                                 ptr(rstd), ptr(gam), ptr(bet), ptr(res), C if res is None else res.stride(0),
                                 int(relu), thr, sc, seed, int(train), ptr(dx), C if dx is None else dx.stride(0),
                                 ptr(dres), C if dres is None else dres.stride(0), ptr(dgam), ptr(dbet), int(acc), M,
                                 C, o.stream())


def bn_case(dtype, M, C, kind, epi, p, pad, train=True, seed=0x5EEDBA5E, memo=None):
    """One forward + backward pair, each launched twice. memo (shared by the cases of one (dtype, M, C,
    kind)) keeps what does not depend on the padding or on p: the host keep mask per p, the float64 /
    float32 forward reference per epilogue, the backward reference per (epilogue, p)."""
    o = ops()
    memo = {} if memo is None else memo

    def cached(key, fn):
        if key not in memo:
            memo[key] = fn()
        return memo[key]

    dt = tdt(dtype)
    out_round = BF_ROUND if dtype == "bf16" else 0.0
    mode = "train" if train else "eval"
    tag = f"bn[{dtype} M{M} C{C} {kind} {epi} p{p} pad{pad} {mode}]"
    rtag = f"bn[{dtype} M{M} C{C} {kind} {epi} p{p} {mode}]"
    relu, use_res = EPIS[epi]["relu"], EPIS[epi]["res"]
    inp = bn_inputs(M, C, kind)
    mom, eps = f32v(0.1), f32v(1e-5)
    thr, sc = o.drop_args(p)
    sc = f32v(sc)
    xd, _ = nanview(M, C, pad, dt, inp["x"])
    rd = nanview(M, C, pad, dt, inp["res"])[0] if use_res else None
    dyd, _ = nanview(M, C, pad, dt, inp["dy"])
    gd, bd = inp["gam"].to(DEV), inp["bet"].to(DEV)
    # the exact values the kernels see (the same for every padding)
    x, dy, res_all = cached("inputs", lambda: (exact(xd), exact(dyd), exact(nanview(M, C, 0, dt, inp["res"])[0])))
    res = res_all if use_res else None
    gam, bet, rm0, rv0 = (inp[k].double() for k in ("gam", "bet", "rm", "rv"))
    keep = cached(("keep", p), lambda: keep_mask(seed, (M, C), p)) if p > 0 else None

    # ---- forward, twice (bit-identical repeat), fresh running buffers each time
    outs = []
    for _ in range(2):
        yd, yp = nanview(M, C, pad, dt)
        mean, rstd = (torch.full((C,), float("nan"), device=DEV) for _ in range(2))
        rm, rv = inp["rm"].to(DEV), inp["rv"].to(DEV)
        nbt = torch.zeros((), dtype=torch.int64, device=DEV)
        rc = call_bn_fwd(xd, gd, bd, rm, rv, nbt, train, mom, eps, rd, relu, thr, sc, seed, yd, mean, rstd, M, C)
        assert rc == 0, last_error()
        outs.append((yp, mean, rstd, rm, rv, yd, nbt))
    for a, b, n in zip(outs[0][:5], outs[1][:5], ("y parent", "mean", "rstd", "running_mean", "running_var")):
        assert_bits_equal(f"{tag} repeat {n}", a, b)
    yp, mean, rstd, rm, rv, yd, nbt = outs[0]
    untouched(tag + " y", yp, M, C)
    assert int(nbt) == (1 if train else 0)

    def fwd_ref():
        f = {}
        f["v"], f["mean"], f["rstd"], f["rm"], f["rv"] = R.batchnorm(x, gam, bet, rm0, rv0, train, mom, eps, res=res)
        f["s_v"] = (x.abs() + f["mean"].abs()) * f["rstd"] * gam.abs() + bet.abs() + (res.abs() if use_res else 0)
        v32, mean32, rstd32, rm32, rv32 = R.batchnorm(x.float(), gam.float(), bet.float(), rm0.float(), rv0.float(),
                                                      train, mom, eps, res=None if res is None else res.float())
        f["s_mean"] = x.abs().mean(0) if train else rm0.abs()
        f["c_v"] = measure_c(rtag + ".y", dtype, [(v32, f["v"], f["s_v"])])
        f["c_mean"] = measure_c(rtag + ".mean", dtype, [(mean32, f["mean"], f["s_mean"])])
        f["c_rstd"] = measure_c(rtag + ".rstd", dtype, [(rstd32, f["rstd"], f["rstd"])])
        # elements whose pre-ReLU value is within its own bound of zero: the gate may fall either way
        f["out"] = (f["v"].abs() <= f["c_v"] * U * f["s_v"]) if relu else torch.zeros(M, C, dtype=torch.bool)
        assert f["out"].double().mean().item() <= 1e-3, f"{rtag}: the reference leaves out {f['out'].sum().item()} elements"
        f["y"] = torch.relu(f["v"]) if relu else f["v"]
        if train:
            var_u = ((x - f["mean"]) ** 2).sum(0) / (M - 1)
            f["s_rm"], f["s_rv"] = 0.9 * rm0.abs() + 0.1 * f["s_mean"], 0.9 * rv0 + 0.1 * var_u
            f["c_rm"] = measure_c(rtag + ".running_mean", dtype, [(rm32, f["rm"], f["s_rm"])])
            f["c_rv"] = measure_c(rtag + ".running_var", dtype, [(rv32, f["rv"], f["s_rv"])])
        return f

    F = cached(("fwd", epi, train), fwd_ref)
    y_ref, s_y = F["y"], F["s_v"]
    got_y = exact(yd)
    if keep is not None:
        y_ref, s_y = torch.where(keep, y_ref * sc, torch.zeros((), dtype=F64)), s_y * sc
        assert (got_y[~keep] == 0).all(), f"{tag}: a dropped element is not exactly 0"
    if F["out"].any():
        ok = ~F["out"]
        assert_close(tag + ".y", got_y[ok], y_ref[ok], s_y[ok], F["c_v"], out_round)
    else:
        assert_close(tag + ".y", got_y, y_ref, s_y, F["c_v"], out_round)
    assert_close(tag + ".mean", mean, F["mean"], F["s_mean"], F["c_mean"], 0.0)
    assert_close(tag + ".rstd", rstd, F["rstd"], F["rstd"], F["c_rstd"], 0.0)
    if train:
        assert_close(tag + ".running_mean", rm, F["rm"], F["s_rm"], F["c_rm"], 0.0)
        assert_close(tag + ".running_var", rv, F["rv"], F["s_rv"], F["c_rv"], 0.0)
    else:
        assert_bits_equal(tag + " running_mean unchanged", rm, inp["rm"].to(DEV))
        assert_bits_equal(tag + " running_var unchanged", rv, inp["rv"].to(DEV))

    # ---- backward with the fp32 statistics the forward saved, twice
    m64, r64 = exact(mean), exact(rstd)

    def bwd_ref():
        b = dict(m64=m64, r64=r64, gate=None, near=None, cols_ok=torch.ones(C, dtype=torch.bool))
        xh = (x - m64) * r64
        if relu:
            vb = xh * gam + bet + (res if use_res else 0)
            s_vb = xh.abs() * gam.abs() + bet.abs() + (res.abs() if use_res else 0)
            b["gate"] = vb > 0
            b["near"] = vb.abs() <= 16 * U * s_vb  # one fma and one add from the values at hand
            assert b["near"].double().mean().item() <= 1e-3, \
                f"{rtag}: the reference leaves out {b['near'].sum().item()} elements"
            b["cols_ok"] = ~b["near"].any(0)
        b["dx"], b["g"], b["dg"], b["db"] = R.batchnorm_bwd(dy, x, m64, r64, gam, bet, train, res=res, relu=relu,
                                                            keep=keep, scale=sc, gate=b["gate"])
        dx32, _, dg32, db32 = R.batchnorm_bwd(dy.float(), x.float(), m64.float(), r64.float(), gam.float(),
                                              bet.float(), train, res=None if res is None else res.float(),
                                              relu=relu, keep=keep, scale=sc, gate=b["gate"])
        xha = (x.abs() + m64.abs()) * r64
        b["ga"] = b["g"].abs()
        b["s_db"], b["s_dg"] = b["ga"].sum(0), (b["ga"] * xha).sum(0)
        b["s_dx"] = gam.abs() * r64 * (b["ga"] + (b["s_db"] / M + xha * (b["s_dg"] / M) if train else 0))
        b["c_dx"] = measure_c(rtag + ".dx", dtype, [(dx32, b["dx"], b["s_dx"])])
        b["c_dg"] = measure_c(rtag + ".dgamma", dtype, [(dg32, b["dg"], b["s_dg"])])
        b["c_db"] = measure_c(rtag + ".dbeta", dtype, [(db32, b["db"], b["s_db"])])
        return b

    Bk = cached(("bwd", epi, p, train), bwd_ref)
    # the statistics do not depend on the strides: the cached reference used the same bits
    assert torch.equal(Bk["m64"], m64) and torch.equal(Bk["r64"], r64), f"{tag}: mean / rstd depend on the padding"
    bouts = []
    for _ in range(2):
        dxd, dxp = nanview(M, C, pad, dt)
        drd, drp = nanview(M, C, pad, dt)
        dgam, dbet = torch.full((C,), 0.5, device=DEV), torch.full((C,), -0.25, device=DEV)
        rc = call_bn_bwd(dyd, xd, mean, rstd, gd, bd, rd, relu, thr, sc, seed, train, dxd, drd, dgam, dbet, 1, M, C)
        assert rc == 0, last_error()
        bouts.append((dxp, drp, dgam, dbet, dxd, drd))
    for a, b, n in zip(bouts[0][:4], bouts[1][:4], ("dx parent", "dres parent", "dgamma", "dbeta")):
        assert_bits_equal(f"{tag} repeat {n}", a, b)
    dxp, drp, dgam, dbet, dxd, drd = bouts[0]
    untouched(tag + " dx", dxp, M, C)
    untouched(tag + " dres", drp, M, C)
    got_dres, got_dx = exact(drd), exact(dxd)
    if keep is not None:
        assert (got_dres[~keep] == 0).all(), f"{tag}: dres of a dropped element is not exactly 0"
    cols_ok = Bk["cols_ok"]
    if cols_ok.all():
        assert_close(tag + ".dres", got_dres, Bk["g"], Bk["ga"], 16.0, out_round)
        assert_close(tag + ".dx", got_dx, Bk["dx"], Bk["s_dx"], Bk["c_dx"], out_round)
    else:
        el_ok = ~Bk["near"]
        assert_close(tag + ".dres", got_dres[el_ok], Bk["g"][el_ok], Bk["ga"][el_ok], 16.0, out_round)
        assert_close(tag + ".dx", got_dx[:, cols_ok], Bk["dx"][:, cols_ok], Bk["s_dx"][:, cols_ok], Bk["c_dx"], out_round)
    # accumulate = 1 on top of 0.5 / -0.25
    assert_close(tag + ".dgamma", exact(dgam)[cols_ok], (Bk["dg"] + 0.5)[cols_ok], (Bk["s_dg"] + 0.5)[cols_ok],
                 Bk["c_dg"], 0.0)
    assert_close(tag + ".dbeta", exact(dbet)[cols_ok], (Bk["db"] - 0.25)[cols_ok], (Bk["s_db"] + 0.25)[cols_ok],
                 Bk["c_db"], 0.0)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", BN_C)
@pytest.mark.parametrize("M", BN_M)
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_batchnorm_forward_backward(dtype, M, C, kind):
    """The full cross of epilogue x p x padding for every shape and input kind."""
    memo = {}
    for epi in EPIS:
        for p in (0.0, 0.3):
            for pad in (0, 8):
                bn_case(dtype, M, C, kind, epi, p, pad, memo=memo)


@pytest.mark.parametrize("epi", list(EPIS))
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_batchnorm_eval_mode(dtype, epi):
    """Running statistics normalise; nothing is updated. M = 1 is allowed in eval mode."""
    for M, C in ((1, 8), (37, 24), (36, 512)):
        for pad in (0, 8):
            bn_case(dtype, M, C, "randn", epi, 0.0, pad, train=False)


# ---------------------------------------------------------------------- seq mean, logits
@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("D", [8, 384, 512])
@pytest.mark.parametrize("B", [1, 2, 64])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_seq_mean(dtype, B, D, pad):
    o = ops()
    dt = tdt(dtype)
    out_round = BF_ROUND if dtype == "bf16" else 0.0
    Ls = 18
    g = torch.Generator().manual_seed(B * 1000 + D)
    xd, _ = nanview(B * Ls, D, pad, dt, torch.randn(B * Ls, D, generator=g) + 0.5)
    dyd, _ = nanview(B, D, pad, dt, torch.randn(B, D, generator=g))
    for _ in range(2):
        yd, yp = nanview(B, D, pad, dt)
        assert L().fer_seq_mean_fwd(o.dcode(xd), xd.data_ptr(), xd.stride(0), yd.data_ptr(), yd.stride(0), B, Ls, D,
                                    o.stream()) == 0, last_error()
        dxd, dxp = nanview(B * Ls, D, pad, dt)
        assert L().fer_seq_mean_bwd(o.dcode(dyd), dyd.data_ptr(), dyd.stride(0), dxd.data_ptr(), dxd.stride(0), B, Ls,
                                    D, o.stream()) == 0, last_error()
        if _ == 0:
            first = (yp.clone(), dxp.clone())
    assert_bits_equal("seq_mean repeat", yp, first[0])
    assert_bits_equal("seq_mean_bwd repeat", dxp, first[1])
    x, dy = exact(xd), exact(dyd)
    ref, scale = R.seq_mean(x, B, Ls), R.seq_mean(x.abs(), B, Ls)
    c = measure_c("seq_mean", dtype, [(R.seq_mean(x.float(), B, Ls), ref, scale)])
    assert_close("seq_mean", yd, ref, scale, c, out_round)
    untouched("seq_mean", yp, B, D)
    dref = (dy / Ls)[:, None, :].expand(B, Ls, D).reshape(B * Ls, D)
    assert_close("seq_mean_bwd", dxd, dref, dref.abs(), 16.0, out_round)
    untouched("seq_mean_bwd", dxp, B * Ls, D)


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("D", [8, 384, 512])
@pytest.mark.parametrize("B", [1, 2, 64])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_logits(dtype, B, D, pad):
    o = ops()
    dt = tdt(dtype)
    out_round = BF_ROUND if dtype == "bf16" else 0.0
    Cc = 7
    g = torch.Generator().manual_seed(B * 1000 + D + 1)
    xd, _ = nanview(B, D, pad, dt, torch.randn(B, D, generator=g))
    gd, _ = nanview(B, D, pad, dt, torch.rand(B, D, generator=g) * 1.4)
    W, bias = torch.randn(Cc, D, generator=g) / D ** 0.5, 0.1 * torch.randn(Cc, generator=g)
    dl = torch.randn(B, Cc, generator=g)
    Wd, bd_, dld = W.to(DEV), bias.to(DEV), dl.to(DEV)
    x, gt, W64, b64, dl64 = exact(xd), exact(gd), W.double(), bias.double(), dl.double()
    runs = []
    for _ in range(2):
        lp = torch.full((B + 2 * GUARD, Cc), float("nan"), device=DEV)
        lg = lp[GUARD:GUARD + B]
        assert L().fer_logits_fwd(o.dcode(xd), xd.data_ptr(), xd.stride(0), Wd.data_ptr(), bd_.data_ptr(),
                                  lg.data_ptr(), B, D, Cc, o.stream()) == 0, last_error()
        dxd, dxp = nanview(B, D, pad, dt)
        dW, db = torch.full((Cc, D), 0.5, device=DEV), torch.full((Cc,), -0.25, device=DEV)
        assert L().fer_logits_bwd(o.dcode(xd), xd.data_ptr(), xd.stride(0), Wd.data_ptr(), dld.data_ptr(),
                                  gd.data_ptr(), gd.stride(0), dxd.data_ptr(), dxd.stride(0), dW.data_ptr(),
                                  db.data_ptr(), 1, B, D, Cc, o.stream()) == 0, last_error()
        runs.append((lp, dxp, dW, db, lg, dxd))
    for a, b, n in zip(runs[0][:4], runs[1][:4], ("logits", "dx", "dW", "dbias")):
        assert_bits_equal(f"logits repeat {n}", a, b)
    lp, dxp, dW, db, lg, dxd = runs[0]
    ref, scale = R.logits(x, W64, b64), R.logits(x.abs(), W64.abs(), b64.abs())
    c = measure_c("logits_fwd", dtype, [(R.logits(x.float(), W, bias), ref, scale)])
    assert_close("logits_fwd", lg, ref, scale, c, 0.0)
    a = lp.clone()
    a[GUARD:GUARD + B] = 0
    b = torch.full_like(lp, float("nan"))
    b[GUARD:GUARD + B] = 0
    assert_bits_equal("logits guard rows", a, b)
    dx_ref, s_dx = (dl64 @ W64) * gt, (dl64.abs() @ W64.abs()) * gt
    dW_ref, s_dW = dl64.t() @ x + 0.5, dl64.abs().t() @ x.abs() + 0.5
    db_ref, s_db = dl64.sum(0) - 0.25, dl64.abs().sum(0) + 0.25
    c_dx = measure_c("logits_bwd.dx", dtype, [((dl @ W) * gt.float(), dx_ref, s_dx)])
    c_dW = measure_c("logits_bwd.dW", dtype, [(dl.t() @ x.float() + 0.5, dW_ref, s_dW)])
    c_db = measure_c("logits_bwd.dbias", dtype, [(dl.sum(0) - 0.25, db_ref, s_db)])
    assert_close("logits_bwd.dx", dxd, dx_ref, s_dx, c_dx, out_round)
    untouched("logits_bwd.dx", dxp, B, D)
    assert_close("logits_bwd.dW", dW, dW_ref, s_dW, c_dW, 0.0)
    assert_close("logits_bwd.dbias", db, db_ref, s_db, c_db, 0.0)


# ---------------------------------------------------------------------- argument rejections
def test_rejections_leave_outputs_untouched():
    """Every rejected call returns non-zero, sets fer_last_error and writes nothing."""
    o = ops()
    lib = L()
    st = o.stream()
    M, C, B, Ls = 36, 16, 2, 18
    for dtype in ("bf16", "fp32"):
        dt = tdt(dtype)
        code = 0 if dtype == "bf16" else 1
        x = torch.randn(M, C, device=DEV).to(dt)
        wide = torch.randn(M, 3 * C, device=DEV).to(dt)
        vec = lambda v=1.0: torch.full((C,), v, device=DEV)  # noqa: E731
        nbt = torch.zeros((), dtype=torch.int64, device=DEV)

        def rejected(name, fn, *outs):
            rc = fn()
            assert rc != 0, f"{name}: accepted"
            msg = last_error()
            assert msg and name.split(":")[0] in msg, (name, msg)
            for t in outs:
                all_nan(name, t)

        y = torch.full((M, 3 * C), float("nan"), dtype=dt, device=DEV)
        small = torch.full((M, C), float("nan"), dtype=dt, device=DEV)
        stat = torch.full((2, C), float("nan"), device=DEV)
        odd = C + (4 if dtype == "bf16" else 2)  # not a multiple of the piece
        # conv1d_cols
        rejected("conv1d_cols: dtype", lambda: lib.fer_conv1d_cols(7, x.data_ptr(), C, y.data_ptr(), 3 * C, B, Ls, C, st), y)
        rejected("conv1d_cols: B", lambda: lib.fer_conv1d_cols(code, x.data_ptr(), C, y.data_ptr(), 3 * C, 0, Ls, C, st), y)
        rejected("conv1d_cols: C", lambda: lib.fer_conv1d_cols(code, x.data_ptr(), C, y.data_ptr(), 3 * C, B, Ls, 3, st), y)
        rejected("conv1d_cols: ldc", lambda: lib.fer_conv1d_cols(code, x.data_ptr(), C, y.data_ptr(), 3 * C - 8, B, Ls, C, st), y)
        rejected("conv1d_cols: align", lambda: lib.fer_conv1d_cols(code, x.data_ptr(), C, y.data_ptr() + 4, 3 * C, B, Ls, C, st), y)
        rejected("conv1d_cols: element count", lambda: lib.fer_conv1d_cols(code, x.data_ptr(), 8, y.data_ptr(), 24, 1 << 30, 1 << 10, 8, st), y)
        rejected("conv1d_cols: null", lambda: lib.fer_conv1d_cols(code, None, C, y.data_ptr(), 3 * C, B, Ls, C, st), y)
        # conv1d_cols_bwd
        rejected("conv1d_cols_bwd: C", lambda: lib.fer_conv1d_cols_bwd(code, wide.data_ptr(), 3 * C, None, C, small.data_ptr(), C, B, Ls, C - 2, st), small)
        rejected("conv1d_cols_bwd: ldd", lambda: lib.fer_conv1d_cols_bwd(code, wide.data_ptr(), C, None, C, small.data_ptr(), C, B, Ls, C, st), small)
        rejected("conv1d_cols_bwd: dtype", lambda: lib.fer_conv1d_cols_bwd(4, wide.data_ptr(), 3 * C, None, C, small.data_ptr(), C, B, Ls, C, st), small)
        rejected("conv1d_cols_bwd: B", lambda: lib.fer_conv1d_cols_bwd(code, wide.data_ptr(), 3 * C, None, C, small.data_ptr(), C, 0, Ls, C, st), small)
        rejected("conv1d_cols_bwd: L", lambda: lib.fer_conv1d_cols_bwd(code, wide.data_ptr(), 3 * C, None, C, small.data_ptr(), C, B, -1, C, st), small)
        rejected("conv1d_cols_bwd: dx align", lambda: lib.fer_conv1d_cols_bwd(code, wide.data_ptr(), 3 * C, None, C, small.data_ptr() + 4, C, B, Ls, C, st), small)
        rejected("conv1d_cols_bwd: element count", lambda: lib.fer_conv1d_cols_bwd(code, wide.data_ptr(), 24, None, 8, small.data_ptr(), 8, 1 << 30, 1 << 11, 8, st), small)
        rejected("conv1d_cols_bwd: res", lambda: lib.fer_conv1d_cols_bwd(code, wide.data_ptr(), 3 * C, x.data_ptr() + 2, C, small.data_ptr(), C, B, Ls, C, st), small)
        # batchnorm_fwd
        g, b, rm, rv = vec(), vec(0.0), vec(0.0), vec()

        def bnf(**kw):
            a = dict(dtype=code, x=x.data_ptr(), ldx=C, g=g.data_ptr(), b=b.data_ptr(), rm=rm.data_ptr(), rv=rv.data_ptr(),
                     train=1, mom=0.1, eps=1e-5, res=None, ldr=C, thr=0, y=small.data_ptr(), ldy=C, M=M, C=C)
            a.update(kw)
            return lib.fer_batchnorm_fwd(a["dtype"], a["x"], a["ldx"], a["g"], a["b"], a["rm"], a["rv"], nbt.data_ptr(),
                                         a["train"], a["mom"], a["eps"], a["res"], a["ldr"], 1, a["thr"], 1.0, 1,
                                         a["y"], a["ldy"], stat[0].data_ptr(), stat[1].data_ptr(), a["M"], a["C"], st)

        for name, kw in (("dtype", dict(dtype=3)), ("M1 train", dict(M=1)), ("M0", dict(M=0)), ("C", dict(C=C - 2)),
                         ("ldx", dict(ldx=odd)), ("ldy", dict(ldy=C - 8)), ("y align", dict(y=small.data_ptr() + 2)),
                         ("gamma null", dict(g=None)), ("beta null", dict(b=None)),
                         ("ldr", dict(res=x.data_ptr(), ldr=odd)), ("dropout range", dict(thr=19661, M=1 << 28)),
                         ("eval without stats", dict(train=0, rm=None)),
                         ("momentum", dict(mom=1.5)), ("eps", dict(eps=-1.0)),
                         ("res align", dict(res=x.data_ptr() + 2))):
            rejected(f"batchnorm_fwd: {name}", lambda kw=kw: bnf(**kw), small, stat)
        assert int(nbt) == 0 and (rm == 0).all() and (rv == 1).all()
        # batchnorm_bwd
        mean, rstd = vec(0.0), vec()
        dgb = torch.full((2, C), float("nan"), device=DEV)

        def bnb(**kw):
            a = dict(dtype=code, dy=x.data_ptr(), x=x.data_ptr(), mean=mean.data_ptr(), dx=small.data_ptr(), lddx=C,
                     dg=dgb[0].data_ptr(), db=dgb[1].data_ptr(), M=M, C=C, res=None, thr=0)
            a.update(kw)
            return lib.fer_batchnorm_bwd(a["dtype"], a["dy"], C, a["x"], C, a["mean"], rstd.data_ptr(), g.data_ptr(),
                                         b.data_ptr(), a["res"], C, 1, a["thr"], 1.0, 1, 1, a["dx"], a["lddx"], None, C,
                                         a["dg"], a["db"], 0, a["M"], a["C"], st)

        for name, kw in (("dtype", dict(dtype=-1)), ("M0", dict(M=0)), ("C", dict(C=C + 2)), ("mean null", dict(mean=None)),
                         ("no output", dict(dx=None, dg=None, db=None)), ("dy null", dict(dy=None)),
                         ("lddx", dict(lddx=odd)), ("res align", dict(res=x.data_ptr() + 2)),
                         ("dropout range", dict(thr=19661, M=1 << 28))):
            rejected(f"batchnorm_bwd: {name}", lambda kw=kw: bnb(**kw), small, dgb)
        # seq mean
        pooled = torch.full((B, C), float("nan"), dtype=dt, device=DEV)
        rejected("seq_mean_fwd: L", lambda: lib.fer_seq_mean_fwd(code, x.data_ptr(), C, pooled.data_ptr(), C, B, 0, C, st), pooled)
        rejected("seq_mean_fwd: C", lambda: lib.fer_seq_mean_fwd(code, x.data_ptr(), C, pooled.data_ptr(), C, B, Ls, C - 2, st), pooled)
        rejected("seq_mean_fwd: ldy", lambda: lib.fer_seq_mean_fwd(code, x.data_ptr(), C, pooled.data_ptr(), C - 8, B, Ls, C, st), pooled)
        rejected("seq_mean_bwd: dtype", lambda: lib.fer_seq_mean_bwd(9, pooled.data_ptr(), C, small.data_ptr(), C, B, Ls, C, st), small)
        rejected("seq_mean_bwd: C", lambda: lib.fer_seq_mean_bwd(code, pooled.data_ptr(), C, small.data_ptr(), C, B, Ls, C - 2, st), small)
        rejected("seq_mean_bwd: lddx", lambda: lib.fer_seq_mean_bwd(code, x.data_ptr(), C, small.data_ptr(), odd, B, Ls, C, st), small)
        # logits
        W, lg = torch.randn(7, C, device=DEV), torch.full((B, 7), float("nan"), device=DEV)
        dl = torch.randn(B, 7, device=DEV)
        dW = torch.full((7, C), float("nan"), device=DEV)
        rejected("logits_fwd: dtype", lambda: lib.fer_logits_fwd(5, x.data_ptr(), C, W.data_ptr(), None, lg.data_ptr(), B, C, 7, st), lg)
        rejected("logits_fwd: B", lambda: lib.fer_logits_fwd(code, x.data_ptr(), C, W.data_ptr(), None, lg.data_ptr(), 0, C, 7, st), lg)
        rejected("logits_fwd: ldx", lambda: lib.fer_logits_fwd(code, x.data_ptr(), C - 1, W.data_ptr(), None, lg.data_ptr(), B, C, 7, st), lg)
        rejected("logits_fwd: W null", lambda: lib.fer_logits_fwd(code, x.data_ptr(), C, None, None, lg.data_ptr(), B, C, 7, st), lg)
        rejected("logits_fwd: logits null", lambda: lib.fer_logits_fwd(code, x.data_ptr(), C, W.data_ptr(), None, None, B, C, 7, st), lg)
        rejected("logits_bwd: gate ldg", lambda: lib.fer_logits_bwd(code, x.data_ptr(), C, W.data_ptr(), dl.data_ptr(), x.data_ptr(), C - 1, small.data_ptr(), C, dW.data_ptr(), None, 0, B, C, 7, st), dW, small)
        rejected("logits_bwd: no output", lambda: lib.fer_logits_bwd(code, x.data_ptr(), C, W.data_ptr(), dl.data_ptr(), None, C, None, C, None, None, 0, B, C, 7, st), dW)
        rejected("logits_bwd: dlogits null", lambda: lib.fer_logits_bwd(code, x.data_ptr(), C, W.data_ptr(), None, None, C, small.data_ptr(), C, dW.data_ptr(), None, 0, B, C, 7, st), dW, small)
        rejected("logits_bwd: dW without x", lambda: lib.fer_logits_bwd(code, None, C, W.data_ptr(), dl.data_ptr(), None, C, small.data_ptr(), C, dW.data_ptr(), None, 0, B, C, 7, st), dW, small)
        rejected("logits_bwd: lddx", lambda: lib.fer_logits_bwd(code, x.data_ptr(), C, W.data_ptr(), dl.data_ptr(), None, C, small.data_ptr(), C - 1, dW.data_ptr(), None, 0, B, C, 7, st), dW, small)
    torch.cuda.synchronize()


def test_python_wrapper_raises_on_one_row_in_train_mode():
    o = ops()
    x = torch.randn(1, 8, device=DEV)
    one = torch.ones(8, device=DEV)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        o.batchnorm_fwd(x, one, one, one.clone(), one.clone(), None, True)
    y, _, _ = o.batchnorm_fwd(x, one, one, torch.zeros(8, device=DEV), one.clone(), None, False)
    assert torch.isfinite(y).all()
