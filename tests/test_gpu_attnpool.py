"""Element-wise checks of the LatentCNNDeep kernels (csrc/attnpool.hip) through the C ABI against
tests/cnn_deep_ref.py in float64 on the CPU, computed from the exact values handed to the kernel.

Bound: |got - ref| <= out_round * |ref| + c * 2^-23 * scale_i, out_round 2^-8 for
a bf16 output and 0 for fp32; c is measured per case from the same formulas in float32 torch on the CPU
(x 4, floor 16, printed as `c-measure attnpool ...` lines), never from the kernel. Results below a format's
normal range get that format's absolute underflow on top (`close`).

Scales, with S_b = max_l sum_c |x_lc w_c| + |bias| (how far a score's own rounding can move the exponent)
and k_b = 1 + 2 S_b:
  probs  a_l k_b                               y        k_b sum_l a_l |x_lc|
  da     sum_c |dy_c x_lc|                     ds       k_b a_l (s(da_l) + sum_l' a_l' s(da_l'))
  dx     k_b a_l |dy_c| + s(ds_l) |w_c|        dw_part  sum_l s(ds_l) |x_lc|  (the reduced dw: summed over b)
  dbias  sum_l s(ds_l)
The backward is handed the probabilities the forward kernel saved, and its reference starts from those.

Shapes: L in {1, 2, 5, 18, 37, 257} (softmax == 1 with ds exactly 0; not a multiple of the four waves; more
rows than threads) x B in {1, 3} x C in {8, 24, 512, 2056 bf16 / 1028 fp32 (more than 256 pieces)}, and the
model's B = 64, L = 18, C = 512. Inputs: randn (bias null and non-null), constant rows (probs = 1 / L),
w x 30 (near one-hot, small probabilities underflow), x + 100 with sum(w) != 0 (scores ~ 1e3: overflow
without the max subtraction). Every output is a view into a NaN-filled parent with guard rows and, in the
padded run, padded strides; the padding must keep its bits and the results hold no NaN. Each call runs
twice (bit-identical repeat); probs = null gives the same y bits."""
import pytest
import torch

import cnn_deep_ref as D
from abi_harness import (all_nan, exact, f32v, last_error, lib, nanvec, nanview, ops, ptr, tdt, untouched,
                         untouched_vec)
from dropmask import keep_mask
from elemwise import BF_ROUND, U, assert_bits_equal, assert_close, measure_c

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
KINDS = ("randn", "nobias", "const", "sharp", "shift")


def close(name, got, ref, scale, c, out_round):
    """assert_close with the output format's underflow added to the bound. The near-one-hot inputs make
    probabilities, and with them dx = a dy + ds w, as small as the formats go, and below a format's normal
    range its rounding error is no longer relative (out_round * |ref|, 2^-23 * scale) but absolute: half a
    subnormal spacing, 2^-150 for an fp32 result (twice: the stored value and one fp32 intermediate, the
    product a dy) and 2^-134 for a bf16 one on top. The term is given to assert_close as scale units."""
    tiny = 2.0 ** -149 + (2.0 ** -134 if out_round else 0.0)
    assert_close(name, got, ref, torch.as_tensor(scale).double() + tiny / (c * U), c, out_round)


def call_fwd(x, w, bias, y, probs, B, L, C):
    o = ops()
    return lib().fer_attnpool_fwd(o.dcode(x), x.data_ptr(), x.stride(0), ptr(w), ptr(bias), y.data_ptr(), y.stride(0),
                                  ptr(probs), B, L, C, o.stream())


def call_bwd(dy, x, w, probs, dx, dw_part, db_part, B, L, C):
    o = ops()
    return lib().fer_attnpool_bwd(o.dcode(x), dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), ptr(w),
                                  ptr(probs), ptr(dx), C if dx is None else dx.stride(0), ptr(dw_part), ptr(db_part),
                                  B, L, C, o.stream())


def make_inputs(B, L, C, kind):
    g = torch.Generator().manual_seed(B * 100000 + L * 100 + C + KINDS.index(kind))
    x = torch.randn(B, L, C, generator=g)
    w = torch.randn(C, generator=g) / C ** 0.5
    bias = None if kind == "nobias" else torch.tensor([0.3])
    if kind == "const":
        x = x[:, :1].expand(B, L, C).contiguous()
    elif kind == "sharp":
        w = w * 30.0
    elif kind == "shift":
        x = x + 100.0
        w = w + 10.0 / C  # sum(w) ~ 10: scores ~ 1e3
    return x.reshape(B * L, C), w, bias, torch.randn(B, C, generator=g)


def pool_case(dtype, B, L, C, kind):
    """Forward + backward of one (shape, input kind), tight and padded; the references are shared by the
    two paddings (the kernels see the same values)."""
    o = ops()
    dt = tdt(dtype)
    out_round = BF_ROUND if dtype == "bf16" else 0.0
    tag = f"attnpool[{dtype} B{B} L{L} C{C} {kind}]"
    x0, w, bias, dy0 = make_inputs(B, L, C, kind)
    wd, bd = w.to(DEV), None if bias is None else bias.to(DEV)
    w64, b64 = w.double(), None if bias is None else bias.double()
    ref = None
    for pad in (0, 8):
        xd, _ = nanview(B * L, C, pad, dt, x0)
        dyd, _ = nanview(B, C, pad, dt, dy0)
        # ---- forward, twice, then once without probs
        runs = []
        for _ in range(2):
            yd, yp = nanview(B, C, pad, dt)
            pv, pp = nanvec(B * L)
            assert call_fwd(xd, wd, bd, yd, pv, B, L, C) == 0, last_error()
            runs.append((yp, pp, yd, pv))
        assert_bits_equal(tag + " repeat y", runs[0][0], runs[1][0])
        assert_bits_equal(tag + " repeat probs", runs[0][1], runs[1][1])
        yp, pp, yd, pv = runs[0]
        y2, y2p = nanview(B, C, pad, dt)
        assert call_fwd(xd, wd, bd, y2, None, B, L, C) == 0, last_error()
        assert_bits_equal(tag + " y without probs", y2p, yp)
        untouched(tag + " y", yp, B, C)
        untouched_vec(tag + " probs", pp, B * L)
        if ref is None:
            x, dy = exact(xd), exact(dyd)
            x3 = x.reshape(B, L, C)
            y_ref, a = D.attnpool(x, w64, b64, B, L)
            S = (x3.abs() @ w64.abs()).max(1).values + (0.0 if b64 is None else b64.abs().item())
            k = (1.0 + 2.0 * S)[:, None]
            s_a = a * k
            s_y = k * (a[:, :, None] * x3.abs()).sum(1)
            y32, a32 = D.attnpool(x.float(), w, bias, B, L)
            ref = dict(x=x, dy=dy, y=y_ref, a=a, k=k, s_a=s_a, s_y=s_y,
                       c_a=measure_c(tag + ".probs", dtype, [(a32, a, s_a)]),
                       c_y=measure_c(tag + ".y", dtype, [(y32, y_ref, s_y)]))
        else:
            assert torch.equal(ref["x"], exact(xd)) and torch.equal(ref["dy"], exact(dyd))
        x, dy, a, k = ref["x"], ref["dy"], ref["a"], ref["k"]
        x3 = x.reshape(B, L, C)
        got_a, got_y = exact(pv).reshape(B, L), exact(yd)
        assert torch.isfinite(got_a).all() and torch.isfinite(got_y).all(), tag
        close(tag + ".probs", got_a, a, ref["s_a"], ref["c_a"], 0.0)
        close(tag + ".y", got_y, ref["y"], ref["s_y"], ref["c_y"], out_round)
        if kind == "const":
            close(tag + ".probs = 1/L", got_a, torch.full((B, L), 1.0 / L, dtype=F64), ref["s_a"], ref["c_a"], 0.0)
        if L == 1:
            assert (got_a == 1).all(), tag

        # ---- backward from the probabilities the kernel saved, twice
        if "bwd" not in ref or not torch.equal(ref["bwd"]["a_k"], got_a):
            dx_r, dw_r, db_r, da_r, ds_r = D.attnpool_bwd(dy, x, w64, got_a, B, L)
            s_da = (x3.abs() * dy.abs()[:, None, :]).sum(2)
            s_ds = k * got_a * (s_da + (got_a * s_da).sum(1, keepdim=True))
            s_dx = (k * got_a)[:, :, None] * dy.abs()[:, None, :] + s_ds[:, :, None] * w64.abs()
            s_dw = (s_ds[:, :, None] * x3.abs()).sum(1)
            s_db = s_ds.sum(1)
            dx32, dw32, db32, _, _ = D.attnpool_bwd(dy.float(), x.float(), w, got_a.float(), B, L)
            bw = dict(a_k=got_a, dx=dx_r, dw=dw_r, db=db_r, ds=ds_r, s_dx=s_dx.reshape(B * L, C), s_dw=s_dw, s_db=s_db,
                      c_dx=measure_c(tag + ".dx", dtype, [(dx32, dx_r, s_dx.reshape(B * L, C))]),
                      c_dw=measure_c(tag + ".dw_part", dtype, [(dw32, dw_r, s_dw)]),
                      c_db=measure_c(tag + ".dbias_part", dtype, [(db32, db_r, s_db)]),
                      c_dws=measure_c(tag + ".dw", dtype, [(dw32.sum(0) + 0.5, dw_r.sum(0) + 0.5, s_dw.sum(0) + 0.5)]),
                      c_dbs=measure_c(tag + ".dbias", dtype, [(db32.sum() - 0.25, db_r.sum() - 0.25, s_db.sum() + 0.25)]))
            ref["bwd"] = bw
        bw = ref["bwd"]
        bruns = []
        for _ in range(2):
            dxd, dxp = nanview(B * L, C, pad, dt)
            dwd, dwp = nanview(B, C, 0, torch.float32)
            dbv, dbp = nanvec(B)
            assert call_bwd(dyd, xd, wd, pv, dxd, dwd, dbv, B, L, C) == 0, last_error()
            bruns.append((dxp, dwp, dbp, dxd, dwd, dbv))
        for i, n in enumerate(("dx", "dw_part", "dbias_part")):
            assert_bits_equal(f"{tag} repeat {n}", bruns[0][i], bruns[1][i])
        dxp, dwp, dbp, dxd, dwd, dbv = bruns[0]
        untouched(tag + " dx", dxp, B * L, C)
        untouched(tag + " dw_part", dwp, B, C)
        untouched_vec(tag + " dbias_part", dbp, B)
        close(tag + ".dx", dxd, bw["dx"], bw["s_dx"], bw["c_dx"], out_round)
        close(tag + ".dw_part", dwd, bw["dw"], bw["s_dw"], bw["c_dw"], 0.0)
        close(tag + ".dbias_part", dbv, bw["db"], bw["s_db"], bw["c_db"], 0.0)
        if L == 1:  # softmax == 1: ds is exactly 0, dx is dy
            assert (exact(dbv) == 0).all() and (exact(dwd) == 0).all(), tag
            assert_bits_equal(tag + " dx == dy", dxd.contiguous(), dyd.contiguous())
        # each output alone gives the same bits
        only_dx, odp = nanview(B * L, C, pad, dt)
        assert call_bwd(dyd, xd, wd, pv, only_dx, None, None, B, L, C) == 0, last_error()
        assert_bits_equal(tag + " dx alone", odp, dxp)
        only_db, obp = nanvec(B)
        assert call_bwd(dyd, xd, wd, pv, None, None, only_db, B, L, C) == 0, last_error()
        assert_bits_equal(tag + " dbias_part alone", obp, dbp)
        # ---- the wrapper's reduced parameter gradients, accumulated on top of 0.5 / -0.25, twice
        red = []
        for _ in range(2):
            dw, db = torch.full((1, C, 1), 0.5, device=DEV), torch.full((1,), -0.25, device=DEV)
            dx_w = o.attnpool_bwd(dyd, xd, wd, pv, B, L, dw=dw, dbias=db, accumulate=True)
            red.append((dw, db, dx_w))
        assert_bits_equal(tag + " repeat dw", red[0][0], red[1][0])
        assert_bits_equal(tag + " repeat dbias", red[0][1], red[1][1])
        assert_bits_equal(tag + " wrapper dx", red[0][2], dxd.contiguous())
        close(tag + ".dw", red[0][0], bw["dw"].sum(0) + 0.5, bw["s_dw"].sum(0) + 0.5, bw["c_dws"], 0.0)
        close(tag + ".dbias", red[0][1], bw["db"].sum() - 0.25, bw["s_db"].sum() + 0.25, bw["c_dbs"], 0.0)


def big_c(dtype):
    return 2056 if dtype == "bf16" else 1028  # 257 pieces: more than one per thread


@pytest.mark.parametrize("Cn", [8, 24, 512, "big"])
@pytest.mark.parametrize("L", [1, 2, 5, 18, 37, 257])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_attnpool_forward_backward(dtype, L, Cn):
    C = big_c(dtype) if Cn == "big" else Cn
    for B in (1, 3):
        for kind in KINDS:
            pool_case(dtype, B, L, C, kind)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_attnpool_at_the_model_size(dtype):
    pool_case(dtype, 64, 18, 512, "randn")


def test_wrapper_matches_the_abi_call():
    o = ops()
    B, L, C = 3, 18, 24
    x0, w, bias, _ = make_inputs(B, L, C, "randn")
    for dt in (torch.bfloat16, torch.float32):
        x, wd, bd = x0.to(DEV).to(dt), w.to(DEV).reshape(1, C, 1), bias.to(DEV)
        y, probs = o.attnpool_fwd(x, wd, bd, B, L)
        y2 = torch.empty_like(y)
        p2 = torch.empty_like(probs)
        assert call_fwd(x, wd, bd, y2, p2, B, L, C) == 0, last_error()
        assert_bits_equal("wrapper y", y, y2)
        assert_bits_equal("wrapper probs", probs, p2)
        y3, none = o.attnpool_fwd(x, wd, bd, B, L, want_probs=False)
        assert none is None
        assert_bits_equal("wrapper y, no probs", y3, y)
        with pytest.raises(ValueError):
            o.attnpool_fwd(x, wd, bd, B, L + 1)
        with pytest.raises(ValueError):
            o.attnpool_fwd(x, wd[:, :8], bd, B, L)


def test_attnpool_rejections_leave_outputs_untouched():
    """Every rejected call returns non-zero, sets fer_last_error and writes nothing."""
    from fervit._lib import lib as _l  # noqa: F401

    o = ops()
    st = o.stream()
    L_ = lib()
    B, Ls, C = 2, 18, 16
    for dtype in ("bf16", "fp32"):
        dt = tdt(dtype)
        code = 0 if dtype == "bf16" else 1
        odd = C + (4 if dtype == "bf16" else 2)  # not a multiple of the piece
        x = torch.randn(B * Ls, C, device=DEV).to(dt)
        dy = torch.randn(B, C, device=DEV).to(dt)
        w = torch.randn(C + 4, device=DEV)
        probs_in = torch.full((B * Ls,), 1.0 / Ls, device=DEV)
        y = torch.full((B, C), float("nan"), dtype=dt, device=DEV)
        probs = torch.full((B * Ls,), float("nan"), device=DEV)
        dx = torch.full((B * Ls, C), float("nan"), dtype=dt, device=DEV)
        dwp = torch.full((B, C), float("nan"), device=DEV)
        dbp = torch.full((B,), float("nan"), device=DEV)

        def rejected(name, rc, *outs):
            assert rc != 0, f"{name}: accepted"
            msg = last_error()
            assert msg and msg.startswith(name.split(":")[0] + ":"), (name, msg)
            for t in outs:
                all_nan(name, t)

        def fwd(**kw):
            a = dict(dtype=code, x=x.data_ptr(), ldx=C, w=w.data_ptr(), y=y.data_ptr(), ldy=C, B=B, L=Ls, C=C)
            a.update(kw)
            return L_.fer_attnpool_fwd(a["dtype"], a["x"], a["ldx"], a["w"], None, a["y"], a["ldy"], probs.data_ptr(),
                                       a["B"], a["L"], a["C"], st)

        for name, kw in (("dtype", dict(dtype=7)), ("C % V", dict(C=C - 2)), ("B", dict(B=0)), ("L0", dict(L=0)),
                         ("L limit", dict(L=4097)), ("ldx short", dict(ldx=C - 8)), ("ldx piece", dict(ldx=odd)),
                         ("ldy short", dict(ldy=C - 8)), ("x align", dict(x=x.data_ptr() + 4)),
                         ("y align", dict(y=y.data_ptr() + 4)), ("x null", dict(x=None)), ("w null", dict(w=None)),
                         ("w align", dict(w=w.data_ptr() + 4))):
            rejected(f"attnpool_fwd: {name}", fwd(**kw), y, probs)

        def bwd(**kw):
            a = dict(dtype=code, dy=dy.data_ptr(), lddy=C, x=x.data_ptr(), ldx=C, w=w.data_ptr(), p=probs_in.data_ptr(),
                     dx=dx.data_ptr(), lddx=C, dw=dwp.data_ptr(), db=dbp.data_ptr(), B=B, L=Ls, C=C)
            a.update(kw)
            return L_.fer_attnpool_bwd(a["dtype"], a["dy"], a["lddy"], a["x"], a["ldx"], a["w"], a["p"], a["dx"],
                                       a["lddx"], a["dw"], a["db"], a["B"], a["L"], a["C"], st)

        for name, kw in (("dtype", dict(dtype=-1)), ("C % V", dict(C=C - 2)), ("L limit", dict(L=4097)),
                         ("B", dict(B=-1)), ("no output", dict(dx=None, dw=None, db=None)),
                         ("lddy short", dict(lddy=C - 8)), ("ldx piece", dict(ldx=odd)), ("lddx piece", dict(lddx=odd)),
                         ("dx align", dict(dx=dx.data_ptr() + 4)), ("dy null", dict(dy=None)),
                         ("probs null", dict(p=None)), ("w null", dict(w=None)),
                         ("dw_part align", dict(dw=dwp.data_ptr() + 4))):
            rejected(f"attnpool_bwd: {name}", bwd(**kw), dx, dwp, dbp)

        def rd(which, **kw):
            a = dict(dtype=code, x=x.data_ptr(), ldx=C, y=dx.data_ptr(), ldy=C, M=B * Ls, C=C, thr=0)
            a.update(kw)
            if which == "fwd":
                return L_.fer_relu_dropout_fwd(a["dtype"], a["x"], a["ldx"], a["y"], a["ldy"], a["M"], a["C"], a["thr"],
                                               1.0, 1, st)
            return L_.fer_relu_dropout_bwd(a["dtype"], x.data_ptr(), C, a["x"], a["ldx"], a["y"], a["ldy"], a["M"],
                                           a["C"], a["thr"], 1.0, 1, st)

        for which in ("fwd", "bwd"):
            for name, kw in (("dtype", dict(dtype=5)), ("C % V", dict(C=C - 2)), ("M", dict(M=0)),
                             ("ldx short", dict(ldx=C - 8)), ("ldy piece", dict(ldy=odd)),
                             ("y align", dict(y=dx.data_ptr() + 4)), ("x null", dict(x=None)),
                             ("dropout range", dict(thr=19661, M=1 << 28))):
                rejected(f"relu_dropout_{which}: {name}", rd(which, **kw), dx)


# ---------------------------------------------------------------------- ReLU + dropout
@pytest.mark.parametrize("p", [0.0, 0.15, 0.3])
@pytest.mark.parametrize("C", [8, 256])
@pytest.mark.parametrize("M", [1, 18, 72])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_relu_dropout(dtype, M, C, p):
    o = ops()
    dt = tdt(dtype)
    seed = 0x5EEDBA5E
    thr, sc = o.drop_args(p)
    sc = f32v(sc)
    g = torch.Generator().manual_seed(M * 1000 + C)
    x0 = torch.randn(M, C, generator=g)
    x0[0, 0], x0[0, 1], x0[M - 1, C - 1] = 0.0, -0.0, 0.0
    dy0 = torch.randn(M, C, generator=g)
    keep = keep_mask(seed, (M, C), p) if p > 0 else torch.ones(M, C, dtype=torch.bool)
    for pad in (0, 8):
        xd, _ = nanview(M, C, pad, dt, x0)
        dyd, _ = nanview(M, C, pad, dt, dy0)
        assert xd[0, 1].item() == 0 and torch.signbit(xd[0, 1]).item()
        outs = []
        for _ in range(2):
            yd, yp = nanview(M, C, pad, dt)
            dxd, dxp = nanview(M, C, pad, dt)
            assert lib().fer_relu_dropout_fwd(o.dcode(xd), xd.data_ptr(), xd.stride(0), yd.data_ptr(), yd.stride(0), M, C,
                                              thr, sc, seed, o.stream()) == 0, last_error()
            assert lib().fer_relu_dropout_bwd(o.dcode(xd), dyd.data_ptr(), dyd.stride(0), xd.data_ptr(), xd.stride(0),
                                              dxd.data_ptr(), dxd.stride(0), M, C, thr, sc, seed, o.stream()) == 0, \
                last_error()
            outs.append((yp, dxp, yd, dxd))
        assert_bits_equal("relu_dropout repeat y", outs[0][0], outs[1][0])
        assert_bits_equal("relu_dropout repeat dx", outs[0][1], outs[1][1])
        yp, dxp, yd, dxd = outs[0]
        untouched("relu_dropout y", yp, M, C)
        untouched("relu_dropout dx", dxp, M, C)
        xc, dyc = xd.cpu().contiguous(), dyd.cpu().contiguous()
        gate = xc.float() > 0
        zero = torch.zeros((), dtype=dt)
        if p == 0:
            assert_bits_equal("relu", yd.cpu().contiguous(), torch.where(gate, xc, zero))
            assert_bits_equal("relu bwd", dxd.cpu().contiguous(), torch.where(gate, dyc, zero))
        else:
            got_y, got_dx = exact(yd), exact(dxd)
            live = gate & keep
            assert (got_y[~live] == 0).all() and (got_dx[~live] == 0).all(), "a gated or dropped element is not exactly 0"
            # the keep decisions are exactly the host mask's: every kept, gated-in element is non-zero
            assert (got_y[live] != 0).all()
            assert (got_dx[live & (dyc.double() != 0)] != 0).all()
            y_ref = torch.where(live, xc.double() * sc, torch.zeros((), dtype=F64))
            dx_ref = torch.where(live, dyc.double() * sc, torch.zeros((), dtype=F64))
            c, rnd = (0.0, BF_ROUND) if dtype == "bf16" else (1.0, 0.0)  # 2^-8 relative / one fp32 ulp
            assert_close("relu_dropout y", got_y, y_ref, y_ref.abs(), c, rnd)
            assert_close("relu_dropout dx", got_dx, dx_ref, dx_ref.abs(), c, rnd)
        assert yd[0, 0].item() == 0 and yd[0, 1].item() == 0 and dxd[0, 0].item() == 0 and dxd[0, 1].item() == 0
        # the wrappers make the same calls
        assert_bits_equal("wrapper fwd", o.relu_dropout_fwd(xd, dropout=p, seed=seed), yd.contiguous())
        assert_bits_equal("wrapper bwd", o.relu_dropout_bwd(dyd, xd, dropout=p, seed=seed), dxd.contiguous())
