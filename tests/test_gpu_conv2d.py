"""Element-wise checks of the LatentCNN2D kernels (csrc/conv2d.hip) through the C ABI against
tests/cnn2d_ref.py on the CPU, computed from the exact values handed to the kernel.

Copies (im2col, the pool and its backward without dropout) are compared bit for bit. Sums use the bound of
DESIGN.md section 2.1, |got - ref| <= out_round * |ref| + c * 2^-23 * scale_i against float64, out_round 2^-8
for a bf16 output and 0 for fp32; c is measured per case from the same formulas in float32 torch on the CPU
(x 4, floor 16, printed as `c-measure conv2d...` lines), never from the kernel. Scales:
  cols adjoint  sum of |terms|                       y   |bias| + sum_k |x9 w|
  dw            sum_m |dy x9|    dbias  sum_m |dy|    dx  sum_k sum_co |dy w|
Every operand is a view into a NaN-filled parent with guard rows and, in the padded run, padded strides: the
padding must keep its bits, and a read outside a sample would carry a NaN into the result. Each call runs
twice (bit-identical repeat)."""
import pytest
import torch

import cnn2d_ref as D2
from abi_harness import all_nan, exact, f32v, last_error, lib, nanview, ops, tdt, untouched
from dropmask import keep_mask
from elemwise import BF_ROUND, assert_bits_equal, assert_close, measure_c

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
HW = [(1, 1), (1, 5), (2, 3), (3, 4), (9, 16)]


def out_round(dtype):
    return BF_ROUND if dtype == "bf16" else 0.0


def code(dtype):
    return 0 if dtype == "bf16" else 1


# ---------------------------------------------------------------------- im2col and its adjoint
@pytest.mark.parametrize("hw", HW)
@pytest.mark.parametrize("dtype,C", [("bf16", 8), ("bf16", 24), ("fp32", 4), ("fp32", 8), ("fp32", 24)])
def test_conv2d_cols_and_adjoint(dtype, C, hw):
    H, W = hw
    o = ops()
    dt = tdt(dtype)
    st = o.stream()
    for B in (1, 3):
        M = B * H * W
        tag = f"conv2d_cols[{dtype} B{B} H{H} W{W} C{C}]"
        g = torch.Generator().manual_seed(B * 1000 + H * 100 + W * 10 + C)
        x0 = torch.randn(M, C, generator=g)
        x0[x0 == 0] = 1.0  # a zero in cols is then a padding zero
        d0 = torch.randn(M, 9 * C, generator=g)
        ref = None
        for pad in (0, 8):
            xd, _ = nanview(M, C, pad, dt, x0)
            dd, _ = nanview(M, 9 * C, pad, dt, d0)
            runs = []
            for _ in range(2):
                cd, cp = nanview(M, 9 * C, pad, dt)
                gd, gp = nanview(M, C, pad, dt)
                assert lib().fer_conv2d_cols(code(dtype), xd.data_ptr(), xd.stride(0), cd.data_ptr(), cd.stride(0), B, H,
                                             W, C, st) == 0, last_error()
                assert lib().fer_conv2d_cols_bwd(code(dtype), dd.data_ptr(), dd.stride(0), gd.data_ptr(), gd.stride(0),
                                                 B, H, W, C, st) == 0, last_error()
                runs.append((cp, gp, cd, gd))
            assert_bits_equal(tag + " repeat cols", runs[0][0], runs[1][0])
            assert_bits_equal(tag + " repeat dx", runs[0][1], runs[1][1])
            cp, gp, cd, gd = runs[0]
            untouched(tag + " cols", cp, M, 9 * C)
            untouched(tag + " dx", gp, M, C)
            xc = xd.cpu().contiguous()
            assert_bits_equal(tag, cd.cpu().contiguous(), D2.conv2d_cols(xc, B, H, W))
            if ref is None:
                d64 = exact(dd)
                want = D2.conv2d_cols_bwd(d64, B, H, W)
                scale = D2.conv2d_cols_bwd(d64.abs(), B, H, W)
                c = measure_c(tag + ".adjoint", dtype, [(D2.conv2d_cols_bwd(d64.float(), B, H, W), want, scale)])
                ref = (want, scale, c)
            assert_close(tag + ".adjoint", gd, ref[0], ref[1], ref[2], out_round(dtype))
            # the wrappers make the same calls
            assert_bits_equal(tag + " wrapper", o.conv2d_cols(xd, B, H, W), cd.contiguous())
            assert_bits_equal(tag + " wrapper bwd", o.conv2d_cols_bwd(dd, B, H, W), gd.contiguous())


# ---------------------------------------------------------------------- first layer
def c1_case(dtype, B, H, W, Cout, with_bias):
    o = ops()
    dt = tdt(dtype)
    st = o.stream()
    M = B * H * W
    tag = f"conv2d_c1[{dtype} B{B} H{H} W{W} Cout{Cout} bias{int(with_bias)}]"
    g = torch.Generator().manual_seed(B * 100000 + H * 1000 + W + Cout)
    x0 = torch.randn(M, 1, generator=g)
    w = torch.randn(Cout, 1, 3, 3, generator=g) / 3.0
    bias = torch.randn(Cout, generator=g) if with_bias else None
    dy0 = torch.randn(M, Cout, generator=g)
    wd, bd = w.to(DEV), None if bias is None else bias.to(DEV)
    w64, b64 = w.double(), None if bias is None else bias.double()
    ref = None
    for pad in (0, 8):
        xd, _ = nanview(M, 1, pad, dt, x0, guard=8)
        dyd, _ = nanview(M, Cout, pad, dt, dy0)
        if ref is None:
            x, dy = exact(xd).reshape(-1), exact(dyd)
            x9 = D2.conv2d_cols(x.reshape(-1, 1), B, H, W)
            y_ref = D2.conv2d_c1(x, w64, b64, B, H, W)
            s_y = x9.abs() @ w64.reshape(Cout, 9).abs().t() + (0.0 if b64 is None else b64.abs())
            dw_r, db_r, dx_r = D2.conv2d_c1_bwd(dy, x, w64, B, H, W)
            s_dw = dy.abs().t() @ x9.abs()
            s_db = dy.abs().sum(0)
            s_dx = D2.conv2d_cols_bwd(dy.abs() @ w64.reshape(Cout, 9).abs(), B, H, W).reshape(-1)
            dw32, db32, dx32 = D2.conv2d_c1_bwd(dy.float(), x.float(), w, B, H, W)
            ref = dict(y=y_ref, s_y=s_y, dw=dw_r, db=db_r, dx=dx_r, s_dw=s_dw, s_db=s_db, s_dx=s_dx,
                       c_y=measure_c(tag + ".y", dtype, [(D2.conv2d_c1(x.float(), w, bias, B, H, W), y_ref, s_y)]),
                       c_dw=measure_c(tag + ".dw", dtype, [(dw32, dw_r, s_dw)]),
                       c_db=measure_c(tag + ".dbias", dtype, [(db32, db_r, s_db)]),
                       c_dx=measure_c(tag + ".dx", dtype, [(dx32, dx_r, s_dx)]))
        # ---- forward, twice
        runs = []
        for _ in range(2):
            yd, yp = nanview(M, Cout, pad, dt)
            assert lib().fer_conv2d_c1_fwd(code(dtype), xd.data_ptr(), xd.stride(0), wd.data_ptr(),
                                           None if bd is None else bd.data_ptr(), yd.data_ptr(), yd.stride(0), B, H, W,
                                           Cout, st) == 0, last_error()
            runs.append((yp, yd))
        assert_bits_equal(tag + " repeat y", runs[0][0], runs[1][0])
        untouched(tag + " y", runs[0][0], M, Cout)
        assert_close(tag + ".y", runs[0][1], ref["y"], ref["s_y"], ref["c_y"], out_round(dtype))
        # ---- backward: one strip, three strips and more strips than a small image has pixels
        for n_parts in (1, 3, 40):
            bruns = []
            for _ in range(2):
                pd, pp = nanview(n_parts, Cout * 9, 0, torch.float32)
                dxd, dxp = nanview(M, 1, pad, dt, guard=8)
                assert lib().fer_conv2d_c1_bwd(code(dtype), dyd.data_ptr(), dyd.stride(0), xd.data_ptr(), xd.stride(0),
                                               wd.data_ptr(), pd.data_ptr(), n_parts, dxd.data_ptr(), dxd.stride(0), B,
                                               H, W, Cout, st) == 0, last_error()
                bruns.append((pp, dxp, pd, dxd))
            assert_bits_equal(tag + " repeat dw_part", bruns[0][0], bruns[1][0])
            assert_bits_equal(tag + " repeat dx", bruns[0][1], bruns[1][1])
            pp, dxp, pd, dxd = bruns[0]
            untouched(tag + " dw_part", pp, n_parts, Cout * 9)
            untouched(tag + " dx", dxp, M, 1, guard=8)
            assert_close(tag + ".dx", dxd, ref["dx"], ref["s_dx"], ref["c_dx"], out_round(dtype))
            # the strips' rows added in order by fer_colsum, on top of 0.5
            dw = torch.full((Cout, 9), 0.5, device=DEV)
            o.colsum(pd, dw, accumulate=True)
            assert_close(f"{tag}.dw n_parts={n_parts}", dw, ref["dw"] + 0.5, ref["s_dw"] + 0.5, ref["c_dw"], 0.0)
            # each output alone gives the same bits
            only, op_ = nanview(n_parts, Cout * 9, 0, torch.float32)
            assert lib().fer_conv2d_c1_bwd(code(dtype), dyd.data_ptr(), dyd.stride(0), xd.data_ptr(), xd.stride(0), None,
                                           only.data_ptr(), n_parts, None, 1, B, H, W, Cout, st) == 0, last_error()
            assert_bits_equal(tag + " dw_part alone", op_, pp)
        db = torch.empty(Cout, device=DEV)
        o.colsum(dyd, db)
        assert_close(tag + ".dbias", db, ref["db"], ref["s_db"], ref["c_db"], 0.0)
    # the wrappers: same forward bits, the reduced gradient within the same bound
    xt = x0.reshape(B, H, W).to(DEV).to(dt)
    dyt = dy0.to(DEV).to(dt)
    yw = o.conv2d_c1_fwd(xt, wd, bd, B, H, W)
    assert_bits_equal(tag + " wrapper y", yw, runs[0][1].contiguous())
    gw = torch.zeros(Cout, 1, 3, 3, device=DEV)
    dxw = o.conv2d_c1_bwd(dyt, xt, wd, B, H, W, dw=gw, want_dx=True)
    assert dxw.shape == xt.shape
    assert_close(tag + ".dw wrapper", gw, ref["dw"], ref["s_dw"], ref["c_dw"], 0.0)
    assert_bits_equal(tag + " wrapper dx", dxw.reshape(-1), dxd.contiguous().reshape(-1))


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("Cout", [8, 64])
@pytest.mark.parametrize("hw", [(1, 1), (3, 5), (18, 32), (18, 512)])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_conv2d_first_layer(dtype, hw, Cout, with_bias):
    for B in (1, 2):
        c1_case(dtype, B, hw[0], hw[1], Cout, with_bias)


# ---------------------------------------------------------------------- MaxPool2d + Dropout2d
def pool_input(M, C, g):
    """What stands behind a ReLU: at least 30 % exact zeros; values on a grid bf16 holds, so windows tie."""
    x = torch.relu((torch.randn(M, C, generator=g) * 3).round() / 4)
    assert (x == 0).float().mean().item() >= 0.3 and x.unique().numel() < 40
    return x


@pytest.mark.parametrize("p", [0.0, 0.15, 0.5])
@pytest.mark.parametrize("pool", [0, 1])
@pytest.mark.parametrize("C", [8, 24, 64])
@pytest.mark.parametrize("hw", [(2, 2), (3, 5), (9, 16), (18, 32)])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_pool2_chdrop(dtype, hw, C, pool, p):
    H, W = hw
    o = ops()
    dt = tdt(dtype)
    st = o.stream()
    seed = 0x5EED2D00 + C
    thr, sc = o.drop_args(p)
    sc = f32v(sc)
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    for B in (1, 3):
        M, Mo = B * H * W, B * Ho * Wo
        tag = f"pool2_chdrop[{dtype} B{B} H{H} W{W} C{C} pool{pool} p{p}]"
        g = torch.Generator().manual_seed(B * 1000 + H * 100 + W + C)
        x0 = pool_input(M, C, g)
        dy0 = torch.randn(Mo, C, generator=g)
        dy0[dy0 == 0] = 1.0
        keep = keep_mask(seed, (B, C), p) if p > 0 else None
        for pad in (0, 8):
            xd, _ = nanview(M, C, pad, dt, x0)
            dyd, _ = nanview(Mo, C, pad, dt, dy0)
            runs = []
            for _ in range(2):
                yd, yp = nanview(Mo, C, pad, dt)
                dxd, dxp = nanview(M, C, pad, dt)
                assert lib().fer_pool2_chdrop_fwd(code(dtype), xd.data_ptr(), xd.stride(0), yd.data_ptr(), yd.stride(0), B,
                                                  H, W, C, pool, thr, sc, seed, st) == 0, last_error()
                assert lib().fer_pool2_chdrop_bwd(code(dtype), dyd.data_ptr(), dyd.stride(0), xd.data_ptr(), xd.stride(0),
                                                  dxd.data_ptr(), dxd.stride(0), B, H, W, C, pool, thr, sc, seed,
                                                  st) == 0, last_error()
                runs.append((yp, dxp, yd, dxd))
            assert_bits_equal(tag + " repeat y", runs[0][0], runs[1][0])
            assert_bits_equal(tag + " repeat dx", runs[0][1], runs[1][1])
            yp, dxp, yd, dxd = runs[0]
            untouched(tag + " y", yp, Mo, C)
            untouched(tag + " dx", dxp, M, C)
            xc, dyc = xd.cpu().contiguous(), dyd.cpu().contiguous()
            # the restatement without dropout, in the kernel's own dtype: copies, so bit for bit
            y_plain = D2.pool2_chdrop(xc, B, H, W, bool(pool))
            dx_plain = D2.pool2_chdrop_bwd(dyc, xc, B, H, W, bool(pool))
            if pool:
                ties = D2.pool_argmax(xc.float(), B, H, W)
                assert M < 64 or (ties[1] != 0).any()
            if p == 0:
                assert_bits_equal(tag + " y", yd.cpu().contiguous(), y_plain)
                assert_bits_equal(tag + " dx", dxd.cpu().contiguous(), dx_plain)
            else:
                got_y, got_dx = exact(yd).reshape(B, Ho * Wo, C), exact(dxd).reshape(B, H * W, C)
                drop = ~keep
                assert B * C < 64 or (drop.any() and keep.any())
                # dropped planes are exactly 0 in y and dx; kept planes are non-zero wherever the plain result is
                assert (got_y.permute(0, 2, 1)[drop] == 0).all() and (got_dx.permute(0, 2, 1)[drop] == 0).all(), tag
                yp64, dxp64 = y_plain.double().reshape(B, Ho * Wo, C), dx_plain.double().reshape(B, H * W, C)
                live = keep[:, None, :]
                assert ((got_y != 0) == ((yp64 != 0) & live)).all(), tag + ": keep planes differ from dropmask.keep_mask"
                # dx is non-zero exactly at the restatement's argmax pixels of kept planes
                assert ((got_dx != 0) == ((dxp64 != 0) & live)).all(), tag + ": dx outside the argmax pixel"
                y_ref = torch.where(live, yp64 * sc, torch.zeros((), dtype=F64))
                dx_ref = torch.where(live, dxp64 * sc, torch.zeros((), dtype=F64))
                c = 0.0 if dtype == "bf16" else 1.0  # one rounding of the product: 2^-8 relative / one fp32 ulp
                assert_close(tag + ".y", got_y, y_ref, y_ref.abs(), c, out_round(dtype))
                assert_close(tag + ".dx", got_dx, dx_ref, dx_ref.abs(), c, out_round(dtype))
            if pool:  # the pixels floor division leaves out
                d4 = dxd.reshape(B, H, W, C)
                assert (d4[:, 2 * Ho:] == 0).all() and (d4[:, :, 2 * Wo:] == 0).all()
            assert_bits_equal(tag + " wrapper fwd", o.pool2_chdrop_fwd(xd, B, H, W, pool, dropout=p, seed=seed),
                              yd.contiguous())
            assert_bits_equal(tag + " wrapper bwd", o.pool2_chdrop_bwd(dyd, xd, B, H, W, pool, dropout=p, seed=seed),
                              dxd.contiguous())


# ---------------------------------------------------------------------- rejections
def test_rejections_leave_outputs_untouched():
    """Every rejected call returns non-zero, sets fer_last_error and writes nothing."""
    o = ops()
    st = o.stream()
    L_ = lib()
    B, H, W, C = 2, 3, 4, 16
    M = B * H * W
    for dtype in ("bf16", "fp32"):
        dt = tdt(dtype)
        cd = code(dtype)
        odd = C + (4 if dtype == "bf16" else 2)  # not a multiple of the piece
        x = torch.randn(M, C, device=DEV).to(dt)
        img = torch.randn(M, device=DEV).to(dt)
        w = torch.randn(C + 4, 9, device=DEV)
        big = torch.randn(M, 9 * C, device=DEV).to(dt)

        def nan(*shape, dtype_=dt):
            return torch.full(shape, float("nan"), dtype=dtype_, device=DEV)

        cols, dx, y, ypool, dimg = nan(M, 9 * C), nan(M, C), nan(M, C), nan(B * (H // 2) * (W // 2), C), nan(M)
        part = nan(3, C * 9, dtype_=torch.float32)

        def rejected(name, rc, *outs):
            assert rc != 0, f"{name}: accepted"
            msg = last_error()
            assert msg and msg.startswith(name.split(":")[0] + ":"), (name, msg)
            for t in outs:
                all_nan(name, t)

        def f_cols(**kw):
            a = dict(dtype=cd, x=x.data_ptr(), ldx=C, c=cols.data_ptr(), ldc=9 * C, B=B, H=H, W=W, C=C)
            a.update(kw)
            return L_.fer_conv2d_cols(a["dtype"], a["x"], a["ldx"], a["c"], a["ldc"], a["B"], a["H"], a["W"], a["C"], st)

        for name, kw in (("dtype", dict(dtype=7)), ("C % V", dict(C=C - 2)), ("B", dict(B=0)), ("H", dict(H=0)),
                         ("W", dict(W=-1)), ("ldx short", dict(ldx=C - 8)), ("ldx piece", dict(ldx=odd)),
                         ("ldc short", dict(ldc=9 * C - 8)), ("ldc piece", dict(ldc=9 * C + odd - C)),
                         ("x align", dict(x=x.data_ptr() + 4)), ("cols align", dict(c=cols.data_ptr() + 4)),
                         ("x null", dict(x=None))):
            rejected(f"conv2d_cols: {name}", f_cols(**kw), cols)

        def f_colsb(**kw):
            a = dict(dtype=cd, d=big.data_ptr(), ldd=9 * C, dx=dx.data_ptr(), lddx=C, B=B, H=H, W=W, C=C)
            a.update(kw)
            return L_.fer_conv2d_cols_bwd(a["dtype"], a["d"], a["ldd"], a["dx"], a["lddx"], a["B"], a["H"], a["W"],
                                          a["C"], st)

        for name, kw in (("dtype", dict(dtype=-1)), ("C % V", dict(C=C - 2)), ("B", dict(B=0)),
                         ("ldd short", dict(ldd=9 * C - 8)), ("lddx piece", dict(lddx=odd)),
                         ("dx align", dict(dx=dx.data_ptr() + 4)), ("dcols null", dict(d=None))):
            rejected(f"conv2d_cols_bwd: {name}", f_colsb(**kw), dx)

        def f_c1(**kw):
            a = dict(dtype=cd, x=img.data_ptr(), ldx=1, w=w.data_ptr(), y=y.data_ptr(), ldy=C, B=B, H=H, W=W, C=C)
            a.update(kw)
            return L_.fer_conv2d_c1_fwd(a["dtype"], a["x"], a["ldx"], a["w"], None, a["y"], a["ldy"], a["B"], a["H"],
                                        a["W"], a["C"], st)

        for name, kw in (("dtype", dict(dtype=7)), ("Cout % V", dict(C=C - 2)), ("Cout limit", dict(C=1032, ldy=1032)),
                         ("B", dict(B=0)), ("ldx", dict(ldx=0)), ("ldy short", dict(ldy=C - 8)), ("ldy piece", dict(ldy=odd)),
                         ("y align", dict(y=y.data_ptr() + 4)), ("x null", dict(x=None)), ("w null", dict(w=None))):
            rejected(f"conv2d_c1_fwd: {name}", f_c1(**kw), y)

        def f_c1b(**kw):
            a = dict(dtype=cd, dy=x.data_ptr(), lddy=C, x=img.data_ptr(), ldx=1, w=w.data_ptr(), p=part.data_ptr(), n=3,
                     dx=dimg.data_ptr(), lddx=1, B=B, H=H, W=W, C=C)
            a.update(kw)
            return L_.fer_conv2d_c1_bwd(a["dtype"], a["dy"], a["lddy"], a["x"], a["ldx"], a["w"], a["p"], a["n"], a["dx"],
                                        a["lddx"], a["B"], a["H"], a["W"], a["C"], st)

        for name, kw in (("dtype", dict(dtype=7)), ("Cout % V", dict(C=C - 2)), ("no output", dict(p=None, dx=None)),
                         ("n_parts", dict(n=0)), ("lddy short", dict(lddy=C - 8)), ("lddy piece", dict(lddy=odd)),
                         ("dy align", dict(dy=x.data_ptr() + 4)), ("x null", dict(x=None)), ("w null", dict(w=None)),
                         ("lddx", dict(lddx=0)), ("dw_part align", dict(p=part.data_ptr() + 4))):
            rejected(f"conv2d_c1_bwd: {name}", f_c1b(**kw), part, dimg)

        def f_pool(which, **kw):
            a = dict(dtype=cd, x=x.data_ptr(), ldx=C, y=ypool.data_ptr(), ldy=C, dy=ypool.data_ptr(), dx=dx.data_ptr(),
                     lddx=C, B=B, H=H, W=W, C=C, pool=1, thr=0)
            a.update(kw)
            if which == "fwd":
                return L_.fer_pool2_chdrop_fwd(a["dtype"], a["x"], a["ldx"], a["y"], a["ldy"], a["B"], a["H"], a["W"],
                                               a["C"], a["pool"], a["thr"], 1.0, 1, st)
            return L_.fer_pool2_chdrop_bwd(a["dtype"], x.data_ptr(), C, a["x"], a["ldx"], a["dx"], a["lddx"], a["B"],
                                           a["H"], a["W"], a["C"], a["pool"], a["thr"], 1.0, 1, st)

        for which, out in (("fwd", ypool), ("bwd", dx)):
            for name, kw in (("dtype", dict(dtype=5)), ("pool with H = 1", dict(H=1)), ("pool with W = 1", dict(W=1)),
                             ("pool flag", dict(pool=2)), ("C % V", dict(C=C - 2)), ("B", dict(B=0)),
                             ("ldx short", dict(ldx=C - 8)), ("ldx piece", dict(ldx=odd)),
                             ("x align", dict(x=x.data_ptr() + 4)), ("x null", dict(x=None)),
                             ("thresh", dict(thr=65537)), ("dropout range", dict(thr=19661, B=1 << 29))):
                rejected(f"pool2_chdrop_{which}: {name}", f_pool(which, **kw), out)
        rejected("pool2_chdrop_fwd: ldy piece", f_pool("fwd", ldy=odd), ypool)
        rejected("pool2_chdrop_fwd: y align", f_pool("fwd", y=ypool.data_ptr() + 4), ypool)
        rejected("pool2_chdrop_bwd: lddx piece", f_pool("bwd", lddx=odd), dx)
        rejected("pool2_chdrop_bwd: dx align", f_pool("bwd", dx=dx.data_ptr() + 4), dx)
