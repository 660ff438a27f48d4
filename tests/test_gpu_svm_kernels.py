"""fer_svm_forward and fer_svm_xtr against the float64 restatement (tests/svm_ref.py), through the raw C ABI with
tight and padded row strides (tests/abi_harness.py): every output a view into a NaN-filled parent whose guard
rows and padding must keep their bits, outputs not asked for all NaN, a repeat call bit-identical.

Bounds (DESIGN.md sections 2.1, 2.9): |got - ref| <= c 2^-23 scale, c = 4 x the error of float32 torch on the CPU
against the same restatement (floor 16); scale = sum_f |x w| + |b| for Z, sum_i |r x| for G, sum_i |r| for gb,
sum_i c a m^2 for the loss. R and Dw switch on the sign of m: their bound carries Z's, and an element whose
reference |m| lies inside Z's bound may take either branch, so its `extra` term is the distance between the two
branches (|R| or Dw of the active branch).

Shapes: N = 1, 5, 67 and the slab's neighbourhood (slab - 1, slab, slab + 1, 2 slab + 3: one row short of a slab,
whole slabs, a slab with a one-row and a three-row successor), max_groups * slab + 1 (two slabs per group, F cut
into one chunk), F = 1, 7 (no whole piece), 64, 301 (pieces and a one-element tail, more than one wave of
pieces), 9216 (the real width: F cut into chunks), P = 1, 7, 8. Tight strides of an odd F take the
element-by-element path, padded ones (a multiple of 4) the 16-byte one."""
import numpy as np
import pytest
import torch

import svm_ref as R
from abi_harness import DEV, all_nan, last_error, lib, nanvec, nanview, ops, ptr, untouched, untouched_vec
from elemwise import U, assert_bits_equal, assert_close, measure_c

pytestmark = pytest.mark.gpu


SLAB, MAX_GROUPS = 32, 128  # include/fervit.h FER_SVM_SLAB, FER_SVM_MAX_GROUPS (checked against the library below)
SHAPES = [(1, 1, 1), (5, 7, 7), (67, 64, 8), (SLAB - 1, 301, 7), (SLAB, 301, 8), (SLAB + 1, 64, 1), (2 * SLAB + 3, 301, 7),
          (5, 9216, 7), (67, 9216, 8), (MAX_GROUPS * SLAB + 1, 64, 7)]


def slab():
    return SLAB


def padding(F, padded):
    """Extra columns of a row operand of width F: none (tight), or 8 and up to the next multiple of 4, so that
    the padded stride takes the 16-byte path whatever F is."""
    return 8 + (-F) % 4 if padded else 0


def case(N, F, P, seed):
    """X, W, bias, labels (class P - 1 never occurs in the first slab; class 0 never occurs at all when P > 2),
    classes, Cp, Cn as CPU tensors."""
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(N, F, generator=g)
    W = torch.randn(P, F, generator=g) / max(1.0, F ** 0.5)
    b = torch.randn(P, generator=g) * 0.1
    lo = 1 if P > 2 else 0
    y = torch.randint(lo, max(lo + 1, P), (N,), generator=g)
    y[:slab()][y[:slab()] == P - 1] = lo
    classes = torch.arange(P, dtype=torch.int64)
    Cp = torch.rand(P, generator=g) + 0.5
    Cn = torch.rand(P, generator=g) * 0.1 + 0.05
    return X, W, b, y, classes, Cp, Cn


def ws_for(N, F):
    n = lib().fer_svm_ws(N, F)
    return torch.empty(max(1, n // 4), device=DEV), n


def run_forward(X, W, b, y, classes, Cp, Cn, pad, epilogue=0, Dw_in=None, want_z=True):
    N, F = X.shape
    P = W.shape[0]
    xv, _ = nanview(N, F, padding(F, pad), torch.float32, src=X, align=4)
    wv, _ = nanview(P, F, padding(F, pad), torch.float32, src=W, align=4)
    cp = 3 if pad else 0
    z, zp = nanview(N, P, cp, torch.float32, align=4)
    r, rp = nanview(N, P, cp, torch.float32, align=4)
    d, dp = nanview(N, P, cp, torch.float32, src=Dw_in, align=4)
    loss, lossp = nanvec(P)
    ws, nws = ws_for(N, F)
    dev = [t.to(DEV) for t in (b, y, classes, Cp, Cn)]
    rc = lib().fer_svm_forward(ptr(xv), xv.stride(0), ptr(wv), wv.stride(0), ptr(dev[0]), N, F, P, epilogue, ptr(dev[1]),
                               ptr(dev[2]), ptr(dev[3]), ptr(dev[4]), ptr(z) if want_z else None, z.stride(0), ptr(r),
                               r.stride(0), ptr(d), d.stride(0), ptr(loss), ptr(ws), nws, ops().stream())
    torch.cuda.synchronize()
    assert rc == 0, last_error()
    untouched("R", rp, N, P)
    untouched("Dw", dp, N, P)
    if want_z:
        untouched("Z", zp, N, P)
    else:
        all_nan("Z", zp)
    if epilogue == 0:
        untouched_vec("loss", lossp, P)
    else:
        all_nan("loss", lossp)
    return z, r, d, loss


def run_xtr(X, Rm, pad, want_g=True, want_gb=True):
    N, F = X.shape
    P = Rm.shape[1]
    xv, _ = nanview(N, F, padding(F, pad), torch.float32, src=X, align=4)
    rv, _ = nanview(N, P, 3 if pad else 0, torch.float32, src=Rm, align=4)
    G, Gp = nanview(P, F, padding(F, pad), torch.float32, align=4)
    gb, gbp = nanvec(P)
    ws, nws = ws_for(N, F)
    rc = lib().fer_svm_xtr(ptr(xv), xv.stride(0), ptr(rv), rv.stride(0), N, F, P, ptr(G) if want_g else None, G.stride(0),
                           ptr(gb) if want_gb else None, ptr(ws), nws, ops().stream())
    torch.cuda.synchronize()
    assert rc == 0, last_error()
    untouched("G", Gp, P, F) if want_g else all_nan("G", Gp)
    untouched_vec("gb", gbp, P) if want_gb else all_nan("gb", gbp)
    return G, gb


def forward_ref(X, W, b, y, classes, Cp, Cn):
    """The restatement on the fp32 values, and the bound's scales."""
    Xd, Wd, bd = X.double().numpy(), W.double().numpy(), b.double().numpy()
    s = np.where(y.numpy()[:, None] == classes.numpy()[None, :], 1.0, -1.0)
    c = np.where(s > 0, Cp.double().numpy()[None, :], Cn.double().numpy()[None, :])
    Z, m, Rr, Dw, loss = R.parts(Xd, Wd, bd, s, c)
    zscale = np.abs(Xd) @ np.abs(Wd).T + np.abs(bd)[None, :]
    return Z, m, Rr, Dw, loss, zscale, c


def torch_f32_forward(X, W, b, y, classes, Cp, Cn):
    Z = X @ W.T + b
    s = torch.where(y[:, None] == classes[None, :], 1.0, -1.0)
    c = torch.where(s > 0, Cp[None, :], Cn[None, :])
    m = 1 - s * Z
    ca = torch.where(m > 0, c, torch.zeros_like(c))
    return Z, ca * s * m, ca, (ca * m * m).sum(0)


@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("N,F,P", SHAPES)
def test_forward_hinge_and_scale_against_the_restatement(N, F, P, pad):
    args = case(N, F, P, 7 * N + F + P)
    X, W, b, y, classes, Cp, Cn = args
    Z, m, Rr, Dw, loss, zscale, c = forward_ref(*args)
    tz, tr, td, tl = torch_f32_forward(*args)
    name = f"({N},{F},{P}) pad={pad}"
    cz = measure_c(f"svm Z {name}", "fp32", [(tz, Z, zscale)])
    # a flip of the branch moves R by c |m| and Dw by c; inside Z's bound of m = 0 either branch is right
    zb = cz * U * zscale
    near = np.abs(m) <= zb
    r_extra, d_extra = np.where(near, c * np.abs(m) + c * zb, 0.0), np.where(near, c, 0.0)
    l_extra = (c * (2 * np.abs(m) * zb + zb * zb)).sum(0)  # the loss moves with Z: d(c m^2) <= c (2 |m| dz + dz^2)
    cl = measure_c(f"svm loss {name}", "fp32", [(tl, loss, loss + l_extra, l_extra)])
    z, r, d, l = run_forward(*args, pad)
    assert_close(f"{name} Z", z, Z, zscale, cz, 0.0)
    # R = c a s m inherits Z's error times c, plus its own roundings (a few 2^-23 |R|)
    assert_close(f"{name} R", r, Rr, c * zscale + np.abs(Rr), cz, 0.0, extra=r_extra)
    assert_close(f"{name} Dw", d, Dw, np.zeros_like(Dw), cz, 0.0, extra=d_extra)
    assert_close(f"{name} loss", l, loss, loss + l_extra, cl, 0.0, extra=l_extra)
    # without Z the other outputs hold the same bits; a repeat call too
    z2, r2, d2, l2 = run_forward(*args, pad, want_z=False)
    for nm, a_, b_ in (("R", r2, r), ("Dw", d2, d), ("loss", l2, l)):
        assert_bits_equal(f"{name} {nm} without Z", a_.contiguous(), b_.contiguous())
    z3, r3, d3, l3 = run_forward(*args, pad)
    for nm, a_, b_ in (("Z", z3, z), ("R", r3, r), ("Dw", d3, d), ("loss", l3, l)):
        assert_bits_equal(f"{name} {nm} repeat", a_.contiguous(), b_.contiguous())
    # scale epilogue: R = Dw Z with the weights just produced (exact inputs), Dw left as it was
    dw_in = d.contiguous().cpu()
    zs, rs, ds, _ = run_forward(*args, pad, epilogue=1, Dw_in=dw_in)
    assert_bits_equal(f"{name} scale Z", zs.contiguous(), z.contiguous())
    assert_bits_equal(f"{name} scale keeps Dw", ds.contiguous().cpu(), dw_in)
    want = dw_in.double().numpy() * Z
    assert_close(f"{name} scale R", rs, want, dw_in.double().numpy() * zscale + np.abs(want), cz, 0.0)


@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("N,F,P", SHAPES)
def test_xtr_against_the_restatement(N, F, P, pad):
    g = torch.Generator().manual_seed(N + 3 * F + P)
    X = torch.randn(N, F, generator=g)
    Rm = torch.randn(N, P, generator=g) * (torch.rand(N, P, generator=g) > 0.3)
    Rm[:, P - 1][:slab()] = 0  # a column with nothing in the first slab
    Xd, Rd = X.double().numpy(), Rm.double().numpy()
    Gr, gbr = Rd.T @ Xd, Rd.sum(0)
    gscale, gbscale = np.abs(Rd).T @ np.abs(Xd), np.abs(Rd).sum(0)
    name = f"({N},{F},{P}) pad={pad}"
    c = measure_c(f"svm xtr {name}", "fp32", [(Rm.T @ X, Gr, gscale), (Rm.sum(0), gbr, gbscale)])
    G, gb = run_xtr(X, Rm, pad)
    assert_close(f"{name} G", G, Gr, gscale, c, 0.0)
    assert_close(f"{name} gb", gb, gbr, gbscale, c, 0.0)
    G2, _ = run_xtr(X, Rm, pad, want_gb=False)
    _, gb2 = run_xtr(X, Rm, pad, want_g=False)
    assert_bits_equal(f"{name} G alone", G2.contiguous(), G.contiguous())
    assert_bits_equal(f"{name} gb alone", gb2.contiguous(), gb.contiguous())
    G3, gb3 = run_xtr(X, Rm, pad)
    assert_bits_equal(f"{name} G repeat", G3.contiguous(), G.contiguous())
    assert_bits_equal(f"{name} gb repeat", gb3.contiguous(), gb.contiguous())


def test_a_column_with_every_margin_inactive_is_exactly_zero():
    """Column 1: a huge bias of the right sign puts every sample beyond its margin: Dw = 0, R = 0, loss 0, and the
    column's G and gb are 0 exactly."""
    N, F, P = 2 * slab() + 3, 301, 3
    X, W, b, y, classes, Cp, Cn = case(N, F, P, 5)
    y[:] = 2
    W[1] = 0
    b[1] = -50.0  # class 1 never occurs: s = -1 everywhere, m = 1 - 50 < 0
    z, r, d, l = run_forward(X, W, b, y, classes, Cp, Cn, 1)
    assert (r[:, 1] == 0).all() and (d[:, 1] == 0).all() and l[1].item() == 0.0
    assert (d[:, 0] != 0).any() or (d[:, 2] != 0).any()
    G, gb = run_xtr(X, r.contiguous().cpu(), 1)
    assert (G[1] == 0).all() and gb[1].item() == 0.0


def test_rejections_leave_the_outputs_untouched():
    N, F, P = 5, 64, 7
    X, W, b, y, classes, Cp, Cn = case(N, F, P, 1)
    xv, _ = nanview(N, F, 8, torch.float32, src=X)
    wv, _ = nanview(P, F, 8, torch.float32, src=W)
    z, zp = nanview(N, P, 3, torch.float32, align=4)
    r, rp = nanview(N, P, 3, torch.float32, align=4)
    d, dp = nanview(N, P, 3, torch.float32, align=4)
    G, Gp = nanview(P, F, 8, torch.float32)
    loss, lossp = nanvec(P)
    ws, nws = ws_for(N, F)
    dv = [t.to(DEV) for t in (b, y, classes, Cp, Cn)]
    L, st = lib(), ops().stream()

    def fwd(**over):
        a = dict(X=ptr(xv), ldx=xv.stride(0), W=ptr(wv), ldw=wv.stride(0), bias=ptr(dv[0]), N=N, F=F, P=P, ep=0,
                 labels=ptr(dv[1]), classes=ptr(dv[2]), Cp=ptr(dv[3]), Cn=ptr(dv[4]), Z=ptr(z), ldz=z.stride(0), R=ptr(r),
                 ldr=r.stride(0), Dw=ptr(d), ldd=d.stride(0), loss=ptr(loss), ws=ptr(ws), nws=nws)
        a.update(over)
        return L.fer_svm_forward(*a.values(), st)

    def xtr(**over):
        a = dict(X=ptr(xv), ldx=xv.stride(0), R=ptr(r), ldr=r.stride(0), N=N, F=F, P=P, G=ptr(G), ldg=G.stride(0),
                 gb=ptr(loss), ws=ptr(ws), nws=nws)
        a.update(over)
        return L.fer_svm_xtr(*a.values(), st)

    cases = [("svm_forward", "F must be >= 1", lambda: fwd(F=0)), ("svm_forward", "P must be 1..8", lambda: fwd(P=9)),
             ("svm_forward", "P must be 1..8", lambda: fwd(P=0)), ("svm_forward", "row stride >= F", lambda: fwd(ldx=F - 1)),
             ("svm_forward", "X is required", lambda: fwd(X=None)), ("svm_forward", "workspace", lambda: fwd(nws=nws - 4)),
             ("svm_forward", "workspace", lambda: fwd(ws=ptr(ws) + 4)), ("svm_forward", "workspace", lambda: fwd(ws=None)),
             ("svm_forward", "epilogue must be", lambda: fwd(ep=2)), ("svm_forward", "W (row stride", lambda: fwd(ldw=F - 1)),
             ("svm_forward", "W (row stride", lambda: fwd(bias=None)), ("svm_forward", "R and Dw", lambda: fwd(ldr=P - 1)),
             ("svm_forward", "R and Dw", lambda: fwd(Dw=None)), ("svm_forward", "Z's row stride", lambda: fwd(ldz=P - 1)),
             ("svm_forward", "hinge epilogue needs", lambda: fwd(labels=None)),
             ("svm_forward", "hinge epilogue needs", lambda: fwd(loss=None)),
             ("svm_xtr", "P must be 1..8", lambda: xtr(P=9)), ("svm_xtr", "R is required", lambda: xtr(R=None)),
             ("svm_xtr", "R is required", lambda: xtr(ldr=P - 1)), ("svm_xtr", "no output requested", lambda: xtr(G=None, gb=None)),
             ("svm_xtr", "G's row stride", lambda: xtr(ldg=F - 1)), ("svm_xtr", "workspace", lambda: xtr(nws=0))]
    for entry, msg, call in cases:
        L.fer_set_persistent_mode(0)  # a success does not clear the message
        assert call() != 0, msg
        assert last_error().startswith(entry + ":") and msg in last_error(), (msg, last_error())
    assert fwd(N=0) == 0 and xtr(N=0) == 0  # an empty problem is a no-op
    torch.cuda.synchronize()
    for nm, p in (("Z", zp), ("R", rp), ("Dw", dp), ("G", Gp), ("loss", lossp)):
        all_nan(nm, p)


def test_wrappers_match_the_abi_calls():
    N, F, P = 67, 301, 7
    args = case(N, F, P, 9)
    X, W, b, y, classes, Cp, Cn = args
    z, r, d, l = run_forward(*args, 0)
    dv = [t.to(DEV) for t in args]
    R2, D2, l2, Z2 = ops().svm_hinge(*dv, want_z=True)
    for nm, a_, b_ in (("Z", Z2, z), ("R", R2, r), ("Dw", D2, d), ("loss", l2, l)):
        assert_bits_equal(nm, a_, b_.contiguous())
    assert_bits_equal("decision", ops().svm_decision(dv[0], dv[1], dv[2]), z.contiguous())
    G, gb = run_xtr(X, r.contiguous().cpu(), 0)
    G2, gb2 = ops().svm_xtr(dv[0], R2)
    assert_bits_equal("G", G2, G.contiguous())
    assert_bits_equal("gb", gb2, gb.contiguous())
    S = ops().svm_scale(dv[0], dv[1], dv[2], D2)
    assert_bits_equal("scale", S, D2 * Z2)
    assert ops().svm_slab() == lib().fer_svm_slab() == SLAB and lib().fer_svm_max_groups() == MAX_GROUPS
    with pytest.raises(ValueError):
        ops().svm_xtr(dv[0], torch.zeros(N, 9, device=DEV))
