"""fer_token_cosine against the float64 restatement (tests/metrics_ref.py cosine_ref), through the raw C ABI with
tight and padded row strides (tests/abi_harness.py), in both dtypes: the bf16 MFMA Gram kernel (one 16 x 16
tile per wave: N = 2, 10 inside one tile, 19 and 37 with a partial last tile, 197 with 13 tiles and more than
one workgroup per row tile; D = 32 one k-step, 192 a four-step round plus a tail, 512 and 768 whole rounds)
and the fp32 FMA kernel (8 rows j per wave, 32 per workgroup; D / 4 pieces over 64 lanes).

Bound: c 2^-23 scale, scale = sum_k |x_k y_k| / (max(|x|, eps) max(|y|, eps)), c from float32 torch's
cosine_similarity on the CPU against the same restatement on the same values (x 4, floor 16, DESIGN.md
section 2.1). bf16 tokens are exact inputs (the reference is taken on the values they hold) and the outputs
are fp32, so there is no output-rounding term."""
import numpy as np
import pytest
import torch

import metrics_ref as R
from abi_harness import DEV, all_nan, last_error, lib, nanview, ops, ptr, tdt, untouched
from elemwise import assert_bits_equal, assert_close, measure_c

pytestmark = pytest.mark.gpu

EPS = 1e-8
SHAPES = [(1, 2, 32), (3, 10, 192), (2, 19, 512), (1, 37, 512), (1, 197, 768)]


def tokens_of(kind, B, N, D, dtype, seed):
    """[B, N, D] in `dtype`. "special": randn with a zero row, a row of norm 3e-9 (the clamp at eps = 1e-8 is
    active), two identical rows, and in later batch elements a clamped / a zero CLS row; "mean100": every
    element around 100 (all products positive, cosines near 1)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, N, D, generator=g)
    if kind == "mean100":
        x = x + 100.0
    else:
        x[0, 1] *= 3e-9 / x[0, 1].norm()  # N = 2: CLS against a clamped row
        if N > 5:
            x[0, 2] = 0
            x[0, 4] = x[0, 3]
        if B > 1:
            x[1, 0] *= 3e-9 / x[1, 0].norm()
            x[1, N - 1] = 0
        if B > 2:
            x[2, 0] = 0
    return x.to(tdt(dtype))


def run(x, pad, want_cls=True, want_tok=True, eps=EPS):
    B, N, D = x.shape
    xv, xp = nanview(B * N, D, pad, x.dtype, src=x.reshape(B * N, D))
    cls, clsp = nanview(B, N - 1, 3 if pad else 0, torch.float32, align=4)
    tok, tokp = nanview(B * (N - 1), N - 1, 3 if pad else 0, torch.float32, align=4)
    rc = lib().fer_token_cosine(0 if x.dtype == torch.bfloat16 else 1, ptr(xv), xv.stride(0), B, N, D, eps,
                                ptr(cls) if want_cls else None, cls.stride(0), ptr(tok) if want_tok else None,
                                tok.stride(0), ops().stream())
    torch.cuda.synchronize()
    assert rc == 0, last_error()
    for name, v, p, rows, on in (("cls_sim", cls, clsp, B, want_cls), ("tok_sim", tok, tokp, B * (N - 1), want_tok)):
        if on:
            untouched(name, p, rows, N - 1)
        else:
            all_nan(name, p)
    return cls, tok.reshape(B, N - 1, N - 1)


def torch_f32(x):
    v = x.float()
    cls = torch.cosine_similarity(v[:, :1], v[:, 1:], dim=2, eps=EPS)
    tok = torch.cosine_similarity(v[:, 1:].unsqueeze(2), v[:, 1:].unsqueeze(1), dim=3, eps=EPS)
    return cls, tok


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("kind", ["special", "mean100"])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("B,N,D", SHAPES)
def test_token_cosine_against_the_restatement(B, N, D, dtype, kind, pad):
    x = tokens_of(kind, B, N, D, dtype, 13 * N + D)
    rcls, rtok, scls, stok = R.cosine_ref(x.float().numpy(), EPS)
    f32 = torch_f32(x)
    name = f"({B},{N},{D}) {dtype} {kind} pad={pad}"
    c = measure_c(f"token_cosine {name}", dtype, [(f32[0], rcls, scls), (f32[1], rtok, stok)])
    cls, tok = run(x, pad)
    assert_close(f"{name} cls_sim", cls, rcls, scls, c, 0.0)
    assert_close(f"{name} tok_sim", tok, rtok, stok, c, 0.0)
    if kind == "special" and N > 5:
        t = tok.cpu()
        assert (t[0, 1] == 0).all() and (t[0, :, 1] == 0).all(), "a zero row gives 0, not NaN"
        assert abs(t[0, 2, 3].item() - 1.0) <= c * 2.0 ** -23  # two identical rows
    # each output alone: the same bits
    only_cls, _ = run(x, pad, want_tok=False)
    _, only_tok = run(x, pad, want_cls=False)
    assert_bits_equal(f"{name} cls_sim alone", only_cls.contiguous(), cls.contiguous())
    assert_bits_equal(f"{name} tok_sim alone", only_tok.contiguous(), tok.contiguous())
    again = run(x, pad)
    assert_bits_equal(f"{name} cls_sim repeat", again[0].contiguous(), cls.contiguous())
    assert_bits_equal(f"{name} tok_sim repeat", again[1].contiguous(), tok.contiguous())
    # the matrix of rows 1..N-1 against each other is symmetric up to the bound, its diagonal is 1 or 0
    d = torch.diagonal(tok, dim1=1, dim2=2).cpu().double()
    want = torch.from_numpy(np.diagonal(rtok, axis1=1, axis2=2).copy())
    assert ((d - want).abs() <= c * 2.0 ** -23).all()


def test_token_cosine_eps_is_an_argument():
    x = tokens_of("special", 1, 10, 192, "fp32", 3)
    for eps in (1e-8, 1e-3, 0.0):
        rcls, rtok, scls, stok = R.cosine_ref(x.float().numpy(), eps if eps else 1e-150)
        got = run(x, 0, eps=eps)
        if eps == 0.0:  # the zero row divides by 0: NaN there, everything else as with a tiny eps
            assert torch.isnan(got[1][0, 1]).all()
            keep = torch.ones(9, dtype=torch.bool)
            keep[1] = False
            assert_close("eps=0 tok_sim", got[1][0][keep][:, keep], rtok[0][keep.numpy()][:, keep.numpy()],
                         stok[0][keep.numpy()][:, keep.numpy()], 16.0, 0.0)
        else:
            assert_close(f"eps={eps} cls_sim", got[0], rcls, scls, 16.0, 0.0)
            assert_close(f"eps={eps} tok_sim", got[1], rtok, stok, 16.0, 0.0)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_token_cosine_rejections_leave_the_outputs_untouched(dtype):
    B, N, D = 2, 10, 64
    dt = tdt(dtype)
    code = 0 if dtype == "bf16" else 1
    x = tokens_of("special", B, N, D, dtype, 1)
    xv, _ = nanview(B * N, D, 8, dt, src=x.reshape(B * N, D))
    cls, clsp = nanview(B, N - 1, 3, torch.float32, align=4)
    tok, tokp = nanview(B * (N - 1), N - 1, 3, torch.float32, align=4)
    L, st = lib(), ops().stream()
    ld, lc, lt = xv.stride(0), cls.stride(0), tok.stride(0)
    cases = [
        ("N must be >= 2", (code, ptr(xv), ld, B, 1, D, EPS, ptr(cls), lc, ptr(tok), lt)),
        ("D must be", (code, ptr(xv), ld, B, N, D - (16 if dtype == "bf16" else 2), EPS, ptr(cls), lc, ptr(tok), lt)),
        ("D must be", (code, ptr(xv), ld, B, N, 0, EPS, ptr(cls), lc, ptr(tok), lt)),
        ("16-byte aligned", (code, None, ld, B, N, D, EPS, ptr(cls), lc, ptr(tok), lt)),
        ("16-byte aligned", (code, ptr(xv) + xv.element_size(), ld, B, N, D, EPS, ptr(cls), lc, ptr(tok), lt)),
        ("16-byte aligned", (code, ptr(xv), D - 8, B, N, D, EPS, ptr(cls), lc, ptr(tok), lt)),
        ("16-byte aligned", (code, ptr(xv), ld + 1, B, N, D, EPS, ptr(cls), lc, ptr(tok), lt)),
        ("no output requested", (code, ptr(xv), ld, B, N, D, EPS, None, lc, None, lt)),
        ("row stride must be >= N - 1", (code, ptr(xv), ld, B, N, D, EPS, ptr(cls), N - 2, ptr(tok), lt)),
        ("row stride must be >= N - 1", (code, ptr(xv), ld, B, N, D, EPS, ptr(cls), lc, ptr(tok), N - 2)),
        ("eps must be >= 0", (code, ptr(xv), ld, B, N, D, -1.0, ptr(cls), lc, ptr(tok), lt)),
        ("unknown dtype", (7, ptr(xv), ld, B, N, D, EPS, ptr(cls), lc, ptr(tok), lt)),
    ]
    for msg, args in cases:
        L.fer_set_persistent_mode(0)  # a success does not clear the message
        assert L.fer_token_cosine(*args, st) != 0, msg
        assert last_error().startswith("token_cosine:") and msg in last_error(), (msg, last_error())
    torch.cuda.synchronize()
    all_nan("cls_sim", clsp)
    all_nan("tok_sim", tokp)
    with pytest.raises(ValueError):
        ops().token_cosine(x.to(DEV)[:, :1])
    with pytest.raises(ValueError):
        ops().token_cosine(x.to(DEV), want_cls=False, want_tok=False)


def test_wrapper_matches_the_abi_call():
    x = tokens_of("special", 3, 10, 192, "bf16", 2)
    cls, tok = run(x, 0)
    wc, wt = ops().token_cosine(x.to(DEV), EPS)
    assert wc.shape == (3, 9) and wt.shape == (3, 9, 9)
    assert_bits_equal("cls_sim", wc, cls.contiguous())
    assert_bits_equal("tok_sim", wt, tok.contiguous())
    wc2, none = ops().token_cosine(x.to(DEV), EPS, want_tok=False)
    assert none is None
    assert_bits_equal("cls_sim alone", wc2, wc)
