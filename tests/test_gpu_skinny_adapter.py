"""Element-wise checks of fer_skinny_adapter (csrc/skinny_adapter.hip) against the float64 reference of
tests/skinny_adapter_ref.py: every alpha at every shape, tight and padded row strides, canaries, alpha = 0,
row independence, determinism, the ops wrapper and the rejected calls.

Every comparison is tests/elemwise.py's |got - ref| <= 2^-8 * |ref| + c * 2^-23 * scale + extra with the scale
and the derived `extra` of skinny_adapter_ref's module doc, c measured by elemwise.measure_c on the float32 torch
composition against the same reference. No element is left out."""
import functools

import pytest
import torch

import skinny_adapter_ref as R
from abi_harness import last_error
from abi_harness import lib as L
from abi_harness import ops
from elemwise import BF_ROUND, assert_bits_equal, assert_close, measure_c
from test_gpu_skinny_linear import Out, dev_in, vec  # the canaried operands of the skinny-linear test

pytestmark = pytest.mark.gpu

DEV = "cuda"


def alpha_dev(alpha):
    return torch.tensor([alpha], dtype=torch.float32, device=DEV)


def raw(X, W1, b1, W2, b2, alpha, out, ldc, M, D, A):
    """fer_skinny_adapter on device operands with their own strides; returns the return code."""
    return L().fer_skinny_adapter(X.data_ptr(), X.stride(0), W1.data_ptr(), W1.stride(0), b1.data_ptr(),
                                  W2.data_ptr(), W2.stride(0), b2.data_ptr(), alpha.data_ptr(), out.data_ptr(), ldc,
                                  M, D, A, ops().stream())


@functools.lru_cache(maxsize=None)
def reference(M, D, A, alpha):
    """(operands, ref, scale, extra, c) of one shape and alpha, on the CPU; shared by the tight and the padded run."""
    t = R.operands(M, D, A)
    ref, scale, sacc, carry = R.adapter_ref(t.X, t.W1, t.b1, t.W2, t.b2, alpha)
    c = measure_c("skinny_adapter", f"M={M} D={D} R={A} alpha={alpha}",
                  [(R.adapter_f32(t.X, t.W1, t.b1, t.W2, t.b2, alpha), ref, scale)])
    return t, ref, scale, R.adapter_extra(alpha, sacc, carry, c), c


def launch(t, alpha, pads, M=None):
    """One call on device copies of the operands with (ldx, ldw1, ldw2, ldc) padded by `pads`; returns the Out."""
    M = t.M if M is None else M
    px, p1, p2, pc = pads
    X, W1, W2 = dev_in(t.X[:M], px), dev_in(t.W1, p1), dev_in(t.W2, p2)
    o = Out(M, t.D, pc)
    rc = raw(X, W1, vec(t.b1), W2, vec(t.b2), alpha_dev(alpha), o.view, o.ld, M, t.D, t.R)
    assert rc == 0, last_error()
    torch.cuda.synchronize()
    return o


TIGHT, PADDED = (0, 0, 0, 0), (8, 16, 8, 24)


@pytest.mark.parametrize("pads", [TIGHT, PADDED], ids=["tight", "padded"])
@pytest.mark.parametrize("D,A", R.DRS)
@pytest.mark.parametrize("M", R.MS)
def test_every_alpha(M, D, A, pads):
    worst = 0.0
    for alpha in R.ALPHAS:
        t, ref, scale, extra, c = reference(M, D, A, alpha)
        name = f"skinny_adapter M={M} D={D} R={A} alpha={alpha} pads={pads}"
        o = launch(t, alpha, pads)
        o.check_guards(name)
        got = o.view.float().cpu()
        assert not torch.isnan(got).any(), name
        worst = max(worst, assert_close(name, got, ref, scale, c, BF_ROUND, extra))
        if alpha == 0.0:
            assert_bits_equal(f"{name}: alpha = 0 returns X", o.view.cpu(), t.X.bfloat16())
    print(f"skinny_adapter M={M} D={D} R={A} pads={pads}: worst err / bound {worst:.3f}")


@pytest.mark.parametrize("D,A", [(768, 64), (192, 32), (64, 128)])
def test_rows_do_not_depend_on_m(D, A):
    """Rows 0-18 of an M = 57 call (4 row tiles) equal the M = 19 call (2 row tiles) bit for bit, and row 0 the
    M = 1 call: an element's summation order depends on D and R alone."""
    t57 = R.operands(57, D, A, seed=3)
    a = launch(t57, 0.37, PADDED).view[:19].clone()
    b = launch(t57, 0.37, PADDED, M=19).view
    assert_bits_equal(f"rows 0-18 of M=57 against M=19, D={D} R={A}", a, b)
    c = launch(t57, 0.37, TIGHT, M=1).view
    assert_bits_equal(f"row 0 of M=57 against M=1, D={D} R={A}", a[:1], c)


def test_two_identical_calls_are_bit_equal():
    t = R.operands(37, 768, 64, seed=5)
    assert_bits_equal("two identical calls", launch(t, -1.5, PADDED).view, launch(t, -1.5, PADDED).view)


def test_ops_wrapper_matches_the_raw_call():
    t = R.operands(19, 192, 32, seed=7)
    want = launch(t, 0.37, TIGHT).view
    bf = lambda v: v.to(DEV).bfloat16()
    got = ops().skinny_adapter(bf(t.X), bf(t.W1), vec(t.b1), bf(t.W2), vec(t.b2), alpha_dev(0.37))
    assert_bits_equal("ops.skinny_adapter against the raw call", got, want)


REJECTED = {
    "M = 65": (dict(M=65), "1 <= M <= 64"),
    "D = 24": (dict(D=24), "multiple of 16"),
    "R = 8": (dict(R=8), "adapter width"),
    "R = 144": (dict(R=144), "adapter width"),
    "out == X": (dict(out_is_x=0), "overlap"),
    "out overlaps X's tail": (dict(out_is_x=18), "overlap"),
    "null alpha": (dict(null_alpha=True), "alpha"),
    "misaligned X": (dict(shift_x=2), "aligned"),
}


@pytest.mark.parametrize("what", list(REJECTED))
def test_rejected_calls_leave_out_untouched(what):
    """Each violation of the contract returns a negative code with fer_last_error naming it, before any launch:
    the canaried output (and X, where out was pointed into it) keeps its bits."""
    r, word = REJECTED[what]
    M, D, A, LD = 19, 192, 32, 200
    X = torch.ones(72, LD, dtype=torch.bfloat16, device=DEV)
    X_before = X.clone()
    W1 = torch.zeros(160, LD, dtype=torch.bfloat16, device=DEV)
    W2 = torch.zeros(LD, 160, dtype=torch.bfloat16, device=DEV)
    b1, b2 = torch.zeros(160, device=DEV), torch.zeros(LD, device=DEV)
    alpha = alpha_dev(0.37)
    o = Out(64, D + 8, 8)
    out_ptr, ldc = o.parent.data_ptr(), o.ld
    if "out_is_x" in r:  # out inside X: row out_is_x of X onwards (row 18 is the last row an M = 19 call reads)
        out_ptr, ldc = X.data_ptr() + 2 * LD * r["out_is_x"], LD
    L().fer_set_persistent_mode(0)
    rc = L().fer_skinny_adapter(X.data_ptr() + 2 * r.get("shift_x", 0), LD, W1.data_ptr(), LD, b1.data_ptr(),
                                W2.data_ptr(), 160, b2.data_ptr(), None if r.get("null_alpha") else alpha.data_ptr(),
                                out_ptr, ldc, r.get("M", M), r.get("D", D), r.get("R", A), ops().stream())
    torch.cuda.synchronize()
    assert rc < 0, what
    assert last_error().startswith("skinny_adapter:") and word in last_error(), (what, last_error())
    o.untouched(what)
    assert_bits_equal(f"{what}: X", X, X_before)
