"""Element-wise checks of fer_skinny_linear (csrc/skinny.hip) against the float64 reference of
tests/skinny_ref.py: every flag combination at every shape, tight and padded row strides, canaries,
row independence, determinism and the rejected calls.

Every comparison is tests/elemwise.py's
    |got - ref| <= 2^-8 * |ref| + c * 2^-23 * scale + extra
with scale = sum_k |A'[m,k] W[n,k]| + |bias| + |R'|, c measured by elemwise.measure_c on the float32 torch
composition (skinny_ref.skinny_f32) against the same reference, and, with LN-on-load, extra = 2^-8 * sum_k
|A'[m,k] W[n,k]|: the kernel rounds A' to bf16 as the matrix operand (at most 2^-9 relative per element) and the
float64 reference does not; derived, not measured. ReLU outputs whose pre-activation lies within its own bound
of zero are left out (skinny_ref.relu_live), at most 0.1 % of a case, by assertion."""
import functools

import pytest
import torch

import skinny_ref as R
from abi_harness import last_error
from abi_harness import lib as L
from abi_harness import ops
from elemwise import BF_ROUND, assert_bits_equal, assert_close, measure_c

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 8
ACT = {"none": 0, "gelu": 1, "relu": 2}
NAN = float("nan")


class Out:
    """out [M][N] as the top-left view of a NaN-filled [M + 8][N + pad] parent."""

    def __init__(self, M, N, pad):
        self.parent = torch.full((M + GUARD, N + pad), NAN, dtype=torch.bfloat16, device=DEV)
        self.view = self.parent[:M, :N]
        self.before = self.parent.clone()
        self.ld = self.parent.stride(0)

    def check_guards(self, name):
        M, N = self.view.shape
        after = self.parent.clone()
        after[:M, :N] = self.before[:M, :N]
        assert_bits_equal(f"{name}: the kernel wrote outside its [{M}][{N}] output", after, self.before)

    def untouched(self, name):
        assert_bits_equal(f"{name}: a rejected call wrote to its output", self.parent, self.before)


def dev_in(src, pad):
    """A bf16 device operand as the column-0 view of a parent whose `pad` padding columns are NaN."""
    rows, cols = src.shape
    parent = torch.full((rows, cols + pad), NAN, dtype=torch.bfloat16, device=DEV)
    v = parent[:, :cols]
    v.copy_(src)
    assert v.data_ptr() % 16 == 0
    return v


def vec(t):
    return None if t is None else t.to(DEV).contiguous()


def p(t):
    return None if t is None else t.data_ptr()


def raw(A, W, out, ldc, M, N, K, bias=None, act="none", ln_a=None, res=None, ln_res=None, lda=None, ldw=None, ldr=None,
        ptr_A=None, ptr_out=None):
    """fer_skinny_linear with every argument given; returns the return code."""
    ga, ba, ea = ln_a if ln_a is not None else (None, None, 0.0)
    gr, br, er = ln_res if ln_res is not None else (None, None, 0.0)
    return L().fer_skinny_linear(ptr_A if ptr_A is not None else A.data_ptr(), A.stride(0) if lda is None else lda,
                                 W.data_ptr(), W.stride(0) if ldw is None else ldw, p(bias), ACT[act], p(ga), p(ba),
                                 ea, p(res), (N if res is None else res.stride(0)) if ldr is None else ldr, p(gr),
                                 p(br), er, ptr_out if ptr_out is not None else out.data_ptr(), ldc, M, N, K,
                                 ops().stream())


@functools.lru_cache(maxsize=None)
def reference(M, K, N, fi):
    """(operands, kwargs, ref, scale, extra, live mask or None, c) of one shape and flag combination, on the CPU;
    computed once and shared by the tight and the padded run."""
    f = R.FLAGS[fi]
    t = R.case(M, K, N, f)
    kw = R.call_args(t, f)
    ref, scale, pre, sacc = R.skinny_ref(t.A, t.W, parts=True, **kw)
    c = measure_c("skinny_linear", f"{R.flag_id(f)} M={M} K={K} N={N}", [(R.skinny_f32(t.A, t.W, **kw), ref, scale)])
    extra = BF_ROUND * sacc if f.ln_a else None
    live = R.relu_live(pre, sacc, kw["bias"], c, f.ln_a) if f.act == "relu" else None
    return t, kw, ref, scale, extra, live, c


def launch(t, kw, pads, M=None):
    """One call on device copies of the operands with (lda, ldr, ldc) padded by `pads`; returns the Out."""
    M = t.M if M is None else M
    pa, pr, pc = pads
    A, W = dev_in(t.A[:M], pa), dev_in(t.W, 0)
    res = dev_in(kw["res"][:M], pr) if kw["res"] is not None else None
    o = Out(M, t.N, pc)
    dv = lambda ln: None if ln is None else (vec(ln[0]), vec(ln[1]), ln[2])
    rc = raw(A, W, o.view, o.ld, M, t.N, t.K, bias=vec(kw["bias"]), act=kw["act"], ln_a=dv(kw["ln_a"]), res=res,
             ln_res=dv(kw["ln_res"]))
    assert rc == 0, last_error()
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("pads", [(0, 0, 0), (8, 16, 24)], ids=["tight", "padded"])
@pytest.mark.parametrize("K,N", R.KNS)
@pytest.mark.parametrize("M", R.MS)
def test_every_flag_combination(M, K, N, pads):
    worst = 0.0
    for fi, f in enumerate(R.FLAGS):
        t, kw, ref, scale, extra, live, c = reference(M, K, N, fi)
        name = f"skinny_linear {R.flag_id(f)} M={M} K={K} N={N} pads={pads}"
        o = launch(t, kw, pads)
        o.check_guards(name)
        got = o.view.float().cpu()
        assert not torch.isnan(got).any(), name
        if live is None:
            worst = max(worst, assert_close(name, got, ref, scale, c, BF_ROUND, extra))
        else:
            assert (~live).sum().item() <= 1e-3 * live.numel(), name
            worst = max(worst, assert_close(name, got[live], ref[live], scale[live], c, BF_ROUND,
                                            None if extra is None else extra[live]))
    print(f"skinny_linear M={M} K={K} N={N} pads={pads}: worst err / bound {worst:.3f}")


FULL = next(i for i, f in enumerate(R.FLAGS) if f.ln_a and f.bias and f.act == "gelu" and f.res == "ln")


@pytest.mark.parametrize("K,N", [(512, 1536), (2048, 512), (64, 8)])
def test_rows_do_not_depend_on_m(K, N):
    """Rows 0-18 of an M = 57 call (4 row tiles, 256-column panel chunks) equal the M = 19 call (2 row tiles,
    512-column chunks) bit for bit: an element's summation order depends on K alone."""
    t57 = R.operands(57, K, N, seed=3)
    kw = R.call_args(t57, R.FLAGS[FULL])
    a = launch(t57, kw, (8, 16, 24)).view[:19].clone()
    b = launch(t57, kw, (8, 16, 24), M=19).view
    assert_bits_equal(f"rows 0-18 of M=57 against M=19, K={K} N={N}", a, b)
    c = launch(t57, kw, (0, 0, 0), M=1).view
    assert_bits_equal(f"row 0 of M=57 against M=1, K={K} N={N}", a[:1], c)


def test_two_identical_calls_are_bit_equal():
    t = R.operands(33, 2048, 512, seed=5)
    kw = R.call_args(t, R.FLAGS[FULL])
    assert_bits_equal("two identical calls", launch(t, kw, (8, 16, 24)).view, launch(t, kw, (8, 16, 24)).view)


def test_ops_wrapper_matches_the_raw_call():
    t = R.operands(19, 512, 512, seed=7)
    f = R.FLAGS[FULL]
    kw = R.call_args(t, f)
    want = launch(t, kw, (0, 0, 0)).view
    dv = lambda ln: (vec(ln[0]), vec(ln[1]), ln[2])
    got = ops().skinny_linear(t.A.to(DEV).bfloat16(), t.W.to(DEV).bfloat16(), vec(t.bias), act="gelu",
                              ln_a=dv(kw["ln_a"]), res=t.res.to(DEV).bfloat16(), ln_res=dv(kw["ln_res"]))
    assert_bits_equal("ops.skinny_linear against the raw call", got, want)


REJECTED = {
    "M = 0": dict(M=0),
    "M = 65": dict(M=65),
    "K % 8 != 0": dict(K=508),
    "N % 8 != 0": dict(N=516),
    "misaligned A": dict(shift_A=2),
    "misaligned out": dict(shift_out=2),
    "lda % 8 != 0": dict(lda=516),
    "ldc below N": dict(ldc=504),
    "gamma without beta": dict(half_ln=True),
    "unknown act": dict(act_code=3),
}


@pytest.mark.parametrize("what", list(REJECTED))
def test_rejected_calls_leave_out_untouched(what):
    """Each violation of the contract returns a negative code with fer_last_error set, before any launch: the
    canaried output keeps its bits."""
    r = REJECTED[what]
    M, K, N = 19, 512, 512
    A = torch.zeros(72, 520, dtype=torch.bfloat16, device=DEV)
    W = torch.zeros(N + 8, 520, dtype=torch.bfloat16, device=DEV)
    gamma = torch.ones(K, device=DEV)
    o = Out(64, N + 8, 8)
    L().fer_set_persistent_mode(0)
    a = (None, 520, W.data_ptr(), 520, None, r.get("act_code", 0), gamma.data_ptr() if r.get("half_ln") else None, None,
         1e-5, None, N, None, None, 0.0, None, r.get("ldc", o.ld), r.get("M", M), r.get("N", N), r.get("K", K),
         ops().stream())
    a = list(a)
    a[0] = A.data_ptr() + r.get("shift_A", 0)
    a[1] = r.get("lda", 520)
    a[14] = o.parent.data_ptr() + r.get("shift_out", 0)
    rc = L().fer_skinny_linear(*a)
    torch.cuda.synchronize()
    assert rc < 0, what
    assert last_error().startswith("skinny_linear:"), (what, last_error())
    o.untouched(what)
