"""Element-wise checks of the GEMM family (csrc/gemm.hip): fer_gemm bf16 in its four tile configurations,
the fp32 kernel, split-K and fer_wgrad_group, against float64 torch, on every dispatch branch.

Every comparison is per element:
    |got - ref| <= out_round * |ref| + c * 2^-23 * scale_i + act_abs_i
  * ref is float64 torch on the CPU (on the GPU for the one large case), computed from the exact values
    the kernel was handed (bf16 operands are rounded to bf16 first and then widened; alpha, drop_scale and
    *post_scale are the fp32 values the ABI carries), in the header's epilogue order: alpha, bias, pre, act,
    dropout, post_scale, aux, res, accumulate. Keep masks come from tests/dropmask.py.
  * out_round is 2^-8 for a bf16 destination and 0 for an fp32 one.
  * scale_i is the magnitude fp32 arithmetic handled for the element, carried through the epilogue:
    |alpha| (|A| |B|^T)_mn + |bias_n|; times the activation's Lipschitz constant (ReLU 1, GELU 1.13); times
    drop_scale where kept (0, and the output exactly 0, where dropped); times |*post_scale|; times
    |act'(aux)| or |aux|; plus |res|; plus |c_old| when accumulating. A gated `pre` has the scale of h times
    max |act''| (GELU: 2 phi(0) = 0.798; ReLU: 0, the gate is exact away from h = 0).
  * c is measured in each test, never on the kernel: the same matmul and epilogue in float32 torch on the
    CPU, its worst error in scale_i units, times 4, floor 16; printed as `c-measure gemm <case> <dtype>
    <value>`.
  * act_abs_i is the absolute error of the GELU / GELU' approximations of csrc/common.h (9e-7 and 1e-6,
    derived in DESIGN.md section 2.2) times the factors applied after them.
Outputs (c, pre, colsum, dw) are views into NaN-filled parents with padding columns in every row (padded
runs: 8 for c, and another multiple of 8 for each other operand, so that no two row strides of a call are
equal) and 8 guard rows after the last row; inputs are views into parents whose padding columns are NaN.
After a launch the padding and guard rows must be the same bits as before, and no NaN may be in a result.
Every case runs once with tight and once with padded row strides. A failure names the worst element."""
import ctypes
import functools
import math
import types

import pytest
import torch

from abi_harness import f32v, last_error, nanview, ops, out_round, tdt
from abi_harness import lib as L
from dropmask import keep_mask, keep_mask_torch
from elemwise import U, assert_bits_equal, assert_close, measure_c

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAD, GUARD = 8, 8
GELU_LIP = 1.13  # max |gelu'| = 1.129
GELU_D2_MAX = 0.7979  # max |gelu''| = 2 phi(0)
GELU_ABS = 9e-7  # csrc/common.h: stated for gelu_erf_fast2; the A-S 7.1.26 forms stay below it
GELU_GRAD_ABS = 1e-6  # gelu_erf_grad / gelu_and_grad*: DESIGN.md 2.2
ACT = {"none": 0, "gelu": 1, "relu": 2, "mul": 3}
PRE_GATE = 16
LAYOUTS = [(1, 1), (1, 0), (0, 0), (0, 1)]
CFGS = [3, 5, 8, 11]


class forced_config:
    """fer_gemm_set_config(cfg) for the block (it must return 0: the configuration exists), -1 after it."""

    def __init__(self, cfg):
        self.cfg = cfg

    def __enter__(self):
        assert L().fer_gemm_set_config(self.cfg) == 0, last_error()

    def __exit__(self, *exc):
        assert L().fer_gemm_set_config(-1) == 0


# ---------------------------------------------------------------------- guarded tensors
class Out:
    """An output [rows][cols] as the top-left view of a NaN-filled [rows + GUARD][cols + pad] parent."""

    def __init__(self, rows, cols, pad, dt, init=None):
        self.parent = torch.full((rows + GUARD, cols + pad), float("nan"), dtype=dt, device=DEV)
        self.view = self.parent[:rows, :cols]
        if init is not None:
            self.view.copy_(init.to(dt))
        self.before = self.parent.clone()
        assert self.view.data_ptr() % 16 == 0

    @property
    def ld(self):
        return self.parent.stride(0)

    def check_guards(self, name):
        rows, cols = self.view.shape
        after = self.parent.clone()
        after[:rows, :cols] = self.before[:rows, :cols]
        assert_bits_equal(f"{name}: the kernel wrote outside its [{rows}][{cols}] output", after, self.before)

    def untouched(self, name):
        assert_bits_equal(f"{name}: a rejected call wrote to its output", self.parent, self.before)


def inp(src, pad, dt):
    """An input as the column-0 view of a parent whose `pad` padding columns are NaN."""
    return nanview(*src.shape, pad, dt, src, guard=0)[0]


# ---------------------------------------------------------------------- raw ABI call
def raw_gemm(*, dtype, A, lda, a_kc, B, ldb, b_kc, M, N, K, ws=None, ws_bytes=None, c, ldc, c_f32=0, accumulate=0,
             alpha=1.0, bias=None, act=0, pre=None, ldp=None, res=None, ldr=None, drop_thresh=0, drop_scale=1.0, seed=0,
             drop_ld=None, aux=None, ldx=None, aux_act=0, post_scale=None, colsum=None, colsum_accumulate=0):
    """fer_gemm with every field given (pointers as tensors or integers); returns the return code."""
    from fervit._lib import Epilogue, GemmDesc

    def p(t):
        return t.data_ptr() if isinstance(t, torch.Tensor) else t

    d, e = GemmDesc(), Epilogue()
    d.dtype, d.A, d.lda, d.a_kc, d.B, d.ldb, d.b_kc = dtype, p(A), lda, a_kc, p(B), ldb, b_kc
    d.M, d.N, d.K = M, N, K
    d.ws, d.ws_bytes = p(ws), (0 if ws is None else (ws.numel() * 4 if ws_bytes is None else ws_bytes))
    e.c, e.ldc, e.c_f32, e.accumulate, e.alpha = p(c), ldc, c_f32, accumulate, alpha
    e.bias, e.act = p(bias), act
    e.pre, e.ldp = p(pre), N if ldp is None else ldp
    e.res, e.ldr = p(res), N if ldr is None else ldr
    e.drop_thresh, e.drop_scale, e.seed = drop_thresh, drop_scale, seed & 0xFFFFFFFFFFFFFFFF
    e.drop_ld = N if drop_ld is None else drop_ld
    e.aux, e.ldx, e.aux_act = p(aux), N if ldx is None else ldx, aux_act
    e.post_scale = p(post_scale)
    e.colsum, e.colsum_accumulate = p(colsum), colsum_accumulate
    return L().fer_gemm(ctypes.byref(d), ctypes.byref(e), ops().stream())


# ---------------------------------------------------------------------- the reference
def gelu_parts(x):
    """GELU and its derivative from erf and exp, in the precision of x."""
    cdf = 0.5 * (1.0 + torch.erf(x * 0.7071067811865476))
    pdf = torch.exp(-0.5 * x * x) * 0.3989422804014327
    return x * cdf, cdf + x * pdf


def act_parts(name, x):
    if name == "gelu":
        return gelu_parts(x)
    assert name == "relu"
    return torch.relu(x), (x > 0).to(x.dtype)


SPEC_DEFAULTS = dict(dtype="bf16", a_kc=1, b_kc=1, bias=False, act="none", pre=None, res=False, p=0.0, drop_extra=0,
                     aux=None, alpha=1.0, accumulate=False, c_f32=False, post_scale=None, colsum=None, seed=0x1234_5678_9ABC)


def spec(M, N, K, **kw):
    """One fer_gemm call. pre: None / "plain" / "gate"; aux: None / "gelu" / "relu" / "mul"; colsum: None /
    "plain" / "acc"; drop_extra: drop_ld - N."""
    assert not set(kw) - set(SPEC_DEFAULTS), kw
    sp = types.SimpleNamespace(M=M, N=N, K=K, **dict(SPEC_DEFAULTS, **kw))
    if sp.dtype == "fp32":
        sp.c_f32 = True  # the fp32 path stores fp32 either way; the host wrapper sets the flag from the dtype
    return sp


def epilogue(acc, sacc, t, sp, dtype):
    """The header's epilogue in `dtype` on acc = A B^T. t: the operands' exact values as float64. Returns the
    outputs with their float64 scales (s_*) and absolute terms (a_*)."""
    def f(x):
        return x.to(dtype)

    zero = torch.zeros((), dtype=dtype, device=acc.device)
    z64 = torch.zeros((), dtype=torch.float64, device=acc.device)
    alpha = f32v(sp.alpha)
    v, s = f(acc) * alpha, sacc * abs(alpha)
    if sp.bias:
        v, s = v + f(t.bias), s + t.bias.abs()
    ab = torch.zeros_like(s)
    r = types.SimpleNamespace(h=v, s_h=s, pre=None, colsum=None)
    if sp.pre == "plain":
        r.pre, r.s_pre, r.a_pre = v, s, ab
    g = None
    if sp.act != "none":
        v, g = act_parts(sp.act, v)
        if sp.act == "gelu":
            s_g, a_g = s * GELU_D2_MAX, torch.full_like(s, GELU_GRAD_ABS)
            s, ab = s * GELU_LIP, ab + GELU_ABS
        else:
            s_g, a_g = torch.zeros_like(s), torch.zeros_like(s)
    ds = f32v(t.drop_scale)
    r.kept, r.s_kept, r.a_kept = v * ds, s * ds, ab * ds  # the output of the dropout had it kept everything
    if sp.p > 0:
        v, s, ab = torch.where(t.keep, v * ds, zero), torch.where(t.keep, s * ds, z64), torch.where(t.keep, ab * ds, z64)
        if g is not None:
            g, s_g, a_g = (torch.where(t.keep, g * ds, zero), torch.where(t.keep, s_g * ds, z64),
                           torch.where(t.keep, a_g * ds, z64))
    if sp.pre == "gate":
        r.pre, r.s_pre, r.a_pre = g, s_g, a_g
    if sp.post_scale is not None:
        ps = f32v(sp.post_scale)
        v, s, ab = v * ps, s * abs(ps), ab * abs(ps)
        r.kept, r.s_kept, r.a_kept = r.kept * ps, r.s_kept * abs(ps), r.a_kept * abs(ps)
    if sp.aux is not None:
        x = f(t.aux)
        if sp.aux == "mul":
            fac, fa = x, 0.0
        elif sp.aux == "gelu":
            fac, fa = gelu_parts(x)[1], GELU_GRAD_ABS
        else:
            fac, fa = (x > 0).to(dtype), 0.0
        ab = ab * fac.abs() + v.abs().double() * fa
        v, s = v * fac, s * fac.abs()
    if sp.res:
        v, s = v + f(t.res), s + t.res.abs()
    if sp.accumulate:
        v, s = v + f(t.c_old), s + t.c_old.abs()
    r.c, r.s_c, r.a_c = v, s, ab
    if sp.colsum is not None:
        r.colsum, r.s_colsum, r.a_colsum = v.sum(0), v.abs().double().sum(0), ab.sum(0)
        if sp.colsum == "acc":
            r.colsum, r.s_colsum = r.colsum + f(t.cs_old), r.s_colsum + t.cs_old.abs()
    return r


@functools.lru_cache(maxsize=None)
def operands(M, N, K, dtype, dev="cpu"):
    """Random operands of one shape, rounded to the dtype and widened to float64, with the float64 product,
    its magnitude sum |A| |B|^T and the float32 product (on the CPU). Shared by every case of the shape."""
    dt = tdt(dtype)
    g = torch.Generator(device=dev).manual_seed(M * 1000003 + N * 1009 + K)

    def rn(*shape, scale=1.0, to=dt):
        return (torch.randn(*shape, generator=g, device=dev) * scale).to(to).double()

    t = types.SimpleNamespace(A=rn(M, K), B=rn(N, K, scale=1 / math.sqrt(K)), bias=rn(N, to=torch.float32),
                              res=rn(M, N), aux=rn(M, N), c_old_dt=rn(M, N), c_old_f32=rn(M, N, to=torch.float32),
                              cs_old=rn(N, scale=3.0, to=torch.float32))
    t.acc = t.A @ t.B.t()
    t.sacc = t.A.abs() @ t.B.abs().t()
    t.acc32 = t.A.float().cpu() @ t.B.float().cpu().t()
    return t


def eff(scale, a, c):
    """The absolute term of the bound folded into the scale: c U (s + a / (c U)) = c U s + a."""
    return scale + a / (c * U)


def run_case(tag, sp, *, via="raw", dev="cpu", strides=(False, True), repeat=False):
    """One fer_gemm call against the reference, with tight and with padded strides; every output checked per
    element, keep decisions and guards included. via: "raw" (the ABI, workspace only for column sums),
    "small_ws" (a workspace of 4 M N bytes: too small for two splits), "ops_split" / "ops_nosplit" (ops.gemm with
    split_ws on / off). repeat: a second call must give the same bits. Returns the c of the first run."""
    o = ops()
    M, N, K, dtype = sp.M, sp.N, sp.K, sp.dtype
    dt = tdt(dtype)
    odt = torch.float32 if sp.c_f32 else dt
    op = operands(M, N, K, dtype, dev)
    thr, dscale = o.drop_args(sp.p)
    drop_ld = N + sp.drop_extra
    t = types.SimpleNamespace(bias=op.bias, res=op.res if sp.res else None, aux=op.aux if sp.aux else None,
                              cs_old=op.cs_old, drop_scale=dscale, keep=None,
                              c_old=(op.c_old_f32 if sp.c_f32 else op.c_old_dt) if sp.accumulate else None)
    if sp.p > 0:
        t.keep = (keep_mask(sp.seed, (M, drop_ld), sp.p) if dev == "cpu" else
                  keep_mask_torch(sp.seed, (M, drop_ld), sp.p, device=dev))[:, :N]
    r = epilogue(op.acc, op.sacc, t, sp, torch.float64)
    if dev != "cpu":  # the large case: float64 on the GPU, compared on the CPU
        for k, v in list(vars(r).items()):
            if isinstance(v, torch.Tensor):
                setattr(r, k, v.cpu())
        t = types.SimpleNamespace(**{k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in vars(t).items()})
    # the same in float32 torch on the CPU (its scales are not used)
    q = epilogue(op.acc32, torch.zeros(M, N, dtype=torch.float64), t, sp, torch.float32)
    cs = {}
    if sp.pre == "gate" and sp.act == "relu":
        # the gate (h > 0) is discontinuous at 0: leave out |h| at or below h's own bound (in the gate only)
        c_h = measure_c(f"gemm {tag}.h", dtype, [(q.h, r.h, r.s_h)])
        out = r.h.abs() <= c_h * U * r.s_h
        assert out.double().mean().item() <= 1e-3, f"{tag}: {out.double().mean().item():.2e} of h within its bound of 0"
        q.pre = torch.where(out, r.pre.float(), q.pre)
    else:
        out = None
    for k in ("c", "pre", "colsum"):
        if getattr(r, k) is not None:
            cs[k] = measure_c(f"gemm {tag}.{k}", dtype, [(getattr(q, k), getattr(r, k), getattr(r, "s_" + k))])

    for padded in strides:
        name = f"{tag} {dtype} M={M} N={N} K={K} a_kc={sp.a_kc} b_kc={sp.b_kc} {'padded' if padded else 'tight'}"
        # a different stride for every operand (multiples of 8 elements), so that one taken for another shows
        pad, pad_b, pad_pre, pad_res, pad_aux = (PAD, 2 * PAD, 2 * PAD, 3 * PAD, 5 * PAD) if padded else (0, 0, 0, 0, 0)

        def in_pad(cols, bf_pad):  # fp32 operands: an odd row stride
            return bf_pad if (dtype == "bf16" or not padded) else (bf_pad + 1 if cols % 2 == 0 else bf_pad + 2)

        A = op.A if sp.a_kc else op.A.t()
        B = op.B if sp.b_kc else op.B.t()
        Ad, Bd = inp(A, in_pad(A.shape[1], pad), dt), inp(B, in_pad(B.shape[1], pad_b), dt)
        resd = inp(op.res, pad_res, dt) if sp.res else None
        auxd = inp(op.aux, pad_aux, dt) if sp.aux is not None else None
        biasd = op.bias.float().to(DEV) if sp.bias else None
        psd = torch.tensor([sp.post_scale], dtype=torch.float32, device=DEV) if sp.post_scale is not None else None

        def fresh():
            c = Out(M, N, pad, odt, init=t.c_old if sp.accumulate else None)
            pre = Out(M, N, pad_pre, dt) if sp.pre else None
            col = Out(1, N, pad, torch.float32, init=op.cs_old[None] if sp.colsum == "acc" else None) if sp.colsum else None
            return c, pre, col

        def call(c, pre, col):
            if via in ("raw", "small_ws"):
                ws = None
                if sp.colsum:
                    ws = torch.empty(L().fer_gemm_colsum_ws(M, N) // 4, dtype=torch.float32, device=DEV)
                elif via == "small_ws":
                    ws = torch.empty(M * N, dtype=torch.float32, device=DEV)
                rc = raw_gemm(dtype=o.dcode(Ad), A=Ad, lda=Ad.stride(0), a_kc=sp.a_kc, B=Bd, ldb=Bd.stride(0),
                              b_kc=sp.b_kc, M=M, N=N, K=K, ws=ws, c=c.view, ldc=c.ld, c_f32=int(sp.c_f32),
                              accumulate=int(sp.accumulate), alpha=sp.alpha, bias=biasd,
                              act=ACT[sp.act] | (PRE_GATE if sp.pre == "gate" else 0),
                              pre=None if pre is None else pre.view, ldp=None if pre is None else pre.ld, res=resd,
                              ldr=None if resd is None else resd.stride(0), drop_thresh=thr, drop_scale=dscale,
                              seed=sp.seed, drop_ld=drop_ld, aux=auxd, ldx=None if auxd is None else auxd.stride(0),
                              aux_act=ACT[sp.aux or "none"], post_scale=psd, colsum=None if col is None else col.view,
                              colsum_accumulate=int(sp.colsum == "acc"))
                assert rc == 0, f"{name}: {last_error()}"
            else:
                o.gemm(Ad, Bd, c.view, a_kc=bool(sp.a_kc), b_kc=bool(sp.b_kc), M=M, N=N, K=K, lda=Ad.stride(0),
                       ldb=Bd.stride(0), ldc=c.ld, bias=biasd, act=sp.act, pre=None if pre is None else pre.view,
                       res=resd, dropout=sp.p, seed=sp.seed, drop_ld=drop_ld, aux=auxd, aux_act=sp.aux or "none",
                       alpha=sp.alpha, accumulate=sp.accumulate, post_scale=psd, split_ws=(via == "ops_split"),
                       colsum=None if col is None else col.view, colsum_accumulate=(sp.colsum == "acc"),
                       pre_gate=(sp.pre == "gate"))

        c, pre, col = fresh()
        call(c, pre, col)
        got_c = c.view.float().cpu()
        assert_close(f"{name} c", got_c, r.c, eff(r.s_c, r.a_c, cs["c"]), cs["c"], out_round(odt))
        c.check_guards(f"{name} c")
        if pre is not None:
            got_p = pre.view.float().cpu()
            if out is not None:
                got_p = torch.where(out, r.pre.float(), got_p)
            assert_close(f"{name} pre", got_p, r.pre, eff(r.s_pre, r.a_pre, cs["pre"]), cs["pre"], out_round(dt))
            pre.check_guards(f"{name} pre")
        if col is not None:
            assert_close(f"{name} colsum", col.view[0], r.colsum, eff(r.s_colsum, r.a_colsum, cs["colsum"]),
                         cs["colsum"], 0.0)
            col.check_guards(f"{name} colsum")
        if sp.p > 0 and sp.act != "relu" and sp.aux is None and not sp.res and not sp.accumulate:
            # keep decisions: exactly 0 iff the host mask drops, where the kept value is above its own bound
            bound = out_round(odt) * r.kept.abs() + cs["c"] * U * r.s_kept + r.a_kept
            live = r.kept.abs() > bound
            assert live.double().mean().item() >= 0.99, f"{name}: live set {live.double().mean().item():.4f}"
            wrong = ((got_c != 0) != t.keep) & live
            assert not wrong.any().item(), \
                f"{name}: {int(wrong.sum())} keep decisions differ from the host mask, first at {wrong.nonzero()[0].tolist()}"
        if repeat:
            c2, pre2, col2 = fresh()
            call(c2, pre2, col2)
            assert_bits_equal(f"{name} c, second call", c2.view.contiguous(), c.view.contiguous())
            if pre is not None:
                assert_bits_equal(f"{name} pre, second call", pre2.view.contiguous(), pre.view.contiguous())
            if col is not None:
                assert_bits_equal(f"{name} colsum, second call", col2.view.contiguous(), col.view.contiguous())
    return cs["c"]


# ---------------------------------------------------------------------- (a) configurations x layouts x shapes
# M, N from {8, 72, 136, 264, 520} (tiles of 128^2, 128x64, 256^2: below one tile, ragged, one and two tiles plus 8),
# K from {8, 24, 72, 136, 200, 520} (K-step 64; the ring does two K-steps of 32 per trip: one partial step, odd and
# even trip counts, tails of 8)
SHAPES_A = [(8, 8, 8), (72, 136, 24), (136, 72, 72), (264, 520, 136), (520, 264, 200), (136, 264, 520), (520, 8, 72),
            (8, 520, 200), (72, 72, 520), (264, 136, 8), (136, 136, 136), (520, 520, 24)]
# only the MN-contiguous operand needs M % 8 == 0
SHAPES_A_KC = [(1, 72, 24), (130, 136, 200), (257, 264, 72), (1, 8, 8), (257, 520, 520), (130, 8, 136)]


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: f"a_kc{l[0]}-b_kc{l[1]}")
@pytest.mark.parametrize("cfg", CFGS)
def test_gemm_config_layout_shapes(cfg, layout):
    """Each tile configuration (3: 128^2, 5: BK = 32 ring 256^2, 8: 8-phase 256^2, 11: 128x64 / 128^2) forced
    through fer_gemm_set_config, each of the four operand layouts -- a_kc = 0, b_kc = 1 included -- over the
    shape list, plain store and bias only: the main loops, their K tails and the ragged tile edges (K-contiguous
    layouts: EPI_STORE; the others: the generic epilogue)."""
    a_kc, b_kc = layout
    with forced_config(cfg):
        for M, N, K in SHAPES_A + (SHAPES_A_KC if a_kc else []):
            for bias in (False, True):
                run_case(f"a.cfg{cfg}.{'bias' if bias else 'store'}", spec(M, N, K, a_kc=a_kc, b_kc=b_kc, bias=bias))


# ---------------------------------------------------------------------- (b) epilogues per configuration
EPILOGUES = {
    # the fixed kinds of epi_kind (K-contiguous layouts)
    "store": dict(),
    "store_bias": dict(bias=True),
    "gate": dict(bias=True, act="gelu", pre="gate"),
    "gate_drop": dict(bias=True, act="gelu", pre="gate", p=0.1),
    "gater": dict(bias=True, act="relu", pre="gate"),
    "gater_drop": dict(bias=True, act="relu", pre="gate", p=0.1),
    "res2": dict(bias=True, res=True),
    "res2_drop": dict(bias=True, res=True, p=0.1),
    "mul2": dict(aux="mul"),
    "mul2_bias": dict(aux="mul", bias=True, alpha=2.0),
    "mul2_colsum": dict(aux="mul", colsum="plain"),
    "mul2_colsum_acc": dict(aux="mul", colsum="acc"),
    # the generic epilogue
    "pre_gelu_drop_res": dict(bias=True, pre="plain", act="gelu", p=0.1, res=True),
    "pre_relu_drop_res": dict(bias=True, pre="plain", act="relu", p=0.1, res=True),
    "gelu_drop": dict(bias=True, act="gelu", p=0.1),
    "drop": dict(bias=True, p=0.1),
    "aux_gelu_drop_colsum": dict(aux="gelu", p=0.1, colsum="plain"),
    "aux_relu_drop_colsum": dict(aux="relu", p=0.1, colsum="acc"),
    "post_scale_pre_res": dict(bias=True, pre="plain", post_scale=0.37, res=True),
    "alpha": dict(alpha=-0.5, bias=True),
    "accumulate_bf16": dict(bias=True, accumulate=True),
    "c_f32": dict(bias=True, c_f32=True),
    "c_f32_accumulate": dict(c_f32=True, accumulate=True),
    "c_f32_gelu": dict(bias=True, act="gelu", c_f32=True),
    "res_drop_ld8": dict(bias=True, res=True, p=0.1, drop_extra=8),
    "res_drop_ld4": dict(bias=True, res=True, p=0.1, drop_extra=4),
    "gate_drop_ld8": dict(bias=True, act="gelu", pre="gate", p=0.1, drop_extra=8),
    "gate_drop_ld4": dict(bias=True, act="gelu", pre="gate", p=0.1, drop_extra=4),
    "gater_drop_ld4": dict(bias=True, act="relu", pre="gate", p=0.1, drop_extra=4),
    "gate_colsum": dict(bias=True, act="gelu", pre="gate", p=0.1, colsum="plain"),
}
RAGGED = (264, 136, 200)  # partial in M, N and K for every tile: 256 + 8, 128 + 8, 3 x 64 + 8


@pytest.mark.parametrize("case", sorted(EPILOGUES))
@pytest.mark.parametrize("cfg", CFGS)
def test_gemm_epilogues(cfg, case):
    """Every fixed epilogue kind (EPI_STORE, EPI_GATE, EPI_GATER, EPI_RES2 / EPI_RES with and without dropout,
    EPI_MUL2 / EPI_MUL with and without fused column sums) and the generic epilogue's options, in each tile
    configuration, K-contiguous operands, M = 264, N = 136, K = 200. drop_ld = N + 4 forces the generic epilogue
    (keep4 instead of keep8a). The fused column sums add the fp32 values before they are rounded to the output
    type (csrc/gemm.hip: cs0 += v0 after the epilogue), so no 2^-9 term is added; without colsum_accumulate the
    destination starts as NaN, with it from a random vector."""
    with forced_config(cfg):
        run_case(f"b.cfg{cfg}.{case}", spec(*RAGGED, **EPILOGUES[case]))


@pytest.mark.parametrize("layout", LAYOUTS[1:], ids=lambda l: f"a_kc{l[0]}-b_kc{l[1]}")
@pytest.mark.parametrize("cfg", CFGS)
def test_gemm_generic_epilogue_other_layouts(cfg, layout):
    """The layouts with an MN-contiguous operand always take the generic epilogue: the forms the backward uses
    (dgrad with dropout + act' + column sums; the weight-gradient form c_f32 + accumulate) and a forward form."""
    a_kc, b_kc = layout
    with forced_config(cfg):
        for case in ("aux_gelu_drop_colsum", "c_f32_accumulate", "pre_gelu_drop_res", "res2_drop", "gate_drop"):
            run_case(f"b.cfg{cfg}.layout.{case}", spec(*RAGGED, a_kc=a_kc, b_kc=b_kc, **EPILOGUES[case]))


# ---------------------------------------------------------------------- (c) more 256^2 tiles than CUs
BIG = (8200, 2056, 136)  # 33 x 9 = 297 tiles, an 8-row last tile row and an 8-column last tile column


@pytest.mark.parametrize("case", ["store_bias", "gate_drop", "res2_drop"])
def test_gemm_persistent_many_tiles_elementwise(case):
    """Automatic dispatch at 297 tiles of 256^2 (more than the CUs): the 8-phase persistent kernel walks several
    tiles per workgroup. Store, gate and residual kinds per element against float64 torch matmul on the GPU
    (the float32 measurement stays on the CPU), padded strides."""
    run_case(f"c.{case}", spec(*BIG, **EPILOGUES[case]), dev=DEV, strides=(True,))


@pytest.mark.parametrize("case", ["store_bias", "gate_drop"])
def test_gemm_persistent_modes_bit_identical(case):
    """fer_set_persistent_mode 0 (work queue) against 1 (fixed stride), and a repeat call, bit for bit."""
    o = ops()
    M, N, K = BIG
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, device=DEV, generator=g) / math.sqrt(K)).to(torch.bfloat16)
    b = torch.randn(N, device=DEV, generator=g)
    kw = dict(pre_gate=True, act="gelu", dropout=0.1, seed=77) if case == "gate_drop" else {}
    outs = []
    try:
        for mode in (0, 1, 0):
            assert L().fer_set_persistent_mode(mode) == 0, last_error()
            y = torch.full((M, N), float("nan"), device=DEV, dtype=torch.bfloat16)
            pre = torch.full((M, N), float("nan"), device=DEV, dtype=torch.bfloat16) if kw else None
            o.linear_fwd(x, w, b, out=y, pre=pre, **kw)
            outs.append((y, pre))
    finally:
        L().fer_set_persistent_mode(0)
    assert not torch.isnan(outs[0][0].float()).any().item()
    for i, what in ((1, "mode 1 vs mode 0"), (2, "second call")):
        assert_bits_equal(f"c.{case} c {what}", outs[i][0], outs[0][0])
        if kw:
            assert_bits_equal(f"c.{case} pre {what}", outs[i][1], outs[0][1])


# ---------------------------------------------------------------------- (d) split-K
SPLIT_FORMS = {
    "bias_gelu": dict(bias=True, act="gelu"),
    "res_drop": dict(bias=True, res=True, p=0.1),
    "wgrad": dict(a_kc=0, b_kc=0, c_f32=True, accumulate=True),
}


@pytest.mark.parametrize("form", sorted(SPLIT_FORMS))
@pytest.mark.parametrize("via", ["ops_split", "ops_nosplit", "small_ws"])
@pytest.mark.parametrize("cfg", [-1, 5, 8])
def test_gemm_split_k(cfg, via, form):
    """K = 1032 and 1096 (four K chunks, the last of 72 / 136) at 136 x 72 and 264 x 136: ops.gemm with the
    split-K workspace (slabs + splitk_reduce_kernel, which applies the generic epilogue), without it, and the ABI
    with a workspace of 4 M N bytes -- too small for two splits, so the unsplit kernel runs. The same bound for
    all three; bias + GELU, residual + dropout and the weight-gradient form (c_f32, accumulate, both operands
    MN-contiguous); a second call gives the same bits. Automatic configuration and the two 256^2 kernels."""
    with forced_config(cfg):
        for K in (1032, 1096):
            for M, N in ((136, 72), (264, 136)):
                run_case(f"d.cfg{cfg}.{via}.{form}", spec(M, N, K, **SPLIT_FORMS[form]), via=via, repeat=True)


# ---------------------------------------------------------------------- (e) the fp32 kernel
# 64 x 64 tiles, K-step 16: M in {1, 63, 65, 130}, N in {4, 68, 132}, K in {1, 17, 33, 100}
SHAPES_F32 = [(1, 4, 1), (63, 68, 17), (65, 132, 33), (130, 68, 100), (130, 132, 17), (63, 4, 100), (65, 4, 33),
              (1, 132, 100), (130, 4, 1), (63, 132, 1), (1, 68, 33), (65, 68, 17)]


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: f"a_kc{l[0]}-b_kc{l[1]}")
def test_gemm_f32_layout_shapes(layout):
    """gemm_f32_kernel in each layout over the shape list, plain store and bias only; the padded run gives A and
    B odd row strides."""
    a_kc, b_kc = layout
    for M, N, K in SHAPES_F32:
        for bias in (False, True):
            run_case(f"e.{'bias' if bias else 'store'}", spec(M, N, K, dtype="fp32", a_kc=a_kc, b_kc=b_kc, bias=bias))


@pytest.mark.parametrize("case", sorted(EPILOGUES))
def test_gemm_f32_epilogues(case):
    """epi4<float> with every option combination of the bf16 table (the fixed kinds' flag sets included: the fp32
    kernel has one epilogue), M = 65, N = 132, K = 33, in each layout; the column sums are a separate fer_colsum
    pass over the stored fp32 output."""
    for a_kc, b_kc in LAYOUTS:
        run_case(f"e.{case}", spec(65, 132, 33, dtype="fp32", a_kc=a_kc, b_kc=b_kc, **EPILOGUES[case]))


# ---------------------------------------------------------------------- (f) fer_wgrad_group
WG_SHAPES = [(256, 128, False), (136, 200, True), (384, 512, False), (64, 8, True), (520, 264, False), (8, 8, True),
             (72, 136, False), (128, 128, True)]  # (N, K, accumulate): the list of test_wgrad_group and three more


def wg_call(items, splits):
    """items: (dy view, x view, Out dw, N, K, accumulate). Returns the return code."""
    from fervit._lib import WgradItem

    n = len(items)
    arr = (WgradItem * n)()
    for i, (dy, x, dw, N, K, acc) in enumerate(items):
        arr[i] = WgradItem(dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), dw.view.data_ptr(), dw.ld,
                           dy.shape[0], N, K, int(acc))
    nb = L().fer_wgrad_group_ws(arr, min(n, 8), splits)
    ws = torch.empty(max(1, nb // 4 + 1), dtype=torch.float32, device=DEV)
    return L().fer_wgrad_group(arr, n, splits, ws.data_ptr(), ws.numel() * 4, ops().stream())


@functools.lru_cache(maxsize=None)
def wg_operands(tokens):
    g = torch.Generator().manual_seed(tokens)
    r = []
    for N, K, acc in WG_SHAPES:
        dy = torch.randn(tokens, N, generator=g).to(torch.bfloat16)
        x = torch.randn(tokens, K, generator=g).to(torch.bfloat16)
        init = torch.randn(N, K, generator=g) if acc else None
        ref = dy.double().t() @ x.double()
        scale = dy.double().abs().t() @ x.double().abs()
        f32 = dy.float().t() @ x.float()
        if acc:
            ref, scale, f32 = ref + init.double(), scale + init.double().abs(), f32 + init
        r.append((dy, x, init, ref, scale, f32))
    return r


def wg_items(tokens, pad, shapes=WG_SHAPES):
    data = wg_operands(tokens)
    return [(inp(dy, pad, torch.bfloat16), inp(x, 2 * pad, torch.bfloat16), Out(N, K, 3 * pad, torch.float32, init=init), N, K, acc)
            for (N, K, acc), (dy, x, init, _, _, _) in zip(shapes, data)]


@pytest.mark.parametrize("splits", [0, 1, 2, 3])
@pytest.mark.parametrize("tokens", [8, 72, 1000])
def test_wgrad_group_elementwise(tokens, splits):
    """gemm_wgrad_group_kernel with eight items (the limit) per element against float64: ragged tiles, accumulate
    on / off, tight and padded ld_dy / ld_x / ld_dw, NaN guards round every dw, K splits 0 (automatic) to 3 with the
    in-launch ordered reduction; a second launch gives the same bits."""
    data = wg_operands(tokens)
    c = measure_c(f"gemm f.wgrad_group.tokens{tokens}", "bf16", [(f32, ref, scale) for *_, ref, scale, f32 in data])
    for pad in (0, PAD):
        items = wg_items(tokens, pad)
        assert wg_call(items, splits) == 0, last_error()
        for (dy, x, dw, N, K, acc), (*_, ref, scale, _) in zip(items, data):
            name = f"f.wgrad_group tokens={tokens} splits={splits} N={N} K={K} acc={acc} pad={pad}"
            assert_close(name, dw.view, ref, scale, c, 0.0)
            dw.check_guards(name)
        again = wg_items(tokens, pad)
        assert wg_call(again, splits) == 0, last_error()
        for a, b in zip(again, items):
            assert_bits_equal(f"f.wgrad_group N={a[3]} K={a[4]} second launch", a[2].view.contiguous(), b[2].view.contiguous())


def test_wgrad_group_nine_items_is_an_error():
    """More than eight items: non-zero, fer_last_error set, nothing written."""
    items = wg_items(72, PAD)
    items.append(wg_items(72, PAD)[0])
    assert wg_call(items, 1) != 0 and "1..8 items" in last_error()
    torch.cuda.synchronize()
    for it in items:
        it[2].untouched("wgrad_group with nine items")


# ---------------------------------------------------------------------- (g) rejections
def _reject_base(dtype="bf16", M=16, N=16, K=16):
    dt = tdt(dtype)
    A = torch.ones(M + 8, K + 8, dtype=dt, device=DEV)
    B = torch.ones(N + 8, K + 8, dtype=dt, device=DEV)
    X = torch.ones(M + 8, N + 8, dtype=dt, device=DEV)
    c = Out(M, N, PAD, dt)
    return A, B, X, c, dict(dtype=0 if dtype == "bf16" else 1, A=A, lda=K + 8, a_kc=1, B=B, ldb=K + 8, b_kc=1, M=M, N=N,
                            K=K, c=c.view, ldc=c.ld)


REJECTIONS = {
    "n_not_multiple_of_8": (dict(N=12), "multiples of 8"),
    "n_not_multiple_of_4": (dict(N=14), "multiple of 4"),
    "k_tail_a_kc": (dict(K=12), "A layout"),
    "k_tail_b_kc": (dict(K=12, a_kc=0), "B layout"),
    "m_tail_a_mn": (dict(M=12, a_kc=0), "A layout"),
    "lda": (dict(lda=28), "A layout"),
    "ldb": (dict(ldb=28), "B layout"),
    "ldc": (dict(ldc=28), "multiples of 8"),
    "ldp": (dict(pre="X", ldp=28), "multiples of 8"),
    "ldr": (dict(res="X", ldr=28), "multiples of 8"),
    "ldx": (dict(aux="X", ldx=28, aux_act=3), "multiples of 8"),
    "c_pointer": (dict(c="+8"), "16-byte"),
    "colsum_without_workspace": (dict(colsum="cs"), "workspace"),
}


@pytest.mark.parametrize("case", sorted(REJECTIONS))
def test_gemm_rejections(case):
    """Argument checks of gemm_launch (bf16): each returns non-zero, sets fer_last_error and leaves the NaN-filled
    output as it was."""
    over, msg = REJECTIONS[case]
    A, B, X, c, kw = _reject_base()
    pre = Out(16, 16, PAD, torch.bfloat16)
    cs = Out(1, 16, PAD, torch.float32)
    for k, v in over.items():
        if v == "X":
            v = pre.view if k == "pre" else X
        elif v == "+8":
            v = c.view.data_ptr() + 8
        elif v == "cs":
            v = cs.view
        kw[k] = v
    rc = raw_gemm(**kw)
    assert rc != 0, f"{case}: accepted"
    assert msg in last_error(), last_error()
    torch.cuda.synchronize()
    for o_ in (c, pre, cs):
        o_.untouched(case)


@pytest.mark.parametrize("case", ["mismatched_tokens", "ld_dw_below_k", "ld_x_not_multiple_of_8"])
def test_wgrad_group_rejections(case):
    """Argument checks of fer_wgrad_group: non-zero, fer_last_error set, no dw written."""
    from fervit._lib import WgradItem

    M, N, K = 72, 16, 24
    dy = torch.ones(M, N, dtype=torch.bfloat16, device=DEV)
    x = torch.ones(M, K + 8, dtype=torch.bfloat16, device=DEV)
    dws = [Out(N, K, PAD, torch.float32) for _ in range(2)]
    arr = (WgradItem * 2)()
    for i, dw in enumerate(dws):
        arr[i] = WgradItem(dy.data_ptr(), N, x.data_ptr(), K + 8, dw.view.data_ptr(), dw.ld, M, N, K, 0)
    if case == "mismatched_tokens":
        arr[1].M, msg = 64, "same token count"
    elif case == "ld_dw_below_k":
        arr[1].ld_dw, msg = K - 4, "alignment"
    else:
        arr[1].ld_x, msg = K + 4, "alignment"
    ws = torch.empty(1 << 20, dtype=torch.float32, device=DEV)
    rc = L().fer_wgrad_group(arr, 2, 1, ws.data_ptr(), ws.numel() * 4, ops().stream())
    assert rc != 0 and msg in last_error(), (rc, last_error())
    torch.cuda.synchronize()
    for dw in dws:
        dw.untouched(case)
