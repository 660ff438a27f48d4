"""The deferred-reduction window of csrc/reduce.hip driven through the C ABI: the batch kernel
(part_reduce_multi_kernel) element by element, the queue and the arena (reduction_ws / part_reduce), and the
host checks of fer_reduce_defer.

Three kinds of check:
  * Exact: inputs are small integers ({-3..3}, in bf16 or fp32), so every partial and every total is an
    integer far below 2^24 and any summation order gives the same fp32 value: got == the float64 column sum.
    Dropped or doubled rows or blocks, a wrong column mapping and lost ordering all show.
  * Bound: randn inputs, |got - ref| <= c * 2^-23 * |x|.sum(0) with c measured from float32 torch on the CPU
    against the same float64 reference (elemwise.measure_c, as test_gpu_rowops.test_colsum does it).
  * Same bits: the deferred result equals the same call made with the window closed, bit for bit (the
    immediate path is pinned to float64 by test_gpu_rowops.py).
A sum that is claimed to be queued is proven so: its output (NaN or its initial value) holds the same bits
after torch.cuda.synchronize() and before the flush. A call that must run immediately is final after the
synchronize, with no flush.

Every arena is the front of a larger NaN-filled tensor whose tail must keep its bits."""
import functools
import math
import types

import pytest
import torch

import attention_ref as R
from abi_harness import DEV, NAN, f32v, last_error, nanflat, nanview, ops, ptr, tdt, untouched_flat
from abi_harness import lib as L
from elemwise import assert_bits_equal, assert_close, measure_c
from test_gpu_attention_elementwise import Run, case_ref, ctab, family  # noqa: F401 (ctab: a fixture)
from test_gpu_gemm_elementwise import ACT, RAGGED, Out, eff, epilogue, inp, operands, raw_gemm, spec
from test_gpu_rowops import GRADS, call_ln_bwd, call_ln_fwd, ln_bwd_ref, ln_f32, ln_inputs

pytestmark = pytest.mark.gpu

MAX_SET = 2048 * 1024  # reduction_ws defers partial sets up to 2 MB ...
MAX_COLS = 4080        # ... of up to 4080 columns (red_batchable: the 8-column immediate kernel's shapes)
GUARD = 64             # guard elements on each side of an output: one batch-kernel block
WORST = {"ratio": 0.0}


@pytest.fixture(autouse=True)
def closed_window():
    """No test starts inside, or leaves behind, an open window: it would take every later test's sums."""
    assert L().fer_reduce_defer(0, None, 0, None) == 0, last_error()
    yield
    rc = L().fer_reduce_defer(0, None, 0, None)
    torch.cuda.synchronize()
    assert rc == 0, last_error()


# ---------------------------------------------------------------------- helpers
class Arena:
    """`nbytes` of arena at the front of a NaN-filled tensor with a 256 KB tail that nothing may write."""
    TAIL = 65536

    def __init__(self, nbytes):
        self.nbytes = nbytes
        self.n = (nbytes + 3) // 4
        self.parent = torch.full((self.n + self.TAIL,), NAN, dtype=torch.float32, device=DEV)

    def open(self):
        """fer_reduce_defer(1, ...) on the current stream; returns the return code."""
        return L().fer_reduce_defer(1, self.parent.data_ptr(), self.nbytes, ops().stream())

    def check(self, name):
        tail = self.parent[self.n:]
        assert_bits_equal(f"{name}: arena tail", tail, torch.full_like(tail, NAN))


def opened(nbytes):
    a = Arena(nbytes)
    assert a.open() == 0, last_error()
    return a


def flush():
    assert L().fer_reduce_flush() == 0, last_error()
    torch.cuda.synchronize()


def close():
    assert L().fer_reduce_defer(0, None, 0, None) == 0, last_error()
    torch.cuda.synchronize()


def colsum(xv, out, acc=False, scale=None):
    """fer_colsum through the ABI on the current stream, with a workspace of exactly fer_colsum_ws bytes."""
    M, N = xv.shape
    nbytes = L().fer_colsum_ws(M, N)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=DEV)
    rc = L().fer_colsum(ops().dcode(xv), xv.data_ptr(), xv.stride(0), M, N, out.data_ptr(), int(acc), ptr(scale),
                        ws.data_ptr(), nbytes, ops().stream())
    assert rc == 0, last_error()


def colsum_nb(M):
    return min(-(-M // 32), 256)


def deferrable(M, N):
    """The documented rule of the window: sets up to 2 MB, up to 4080 columns."""
    return N <= MAX_COLS and colsum_nb(M) * N * 4 <= MAX_SET


class Vec:
    """An fp32 output [n] inside a NaN-filled parent with GUARD elements on each side. init: None (NaN) or the
    values an accumulate lands on."""

    def __init__(self, n, init=None):
        self.n = n
        self.v, self.parent = nanflat(n, torch.float32, init, guard=GUARD)
        self.before = self.parent.clone()

    def unchanged(self, name):
        assert_bits_equal(f"{name}: not queued (written before the flush)", self.parent, self.before)

    def guards(self, name):
        untouched_flat(name, self.parent, self.n, guard=GUARD)

    def f64(self):
        return self.v.cpu().double()


def is_exact(name, vec, ref):
    got = vec.f64()
    bad = got != ref  # NaN != ref
    assert not bad.any().item(), (f"{name}: {int(bad.sum())} of {bad.numel()} sums differ from the exact integer sum, "
                                  f"first at {int(bad.nonzero()[0])}: {got[bad][0].item()} vs {ref[bad][0].item()}")
    vec.guards(name)


@functools.lru_cache(maxsize=2)
def sources(M, N):
    """randn and integer sources of one shape (shared by both dtypes) and integer / random initial values."""
    g = torch.Generator().manual_seed(M * 4099 + N)
    return types.SimpleNamespace(x=torch.randn(M, N, generator=g),
                                 xi=torch.randint(-3, 4, (M, N), generator=g, dtype=torch.int8).float(),
                                 init=torch.randn(N, generator=g) * 5,
                                 initi=torch.randint(-5, 6, (N,), generator=g).float())


def ints(M, N, seed, dtype="fp32", mult=1):
    """An integer input ({-3..3} * mult) as a device view with row stride N + 4, and its float64 column sum."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, (M, N), generator=g).float() * mult
    xv = nanview(M, N, 4, tdt(dtype), x, guard=0)[0]
    return xv, x.double().sum(0)


# ---------------------------------------------------------------------- 1. the batch kernel, element by element
NBS = (1, 31, 32, 33, 224, 225, 256)
WIDTHS = (4, 60, 64, 68, 4080)
BATCH_CASES = sorted({(32 * nb, 68) for nb in NBS} | {(33, 68)} | {(32 * nb, N) for nb in (33, 256) for N in WIDTHS})


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("M,N", BATCH_CASES)
def test_batch_kernel_colsum(dtype, M, N):
    """part_reduce_multi_kernel behind fer_colsum (nb = min(ceil(M / 32), 256) partial rows of N columns, input
    row stride N + 4): nb = 1, 31, 32, 33 around the 32 row phases, 224 / 225 on either side of the 8-deep
    iteration (`bb + 224 < nb`), 256 the cap, M = 33 two blocks of 17 and 16 rows; N = 4 one live lane, 60 a short
    block, 64 one block, 68 a second block with 4 live lanes, 4080 the widest batchable (64 blocks).
    Seven reductions are queued before the one flush -- wide, this shape (randn, plain), narrow, this shape
    (randn, accumulate on random values), this shape (integers, plain and accumulate), wide -- so the block walk
    over blk0 meets descriptors that do not start at block 0. nb = 256 at N = 4080 is a 4 MB set, above the 2 MB
    cut-off: those four run immediately (asserted final before the flush) and the check is the immediate
    kernel's."""
    dt = tdt(dtype)
    s = sources(M, N)
    queued = deferrable(M, N)
    print(f"colsum M={M} N={N}: nb = {colsum_nb(M)}, {'queued' if queued else 'immediate (set above 2 MB)'}")
    xv = nanview(M, N, 4, dt, s.x, guard=0)[0]
    xiv = nanview(M, N, 4, dt, s.xi, guard=0)[0]
    x = xv.float().cpu()
    ref, scale = x.double().sum(0), x.double().abs().sum(0)
    f32 = x.sum(0)
    refi = s.xi.double().sum(0)
    wide_a, ref_a = ints(96, 132, 1)
    narrow, ref_n = ints(64, 4, 2, "bf16")
    wide_b, ref_b = ints(160, 200, 3, "bf16")

    def outs():
        return types.SimpleNamespace(a=Vec(132), plain=Vec(N), n=Vec(4), acc=Vec(N, s.init), iplain=Vec(N),
                                     iacc=Vec(N, s.initi), b=Vec(200))

    def run(o):
        colsum(wide_a, o.a.v)
        colsum(xv, o.plain.v)
        colsum(narrow, o.n.v)
        colsum(xv, o.acc.v, acc=True)
        colsum(xiv, o.iplain.v)
        colsum(xiv, o.iacc.v, acc=True)
        colsum(wide_b, o.b.v)

    imm = outs()
    run(imm)
    torch.cuda.synchronize()
    arena = opened(16 << 20)
    d = outs()
    run(d)
    torch.cuda.synchronize()
    for k in ("a", "n", "b"):
        getattr(d, k).unchanged(f"filler {k}")
    if queued:
        for k in ("plain", "acc", "iplain", "iacc"):
            getattr(d, k).unchanged(k)
    else:
        for k in ("plain", "acc", "iplain", "iacc"):
            assert_bits_equal(f"{k}: a set above 2 MB runs immediately", getattr(d, k).parent, getattr(imm, k).parent)
    flush()
    arena.check("batch")
    # Exact
    is_exact("wide filler a", d.a, ref_a)
    is_exact("narrow filler", d.n, ref_n)
    is_exact("wide filler b", d.b, ref_b)
    is_exact("integers", d.iplain, refi)
    is_exact("integers, accumulate", d.iacc, refi + s.initi.double())
    # Bound
    c = measure_c("window.colsum", dtype, [(f32, ref, scale)])
    w = assert_close(f"deferred colsum {dtype}", d.plain.v, ref, scale, c, 0.0)
    ref2, scale2 = s.init.double() + ref, s.init.double().abs() + scale
    c2 = measure_c("window.colsum.acc", dtype, [(s.init + f32, ref2, scale2)])
    w = max(w, assert_close(f"deferred colsum {dtype} accumulate", d.acc.v, ref2, scale2, c2, 0.0))
    d.plain.guards("plain")
    d.acc.guards("accumulate")
    WORST["ratio"] = max(WORST["ratio"], w)
    print(f"window colsum {dtype} M={M} N={N}: worst err/bound {w:.3f} (module so far {WORST['ratio']:.3f})")
    # Same bits
    for k in vars(d):
        assert_bits_equal(f"{k}: deferred vs window closed", getattr(d, k).parent, getattr(imm, k).parent)


# ---- LayerNorm backward: the segmented form (ncols = 3 D, seg = D)
def ln_case(dtype, M, D):
    """Device operands of one LayerNorm backward (no residual, no dropout) with the statistics of its own
    forward, the float64 gradients and the c of each."""
    dt = tdt(dtype)
    x0, gam, bet, dy0, _ = ln_inputs(M, D, 1, 1000 * D + M)
    t = types.SimpleNamespace(M=M, D=D)
    t.x, t.dy = nanview(M, D, 0, dt, x0, guard=0)[0], nanview(M, D, 0, dt, dy0, guard=0)[0]
    t.g, b = gam.to(DEV).contiguous(), bet.to(DEV).contiguous()
    t.mean, t.rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    y = torch.empty(M, D, dtype=dt, device=DEV)
    eps = f32v(1e-5)
    assert call_ln_fwd(t.x, t.g, b, 1, 1, y, t.mean, t.rstd, M, D, eps) == 0, last_error()
    t.dx = torch.empty(M, D, dtype=dt, device=DEV)
    t.nb = L().fer_layernorm_bwd_ws(M, D) // (12 * D)
    x, dy = t.x.float().cpu().double(), t.dy.float().cpu().double()
    G = gam.double()[torch.zeros(M, dtype=torch.long)]
    t.ref = ln_bwd_ref(x, dy, G, None, t.mean.cpu().double(), t.rstd.cpu().double(), None, 1.0)
    mu = x.mean(1)
    rs = (((x - mu[:, None]) ** 2).mean(1) + eps) ** -0.5  # the statistics float32 torch works from
    bx = ln_bwd_ref(x, dy, G, None, mu, rs, None, 1.0)
    t32 = ln_f32(x, gam, bet, torch.zeros(M, dtype=torch.long), eps, dy, None, None, 1.0)
    t.c = {k: measure_c(f"window.ln.{k}", dtype, [(t32[k], bx[k], bx["s_" + k])]) for k in GRADS}
    return t


def ln_bwd(t, flat, want, acc=False, base=0):
    """fer_layernorm_bwd with dgamma, dbeta, dbias = the three D-slices of `flat` from `base` (null unless wanted)."""
    o = [flat[base + k * t.D:base + (k + 1) * t.D] if GRADS[k] in want else None for k in range(3)]
    rc = call_ln_bwd(t.dy, t.x, t.mean, t.rstd, t.g, 1, 1, None, t.dx, None, 0, 1.0, 0, o[0], o[1], o[2], acc, t.M, t.D)
    assert rc == 0, last_error()


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("want,acc", [(GRADS, False), (GRADS, True), (("dbeta",), False), (("dbias",), False)],
                         ids=["all", "all-accumulate", "dbeta", "dbias"])
def test_batch_kernel_layernorm_bwd(dtype, want, acc):
    """fer_layernorm_bwd, M = 100, D = 68: 204 columns in segments of 68, so the 64-column blocks straddle both
    segment boundaries and the last block has 12 live lanes. dgamma / dbeta / dbias are the three slices of one
    guarded buffer; with only dbeta (o0 null) or only dbias (o0 and o1 null) the slices of the outputs that
    were not asked for keep their NaN. Queued between a wide and a narrow colsum."""
    M, D = 100, 68
    t = ln_case(dtype, M, D)
    print(f"layernorm_bwd M={M} D={D}: nb = {t.nb}")
    g = torch.Generator().manual_seed(11)
    init = torch.randn(3 * D, generator=g) * 3 if acc else None
    wide, ref_w = ints(96, 132, 4)
    narrow, ref_n = ints(64, 4, 5)
    imm = Vec(3 * D, init)
    ln_bwd(t, imm.v, want, acc)
    torch.cuda.synchronize()
    arena = opened(1 << 20)
    d, ow, on = Vec(3 * D, init), Vec(132), Vec(4)
    colsum(wide, ow.v)
    ln_bwd(t, d.v, want, acc)
    colsum(narrow, on.v)
    torch.cuda.synchronize()
    for name, v in (("layernorm_bwd", d), ("wide", ow), ("narrow", on)):
        v.unchanged(name)
    flush()
    arena.check("layernorm_bwd")
    is_exact("wide", ow, ref_w)
    is_exact("narrow", on, ref_n)
    assert_bits_equal("layernorm_bwd: deferred vs window closed", d.parent, imm.parent)
    d.guards("layernorm_bwd")
    got = d.f64()
    for k, name in enumerate(GRADS):
        sl = slice(k * D, (k + 1) * D)
        if name not in want:
            assert torch.isnan(got[sl]).all().item(), f"{name} was not asked for and was written"
            continue
        ref, scale = t.ref[name], t.ref["s_" + name]
        if acc:
            ref, scale = ref + init[sl].double(), scale + init[sl].double().abs()
        w = assert_close(f"deferred {name} {dtype}", got[sl], ref, scale, t.c[name], 0.0)
        WORST["ratio"] = max(WORST["ratio"], w)
        print(f"window layernorm_bwd {dtype} {name}: worst err/bound {w:.3f} (module so far {WORST['ratio']:.3f})")


def test_batch_kernel_dead_lanes_do_not_store():
    """The last block of a 204-column LayerNorm reduction has 52 lanes past ncols. A store from them would
    land on dbias[0..51] (c / seg = 3 selects the third output) with a sum of 0, racing the block that owns
    those columns, so one reduction shows it only now and then: 40 of them in one launch, each into a buffer
    of its own, every one the bits of the call with the window closed."""
    t = ln_case("fp32", 100, 68)
    imm = Vec(204)
    ln_bwd(t, imm.v, GRADS)
    torch.cuda.synchronize()
    arena = opened(1 << 20)
    bufs = [Vec(204) for _ in range(40)]
    for i, b in enumerate(bufs):
        ln_bwd(t, b.v, GRADS if i % 2 else ("dbias",))
    torch.cuda.synchronize()
    for b in bufs:
        b.unchanged("layernorm_bwd")
    flush()
    arena.check("dead lanes")
    for i, b in enumerate(bufs):
        assert_bits_equal(f"reduction {i} of 40: dbias", b.v[136:], imm.v[136:])
        if i % 2:
            assert_bits_equal(f"reduction {i} of 40", b.parent, imm.parent)
        else:
            assert torch.isnan(b.v[:136]).all().item(), f"reduction {i} of 40: outputs that were not asked for"
            b.guards(f"reduction {i} of 40")


# ---- fer_gemm's fused column sums
@pytest.mark.parametrize("mode", ["plain", "acc"])
def test_batch_kernel_gemm_colsum(mode):
    """fer_gemm with the colsum epilogue (bf16, the EPI_MUL form of the GEMM module's `mul2_colsum` cases,
    M = 264, N = 136, K = 200, its smallest colsum shape): one partial row per tile row, nb = ceil(M / tile
    rows). Plain and colsum_accumulate, against the GEMM module's float64 epilogue and bound."""
    M, N, K = RAGGED
    sp = spec(M, N, K, aux="mul", colsum=mode)
    print(f"gemm colsum M={M} N={N}: nb = {-(-M // 256)} or {-(-M // 128)} (tile rows of 256 or 128)")
    op = operands(M, N, K, "bf16")
    t = types.SimpleNamespace(bias=op.bias, res=None, aux=op.aux, cs_old=op.cs_old, drop_scale=1.0, keep=None,
                              c_old=None)
    r = epilogue(op.acc, op.sacc, t, sp, torch.float64)
    q = epilogue(op.acc32, torch.zeros(M, N, dtype=torch.float64), t, sp, torch.float32)
    c = measure_c("window.gemm.colsum", "bf16", [(q.colsum, r.colsum, r.s_colsum)])
    A, B, aux = inp(op.A, 8, torch.bfloat16), inp(op.B, 16, torch.bfloat16), inp(op.aux, 40, torch.bfloat16)
    ws = torch.empty(L().fer_gemm_colsum_ws(M, N) // 4, dtype=torch.float32, device=DEV)

    def call():
        cout = Out(M, N, 8, torch.bfloat16)
        col = Out(1, N, 8, torch.float32, init=op.cs_old[None] if mode == "acc" else None)
        rc = raw_gemm(dtype=0, A=A, lda=A.stride(0), a_kc=1, B=B, ldb=B.stride(0), b_kc=1, M=M, N=N, K=K, ws=ws,
                      c=cout.view, ldc=cout.ld, aux=aux, ldx=aux.stride(0), aux_act=ACT["mul"], colsum=col.view,
                      colsum_accumulate=int(mode == "acc"))
        assert rc == 0, last_error()
        return cout, col

    c_imm, col_imm = call()
    torch.cuda.synchronize()
    arena = opened(1 << 20)
    wide, ref_w = ints(96, 132, 6)
    ow = Vec(132)
    colsum(wide, ow.v)
    c_def, col_def = call()
    torch.cuda.synchronize()
    col_def.untouched("gemm colsum: queued")
    ow.unchanged("wide")
    flush()
    arena.check("gemm")
    is_exact("wide", ow, ref_w)
    assert_bits_equal("gemm c with the window open / closed", c_def.parent, c_imm.parent)
    assert_bits_equal("gemm colsum: deferred vs window closed", col_def.parent, col_imm.parent)
    col_def.check_guards("gemm colsum")
    w = assert_close("deferred gemm colsum", col_def.view[0], r.colsum, eff(r.s_colsum, r.a_colsum, c), c, 0.0)
    print(f"window gemm colsum {mode}: worst err/bound {w:.3f}")


# ---- fer_attention_bwd's bias gradient
@pytest.mark.parametrize("B,N,H,dh", [(2, 1, 2, 64), (2, 225, 2, 24), (40, 224, 2, 64)],
                         ids=["persistent", "fused", "persistent-nb280"])
def test_batch_kernel_attention_colsum(B, N, H, dh, ctab):  # noqa: F811
    """fer_attention_bwd with colsum, bf16, at the smallest N, H, dh of the attention module's persistent
    (N = 1: B * 1 partial rows) and fused (N = 225, dh = 24: B partial rows) cases, accumulated onto the
    module's known vector, against its float64 check. The third case is the producer with more than 256
    partial rows: the persistent family writes B * ceil(N / 32) = 40 * 7 = 280 of them, so the 8-deep
    iteration runs and leaves a tail (phases 0..23 have a ninth row)."""
    fam = family("bf16", N, dh)
    assert fam == ("fused" if N == 225 else "pers")
    nb = B * (-(-N // 32)) if fam == "pers" else B
    print(f"attention_bwd {fam} B={B} N={N} H={H} dh={dh}: nb = {nb}")
    qkv, dout, keep, r, seed = case_ref(B, N, H, dh, "normal", 0.0)
    imm = Run("bf16", B, N, H, dh, 0.0, qkv, dout, seed, False).forward()
    imm.backward("acc")
    arena = opened(1 << 20)
    wide, ref_w = ints(96, 132, 7)
    ow = Vec(132)
    colsum(wide, ow.v)
    d = Run("bf16", B, N, H, dh, 0.0, qkv, dout, seed, False).forward()
    d.backward("acc")  # synchronizes
    ow.unchanged("wide")
    assert_bits_equal("attention colsum: queued", d.cs, d.cs_old)
    flush()
    arena.check("attention")
    is_exact("wide", ow, ref_w)
    assert_bits_equal("attention colsum: deferred vs window closed", d.cs_par, imm.cs_par)
    assert_bits_equal("attention dqkv with the window open / closed", d.dqkv, imm.dqkv)
    r.bwd(d.out.float())
    wb = {}
    R.check_colsum(f"deferred attention {fam}", r, d.cs, d.cs_old, ctab["bf16"], "bf16", sums_rounded=False, worst=wb)
    print(f"window attention colsum {fam}: worst err/bound {wb['colsum']:.3f}")


# ---------------------------------------------------------------------- 2. the queue and the arena
def test_queue_overflow():
    """60 small sums (M = N = 64) in one window: more than the batch takes, so reduction_ws runs the full queue
    before it hands out the next slice. Before any explicit flush the first is final and the last is not."""
    arena = opened(1 << 20)
    xs = [ints(64, 64, 100 + i, "bf16" if i % 2 else "fp32") for i in range(60)]
    outs = [Vec(64) for _ in xs]
    for (xv, _), o in zip(xs, outs):
        colsum(xv, o.v)
    torch.cuda.synchronize()
    is_exact("first of 60, before the flush", outs[0], xs[0][1])
    outs[-1].unchanged("last of 60")
    flush()
    arena.check("overflow")
    for i, ((_, ref), o) in enumerate(zip(xs, outs)):
        is_exact(f"sum {i} of 60", o, ref)


def test_arena_wrap():
    """The minimum arena (65536 bytes) and seven sets of 20480 bytes (M = 640, N = 256): the fourth and the
    seventh do not fit, so the queue runs before the arena is reused from its start. A wrap that overwrote
    partials that were not summed yet gives wrong sums for the first sets."""
    arena = opened(65536)
    assert L().fer_colsum_ws(640, 256) == 20480
    xs = [ints(640, 256, 200 + i, "bf16" if i % 2 else "fp32") for i in range(7)]
    outs = [Vec(256) for _ in xs]
    for (xv, _), o in zip(xs, outs):
        colsum(xv, o.v)
    torch.cuda.synchronize()
    is_exact("first of 7, before the flush", outs[0], xs[0][1])
    outs[-1].unchanged("last of 7")
    flush()
    arena.check("wrap")
    for i, ((_, ref), o) in enumerate(zip(xs, outs)):
        is_exact(f"set {i} of 7", o, ref)


def test_cutoffs():
    """A 16 MB arena: M = 8192, N = 2052 is a set of 256 * 2052 * 4 bytes, above 2 MB, and runs immediately;
    M = 64, N = 4084 is not batchable (256 blocks of 16 columns) and runs immediately on
    part_reduce_kernel<16>; M = 64, N = 4080 is queued."""
    arena = opened(16 << 20)
    assert L().fer_colsum_ws(8192, 2052) > MAX_SET
    big, ref_big = ints(8192, 2052, 300, "bf16")
    wide, ref_wide = ints(64, 4084, 301)
    edge, ref_edge = ints(64, 4080, 302)
    ob, ow, oe = Vec(2052), Vec(4084), Vec(4080)
    colsum(big, ob.v)
    colsum(wide, ow.v)
    colsum(edge, oe.v)
    torch.cuda.synchronize()
    is_exact("set above 2 MB: immediate", ob, ref_big)
    is_exact("N = 4084: immediate", ow, ref_wide)
    oe.unchanged("N = 4080")
    flush()
    arena.check("cutoffs")
    is_exact("N = 4080", oe, ref_edge)
    is_exact("set above 2 MB after the flush", ob, ref_big)
    is_exact("N = 4084 after the flush", ow, ref_wide)


def test_set_larger_than_arena():
    """A 64 KB arena: a set of 81920 bytes (M = 640, N = 1024) cannot be taken and runs immediately; the small
    set after it is queued as usual."""
    arena = opened(65536)
    assert L().fer_colsum_ws(640, 1024) > 65536
    big, ref_big = ints(640, 1024, 400, "bf16")
    small, ref_small = ints(64, 64, 401)
    ob, os_ = Vec(1024), Vec(64)
    colsum(big, ob.v)
    colsum(small, os_.v)
    torch.cuda.synchronize()
    is_exact("set above the arena: immediate", ob, ref_big)
    os_.unchanged("small set after it")
    flush()
    arena.check("larger than arena")
    is_exact("small set", os_, ref_small)
    is_exact("set above the arena after the flush", ob, ref_big)


def test_other_stream():
    """The window belongs to the stream it was opened on: a colsum on another stream runs immediately there
    and leaves the queue alone."""
    arena = opened(1 << 20)
    first, ref_first = ints(96, 132, 500)
    other, ref_other = ints(64, 68, 501, "bf16")
    of, oo = Vec(132), Vec(68)
    colsum(first, of.v)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert ops().stream() == side.cuda_stream
        colsum(other, oo.v)
    side.synchronize()
    is_exact("other stream: immediate", oo, ref_other)
    torch.cuda.synchronize()
    of.unchanged("queued before the other stream's call")
    flush()
    arena.check("other stream")
    is_exact("queued sum", of, ref_first)
    is_exact("other stream after the flush", oo, ref_other)


def test_scale_pointer_in_window():
    """A device scale is not batchable. Onto a queued output the queue runs first and the scaled accumulate
    lands on its result: out = a - 0.75 b, exact with inputs that are multiples of 4. Into an output of its own
    it runs immediately as well (the batch kernel has no scale). The next plain set is queued again."""
    arena = opened(1 << 20)
    a, ref_a = ints(96, 132, 600, mult=4)
    b, ref_b = ints(160, 132, 601, "bf16", mult=4)
    small, ref_s = ints(64, 64, 602)
    s = torch.tensor([-0.75], device=DEV)
    out, own, os_ = Vec(132), Vec(132), Vec(64)
    colsum(a, out.v)
    torch.cuda.synchronize()
    out.unchanged("a")
    colsum(b, out.v, acc=True, scale=s)
    torch.cuda.synchronize()
    is_exact("a - 0.75 b, before the flush", out, ref_a - 0.75 * ref_b)
    colsum(a, own.v, scale=s)  # an output no queued sum touches
    colsum(small, os_.v)
    torch.cuda.synchronize()
    is_exact("-0.75 a into its own output: immediate", own, -0.75 * ref_a)
    os_.unchanged("the set after the scaled ones")
    flush()
    arena.check("scale")
    is_exact("small set", os_, ref_s)
    is_exact("a - 0.75 b after the flush", out, ref_a - 0.75 * ref_b)
    is_exact("-0.75 a after the flush", own, -0.75 * ref_a)


def test_overlap_scan_segmented_outputs():
    """The overlap scan of part_reduce against the three output ranges of a segmented reduction. A queued
    LayerNorm backward (D = 64) writes the three slices of one flat [192] buffer:
      * an accumulating colsum into flat[32:96] (segments 0 and 1), and one into flat[96:160] (segments 1 and
        2 only), run the queue first and then themselves: final after the synchronize, the bits of the same
        two calls with the window closed;
      * the other way round, a queued colsum into flat[128:192] and then the LayerNorm backward (only its
        third output overlaps);
      * a colsum into the 64 floats right behind the queued range is adjacent, not overlapping: both stay
        queued."""
    M, D = 100, 64
    t = ln_case("bf16", M, D)
    print(f"layernorm_bwd M={M} D={D}: nb = {t.nb}")
    xa, ref_a = ints(96, 64, 700)

    init = torch.randn(192, generator=torch.Generator().manual_seed(701))

    def ln_then_colsum(lo):
        buf = Vec(192)
        ln_bwd(t, buf.v, GRADS)
        state = buf.parent.clone()
        colsum(xa, buf.v[lo:lo + 64], acc=True)
        return buf, state

    def colsum_then_ln():
        buf = Vec(192, init)
        colsum(xa, buf.v[128:192])
        state = buf.parent.clone()
        ln_bwd(t, buf.v, GRADS, acc=True)
        return buf, state

    imm = [ln_then_colsum(32)[0], ln_then_colsum(96)[0], colsum_then_ln()[0]]
    torch.cuda.synchronize()
    for b in imm:  # NaN + x = NaN: every accumulate found finished sums
        assert not torch.isnan(b.v).any().item()
        b.guards("overlap, window closed")
    arena = opened(1 << 20)
    for i, fn in enumerate((lambda: ln_then_colsum(32), lambda: ln_then_colsum(96), colsum_then_ln)):
        buf, state = fn()
        torch.cuda.synchronize()
        # `state` was cloned on the stream after the first call: it holds what that call had written by then
        assert_bits_equal(f"overlap {i}: the first call was queued", state, buf.before)
        assert_bits_equal(f"overlap {i}: queue first, then the overlapping call", buf.parent, imm[i].parent)
        flush()
        assert_bits_equal(f"overlap {i}: after the flush", buf.parent, imm[i].parent)
    # adjacent
    buf = Vec(256)
    ln_bwd(t, buf.v, GRADS)
    colsum(xa, buf.v[192:256])
    torch.cuda.synchronize()
    buf.unchanged("adjacent ranges")
    flush()
    arena.check("overlap")
    ref = Vec(256)
    close()
    ln_bwd(t, ref.v, GRADS)
    colsum(xa, ref.v[192:256])
    torch.cuda.synchronize()
    assert_bits_equal("adjacent: deferred vs window closed", buf.parent, ref.parent)
    assert torch.equal(buf.v[192:256].cpu().double(), ref_a)


def test_two_accumulates_one_output():
    """Two accumulates onto one output in one window: the second finds the first queued, so the queue runs
    and then the second: init + a + b, complete after the synchronize and unchanged by the flush."""
    arena = opened(1 << 20)
    a, ref_a = ints(96, 132, 800)
    b, ref_b = ints(160, 132, 801, "bf16")
    g = torch.Generator().manual_seed(802)
    init = torch.randint(-5, 6, (132,), generator=g).float()
    out = Vec(132, init)
    colsum(a, out.v, acc=True)
    torch.cuda.synchronize()
    out.unchanged("first accumulate")
    colsum(b, out.v, acc=True)
    torch.cuda.synchronize()
    is_exact("init + a + b before the flush", out, init.double() + ref_a + ref_b)
    flush()
    arena.check("two accumulates")
    is_exact("init + a + b after the flush", out, init.double() + ref_a + ref_b)


def test_reopen():
    """Mode 1 again with the same arena, size and stream keeps the queue; with another arena the old queue
    runs first; a paused window (mode 2) takes nothing new and a flush still runs what it holds; mode 0 with
    nothing open returns 0."""
    a1, a2 = Arena(1 << 20), Arena(1 << 20)
    x1, r1 = ints(96, 132, 900)
    x2, r2 = ints(64, 68, 901, "bf16")
    x3, r3 = ints(64, 64, 902)
    o1, o2, o3 = Vec(132), Vec(68), Vec(64)
    assert a1.open() == 0, last_error()
    colsum(x1, o1.v)
    assert a1.open() == 0, last_error()
    torch.cuda.synchronize()
    o1.unchanged("same arena again")
    assert a2.open() == 0, last_error()
    torch.cuda.synchronize()
    is_exact("another arena: the old queue ran", o1, r1)
    colsum(x2, o2.v)
    assert L().fer_reduce_defer(2, None, 0, None) == 0, last_error()
    colsum(x3, o3.v)
    torch.cuda.synchronize()
    is_exact("paused: immediate", o3, r3)
    o2.unchanged("queued before the pause")
    flush()
    is_exact("flush of a paused window", o2, r2)
    close()
    assert L().fer_reduce_defer(0, None, 0, None) == 0
    a1.check("reopen 1")
    a2.check("reopen 2")
    is_exact("o1 at the end", o1, r1)


@pytest.mark.parametrize("case", ["short", "null", "mode"])
def test_rejected_calls_leave_no_window(case):
    """An arena of 65535 bytes, a null arena and mode 3 return the library's error and open nothing: the next
    colsum runs immediately."""
    a = Arena(65536)
    st = ops().stream()
    if case == "short":
        rc, msg = L().fer_reduce_defer(1, a.parent.data_ptr(), 65535, st), "reduce_defer: arena too small"
    elif case == "null":
        rc, msg = L().fer_reduce_defer(1, None, 65536, st), "reduce_defer: arena too small"
    else:
        rc, msg = L().fer_reduce_defer(3, a.parent.data_ptr(), 65536, st), "reduce_defer: mode must be 0, 1 or 2"
    assert rc != 0 and msg in last_error(), (rc, last_error())
    x, ref = ints(64, 64, 1000)
    out = Vec(64)
    colsum(x, out.v)
    torch.cuda.synchronize()
    is_exact("after a rejected fer_reduce_defer: immediate", out, ref)
    assert_bits_equal("arena of a rejected call", a.parent, torch.full_like(a.parent, NAN))


# ---------------------------------------------------------------------- 3. fer_colsum_ws
@pytest.mark.parametrize("M,N", [(33, 4084), (3001, 4084), (33, 8192), (3001, 8192), (1, 4), (8193, 68)])
def test_colsum_ws(M, N):
    """fer_colsum_ws = min(ceil(M / 32), 256) * N * 4; with one byte less, or a null workspace, fer_colsum
    returns "workspace too small" and writes neither the output nor the workspace."""
    need = L().fer_colsum_ws(M, N)
    assert need == min(math.ceil(M / 32), 256) * N * 4
    x = torch.ones(M, N, device=DEV)
    out = Vec(N)
    ws = torch.full((need // 4,), NAN, device=DEV)
    for wsp, nbytes in ((ws.data_ptr(), need - 1), (None, need)):
        rc = L().fer_colsum(1, x.data_ptr(), N, M, N, out.v.data_ptr(), 0, None, wsp, nbytes, ops().stream())
        assert rc != 0 and "colsum: workspace too small" in last_error(), (rc, last_error())
    torch.cuda.synchronize()
    out.unchanged("rejected colsum")
    assert_bits_equal("workspace of a rejected colsum", ws, torch.full_like(ws, NAN))
    colsum(x, out.v)
    torch.cuda.synchronize()
    is_exact("with exactly fer_colsum_ws bytes", out, torch.full((N,), float(M), dtype=torch.float64))
