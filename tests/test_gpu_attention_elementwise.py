"""Attention core, element by element against float64: every forward kernel
(attn_fwd_pers<1..7>, attn_fwd_occ<1..7>, attn_fwd_bf16, attn_fwd_gen<1,2>), every backward family
(attn_bwd_pers<1..7>, attn_bwd_fused_bf16, attn_dq_gen / attn_dkv_gen) and the fp32 parity kernels of
csrc/attention.hip, through the raw C ABI with tight and padded row strides, every operand a view into a
NaN-filled parent whose padding columns and guard rows must keep their bits.

The reference, the error model and the checks are tests/attention_ref.py; tests/test_attention_bound_cpu.py
shows on the CPU that a correct bf16 pipeline passes them and that block-edge, keep-bit and delta slips
fail them. c comes from float32 torch on the CPU (elemwise.measure_c), never from a kernel.

l_round of the lse bound is 0 for every kernel: each forward sums the row from the fp32 exponentials and
rounds to bf16 only afterwards, for the P.V MFMA (csrc/attention.hip: attn_fwd_bf16 `l += st[r]` ahead of
drop16_keys / pack8; attn_fwd_pers and attn_fwd_occ `l += (ls[0] + ls[1]) + (ls[2] + ls[3])` ahead of the
keep select and pack8; attn_fwd_gen `l += st[r]`; attn_f32_softmax is fp32 throughout)."""
import functools
import math

import pytest
import torch

import attention_ref as R
from abi_harness import DEV, NAN, last_error, lib, nanvec, nanview, ptr, tdt, untouched, untouched_vec
from elemwise import assert_bits_equal

pytestmark = pytest.mark.gpu

GUARD = 8
# padding columns: out 8, dout 16, qkv 24, dqkv 40 -- no two row strides of a call are equal
PADS = {"qkv": 24, "out": 8, "dout": 16, "dqkv": 40}
WORST = {}  # (kernel family, output) -> worst err / bound seen, printed by every test as a record


def stream():
    return torch.cuda.current_stream().cuda_stream


def family(dtype, N, dh):
    """The kernels the dispatcher (fer_attention_fwd / fer_attention_bwd) takes for this case.

    The library decides this in attn_plan() (csrc/attention.hip). The rule is restated here on purpose: an
    independent statement, so that a slip in the plan shows as a case checked against the wrong family's
    bounds and forced kernels instead of passing unnoticed."""
    if dtype == "fp32":
        return "f32"
    if N <= 224 and dh <= 64:
        return "pers"
    if N <= 256 and dh <= 64:
        return "fused"
    return "gen"


@pytest.fixture(scope="module")
def ctab():
    cases = [(1, N, 2, 64, style, p) for N in (70, 197) for style in ("normal", "peaked") for p in (0.0, 0.1)]
    cases += [(1, 300, 1, 128, "normal", 0.1), (1, 37, 2, 24, "peaked", 0.5)]
    return {dt: R.c_table(cases, dt) for dt in ("bf16", "fp32")}


@pytest.fixture(scope="module")
def ctab_offset():
    """c of the score-offset inputs, measured on their own: fp32 scores of size 40 to 100 cost float32 torch
    more than the other inputs, and the other cases should not inherit that slack."""
    cases = [(1, 100, 2, 64, "offset", 0.1), (1, 300, 1, 128, "offset", 0.1)]
    return {dt: R.c_table(cases, dt + "(offset)") for dt in ("bf16", "fp32")}


@functools.lru_cache(maxsize=48)
def case_ref(B, N, H, dh, style, p, device="cpu"):
    """Inputs, keep mask and fp64 forward reference of one case (shared by dtypes, strides and kernel forms;
    the backward part is redone per call, from the kernel's own out)."""
    seed = 4242 + N
    qkv, dout = R.make_inputs(B, N, H, dh, style, 1000 * N + dh)
    qkv, dout = qkv.to(device), dout.to(device)
    _, ds = R.drop_params(p)
    keep = R.attn_keep(seed, B, N, H, p, device)
    r = R.Ref(qkv, dout, B, N, H, dh, R.f32(1.0 / math.sqrt(dh)), keep, ds)
    return qkv, dout, keep, r, seed


def keep_words(saved, B, N, H):
    """The stored keep words [B*H][nb][nb][32] (int64, 0 .. 2^32-1) behind lse in the saved state."""
    nb = (N + 31) // 32
    off = (B * H * N + 63) // 64 * 64
    w = saved[off:off + B * H * nb * nb * 32].contiguous().view(torch.int32).view(B * H, nb, nb, 32).to(torch.int64)
    return w & 0xFFFFFFFF


def words_to_keep(w, N):
    """word (kb, qb, j) = bits over the 32 queries of block qb for key kb*32 + j -> keep [B*H][N][N]."""
    BH, nb = w.shape[0], w.shape[1]
    bits = (w[..., None] >> torch.arange(32, device=w.device)) & 1  # [bh][kb][qb][j][qi]
    return bits.permute(0, 2, 4, 1, 3).reshape(BH, nb * 32, nb * 32)[:, :N, :N].bool()


def real_key_words(w, N):
    """Words of real keys (kb*32 + j < N); those of padding keys are unspecified."""
    nb = w.shape[1]
    real = (torch.arange(nb, device=w.device)[:, None] * 32 + torch.arange(32, device=w.device)[None, :]) < N
    return w[real[None, :, None, :].expand_as(w)]


class Run:
    """One forward + backward through the ABI with every guard checked."""

    def __init__(self, dtype, B, N, H, dh, p, qkv_src, dout_src, seed, padded):
        self.dtype, self.dims, self.p, self.seed = dtype, (B, N, H, dh), p, seed
        self.code = 0 if dtype == "bf16" else 1
        self.dt = tdt(dtype)
        self.pad = {k: (v if padded else 0) for k, v in PADS.items()}
        self.thr, self.ds = R.drop_params(p)
        self.scale = R.f32(1.0 / math.sqrt(dh))
        D, rows = H * dh, B * N
        self.D, self.rows = D, rows
        self.qkv, _ = nanview(rows, 3 * D, self.pad["qkv"], self.dt, qkv_src, guard=GUARD)
        self.dout, _ = nanview(rows, D, self.pad["dout"], self.dt, dout_src, guard=GUARD)
        self.n_saved = lib().fer_attention_saved_floats(self.code, B, N, H, dh, self.thr)
        assert self.n_saved >= B * H * N
        nws = lib().fer_attention_ws(self.code, B, N, H)
        assert nws >= 0
        self.ws = torch.empty(max(1, (nws + 3) // 4), dtype=torch.float32, device=DEV)

    def forward(self):
        B, N, H, dh = self.dims
        self.out, self.out_par = nanview(self.rows, self.D, self.pad["out"], self.dt, guard=GUARD)
        self.saved, self.saved_par = nanvec(self.n_saved)
        rc = lib().fer_attention_fwd(self.code, ptr(self.qkv), self.qkv.stride(0), ptr(self.out), self.out.stride(0),
                                     ptr(self.saved), self.n_saved, B, N, H, dh, self.scale, self.thr, self.ds,
                                     self.seed, ptr(self.ws), self.ws.numel() * 4, stream())
        assert rc == 0, last_error()
        torch.cuda.synchronize()
        untouched("attention_fwd out", self.out_par, self.rows, self.D, guard=GUARD)
        untouched_vec("attention_fwd saved", self.saved_par, self.n_saved)
        self.lse = self.saved[:B * H * N]
        assert torch.isfinite(self.lse).all(), "lse not fully written"
        assert not torch.isnan(self.out.float()).any(), "NaN in out"
        return self

    def backward(self, colsum="acc"):
        """colsum: None, "set" (colsum_accumulate = 0 into NaN) or "acc" (1, into a known non-zero vector)."""
        B, N, H, dh = self.dims
        self.dqkv, self.dqkv_par = nanview(self.rows, 3 * self.D, self.pad["dqkv"], self.dt, guard=GUARD)
        self.cs = self.cs_par = self.cs_old = None
        if colsum is not None:
            self.cs, self.cs_par = nanvec(3 * self.D)
            if colsum == "acc":
                self.cs_old = (torch.arange(3 * self.D, device=DEV) % 7 - 3).float() * 0.25 + 0.125
                self.cs.copy_(self.cs_old)
        rc = lib().fer_attention_bwd(self.code, ptr(self.qkv), self.qkv.stride(0), ptr(self.out), self.out.stride(0),
                                     ptr(self.dout), self.dout.stride(0), ptr(self.saved), self.n_saved,
                                     ptr(self.dqkv), self.dqkv.stride(0), ptr(self.ws), self.ws.numel() * 4, B, N, H,
                                     dh, self.scale, self.thr, self.ds, self.seed, ptr(self.cs),
                                     int(colsum == "acc"), stream())
        assert rc == 0, last_error()
        torch.cuda.synchronize()
        untouched("attention_bwd dqkv", self.dqkv_par, self.rows, 3 * self.D, guard=GUARD)
        assert not torch.isnan(self.dqkv.float()).any(), "NaN in dqkv"
        if self.cs is not None:
            untouched_vec("attention_bwd colsum", self.cs_par, 3 * self.D)
            assert not torch.isnan(self.cs).any(), "NaN in colsum"
        return self


def check_run(name, run, r, keep, c, colsum="acc"):
    """Forward check, keep words, then the backward from the kernel's own out and saved state."""
    B, N, H, dh = run.dims
    fam = family(run.dtype, N, dh)
    wf, wb = {}, {}
    run.forward()
    R.check_forward(name, r, run.out, run.lse, c, run.dtype, l_round=0.0, worst=wf)
    if fam == "pers" and run.p > 0:  # the stored keep bits are exactly the hash's
        got = words_to_keep(keep_words(run.saved, B, N, H), N)
        assert torch.equal(got.cpu(), keep.reshape(B * H, N, N).cpu()), f"{name}: stored keep bits differ from the hash"
    run.backward(colsum)
    r.bwd(run.out.float())
    R.check_backward(name, r, run.dqkv, c, run.dtype, worst=wb)
    if run.cs is not None:
        R.check_colsum(name, r, run.cs, run.cs_old, c, run.dtype, sums_rounded=fam in ("gen", "f32"), worst=wb)
    return wf, wb


def note(fam_fwd, fam_bwd, wf, wb):
    for fam, w in ((fam_fwd, wf), (fam_bwd, wb)):
        for k, v in w.items():
            WORST[(fam, k)] = max(WORST.get((fam, k), 0.0), v)


def report():
    for (fam, k), v in sorted(WORST.items()):
        print(f"worst attention {fam} {k} {v:.3f}")


class forced_fwd:
    def __init__(self, k):
        self.k = k

    def __enter__(self):
        assert lib().fer_attention_set_fwd_kernel(self.k) == 0

    def __exit__(self, *a):
        lib().fer_attention_set_fwd_kernel(0)


def same_forward(name, a, b, N):
    assert_bits_equal(f"{name} out", a.out, b.out)
    assert_bits_equal(f"{name} lse", a.lse, b.lse)
    if a.p > 0:
        B, _, H, _ = a.dims
        assert torch.equal(real_key_words(keep_words(a.saved, B, N, H), N),
                           real_key_words(keep_words(b.saved, B, N, H), N)), f"{name}: keep words of real keys differ"


def forward_matches(a, b, N):
    try:
        same_forward("", a, b, N)
        return True
    except AssertionError:
        return False


def run_case(B, N, H, dh, dtype, p, ctab, styles=("normal", "peaked")):
    c = ctab[dtype]
    fam = family(dtype, N, dh)
    auto_done = False
    for style in styles:
        qkv, dout, keep, r, seed = case_ref(B, N, H, dh, style, p)
        for padded in (False, True):
            name = f"{dtype} N={N} H={H} dh={dh} p={p} {style} {'padded' if padded else 'tight'}"
            if fam != "pers":
                wf, wb = check_run(name, Run(dtype, B, N, H, dh, p, qkv, dout, seed, padded), r, keep, c)
                note(fam, fam, wf, wb)
                continue
            runs = {}
            for k in (1, 2):
                with forced_fwd(k):
                    runs[k] = Run(dtype, B, N, H, dh, p, qkv, dout, seed, padded)
                    wf, wb = check_run(f"{name} fwd_kernel={k}", runs[k], r, keep, c)
                note("pers" if k == 1 else "occ", "pers", wf, wb)
            same_forward(f"{name}: persistent vs occupancy form", runs[1], runs[2], N)
            assert_bits_equal(f"{name}: dqkv after either forward", runs[1].dqkv, runs[2].dqkv)
            if not auto_done:  # the automatic selection, once per N: one of the two forms, bit for bit
                auto = Run(dtype, B, N, H, dh, p, qkv, dout, seed, padded).forward()
                assert forward_matches(auto, runs[1], N) or forward_matches(auto, runs[2], N), \
                    f"{name}: the automatic forward equals neither forced form"
                auto_done = True
    report()


# ---------------------------------------------------------------------- the cases
# (N, H, dh, p = 0.5 as well). NB = ceil(N / 32).
PERS = [(1, 2, 64, False), (2, 2, 64, False), (19, 3, 64, False), (32, 2, 64, False),      # NB 1
        (33, 2, 64, False), (64, 3, 64, False),                                              # NB 2
        (65, 2, 64, False), (96, 2, 64, False),                                              # NB 3
        (97, 2, 64, False), (100, 3, 64, True),                                              # NB 4: occupancy form with dropout
        (150, 2, 64, False), (160, 2, 64, False),                                            # NB 5
        (161, 2, 64, False), (192, 2, 64, False),                                            # NB 6: first with the helper wave
        (197, 3, 64, True), (224, 2, 64, False)]                                             # NB 7
WIDTHS = [(N, 3, dh, False) for N in (37, 197) for dh in (8, 16, 24, 40, 56)]
FUSED = [(225, 2, 64, False), (250, 3, 64, True), (256, 2, 64, False),
         (225, 2, 24, False), (250, 2, 24, False), (256, 3, 24, False)]
# GEN_ROWS = 128: N = 256 is a multiple, the others are not
GEN = [(257, 2, 64, True), (300, 2, 128, True), (19, 3, 72, False), (130, 2, 104, False), (37, 3, 96, False),
       (256, 2, 96, False)]
CASES = [(N, H, dh, p) for N, H, dh, half in PERS + WIDTHS + FUSED + GEN for p in ((0.0, 0.1, 0.5) if half else (0.0, 0.1))]


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("N,H,dh,p", CASES)
def test_attention_elementwise(N, H, dh, p, dtype, ctab):
    run_case(2, N, H, dh, dtype, p, ctab)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("N,dh", [(197, 64), (300, 128)])
def test_attention_score_offset(N, dh, dtype, ctab_offset):
    """Scores of a row near +-40 with one key 100 below or above the rest: the running max far from 0, ex2
    flushing below 2^-126, one-hot rows; lse as the accumulator's start value in the persistent backward."""
    run_case(2, N, 2, dh, dtype, 0.1, ctab_offset, styles=("offset",))


@pytest.mark.parametrize("dtype", ["fp32"])
@pytest.mark.parametrize("dh", [5, 20])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_attention_fp32_any_head_width(dh, p, dtype, ctab):
    """The fp32 ABI has no dh % 8 rule. H = 4: the fused bias gradient goes through fer_colsum, which takes
    3*H*dh and ld_dqkv in multiples of 4 only."""
    run_case(2, 37, 4, dh, dtype, p, ctab)


# one shape per backward path
VARIANTS = [("bf16", 100, 2, 64), ("bf16", 197, 2, 64), ("bf16", 250, 2, 64), ("bf16", 300, 2, 128), ("fp32", 37, 2, 64)]


@pytest.mark.parametrize("dtype,N,H,dh", VARIANTS)
def test_attention_backward_variants(dtype, N, H, dh, ctab):
    """colsum = None, colsum_accumulate = 0 into a NaN-filled vector, 1 into a known non-zero one; dqkv is
    the same bits in all three, and a second call reproduces every bit."""
    B, p = 2, 0.1
    qkv, dout, keep, r, seed = case_ref(B, N, H, dh, "peaked", p)
    fam = family(dtype, N, dh)
    res = {}
    for padded in (False, True):
        for mode in (None, "set", "acc"):
            name = f"{dtype} N={N} dh={dh} colsum={mode} {'padded' if padded else 'tight'}"
            run = Run(dtype, B, N, H, dh, p, qkv, dout, seed, padded)
            wf, wb = check_run(name, run, r, keep, ctab[dtype], colsum=mode)
            note(fam, fam, wf, wb)
            first_dqkv = run.dqkv.clone()
            first_cs = None if run.cs is None else run.cs.clone()
            run.backward(mode)
            assert_bits_equal(f"{name}: second backward dqkv", run.dqkv, first_dqkv)
            if first_cs is not None:
                assert_bits_equal(f"{name}: second backward colsum", run.cs, first_cs)
            res[mode] = first_dqkv
        assert_bits_equal("dqkv with and without colsum", res[None], res["set"])
        assert_bits_equal("dqkv with colsum set / accumulated", res["set"], res["acc"])
    report()


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_attention_multi_unit(p, dtype, ctab):
    """More (batch, head) units than workgroups: B*H = 384 units of N = 197 on 256 workgroups, fp64 reference
    on the GPU; under the work queue and under the fixed stride, which must agree bit for bit."""
    B, N, H, dh = 32, 197, 12, 64
    qkv, dout, keep, r, seed = case_ref(B, N, H, dh, "normal", p, DEV)
    runs = []
    try:
        for mode in ((0, 1) if dtype == "bf16" else (0,)):
            assert lib().fer_set_persistent_mode(mode) == 0
            for k in ((1, 2) if dtype == "bf16" else (0,)):
                with forced_fwd(k):
                    run = Run(dtype, B, N, H, dh, p, qkv, dout, seed, padded=(mode == 1))
                    wf, wb = check_run(f"{dtype} multi-unit p={p} mode={mode} fwd_kernel={k}", run, r, keep, ctab[dtype])
                note({0: "f32", 1: "pers", 2: "occ"}[k], family(dtype, N, dh), wf, wb)
                runs.append(run)
    finally:
        lib().fer_set_persistent_mode(0)
    for other in runs[1:]:
        same_forward("multi-unit", runs[0], other, N)
        assert_bits_equal("multi-unit dqkv", runs[0].dqkv, other.dqkv)
        assert_bits_equal("multi-unit colsum", runs[0].cs, other.cs)
    case_ref.cache_clear()  # the one large reference
    report()


def test_attention_rejected_calls():
    """Each returns non-zero, sets its message and leaves NaN-filled outputs bit-identical."""
    B, N, H = 2, 37, 2
    L = lib()

    def attempt(dh, msg_f, msg_b, ld_qkv_extra=0, short_saved=0, dh_alloc=None):
        da = dh_alloc or dh
        D = H * da
        qkv = torch.zeros(B * N, 3 * D + 8, dtype=torch.bfloat16, device=DEV)
        dout = torch.zeros(B * N, D, dtype=torch.bfloat16, device=DEV)
        out = torch.full((B * N, D), NAN, dtype=torch.bfloat16, device=DEV)
        dqkv = torch.full((B * N, 3 * D), NAN, dtype=torch.bfloat16, device=DEV)
        cs = torch.full((3 * D,), NAN, device=DEV)
        n = L.fer_attention_saved_floats(0, B, N, H, da, 6554)
        saved = torch.full((n,), NAN, device=DEV)
        ws = torch.empty(max(1, L.fer_attention_ws(0, B, N, H) // 4), device=DEV)
        ld = 3 * D + ld_qkv_extra
        scale = R.f32(1 / math.sqrt(dh))
        rc = L.fer_attention_fwd(0, ptr(qkv), ld, ptr(out), D, ptr(saved), n - short_saved, B, N, H, dh, scale, 6554,
                                 R.f32(1 / 0.9), 1, ptr(ws), ws.numel() * 4, stream())
        assert rc != 0 and msg_f in last_error(), (rc, last_error())
        rc = L.fer_attention_bwd(0, ptr(qkv), ld, ptr(dout), D, ptr(dout), D, ptr(saved), n - short_saved, ptr(dqkv),
                                 3 * D, ptr(ws), ws.numel() * 4, B, N, H, dh, scale, 6554, R.f32(1 / 0.9), 1, ptr(cs),
                                 0, stream())
        assert rc != 0 and msg_b in last_error(), (rc, last_error())
        torch.cuda.synchronize()
        for name, t in (("out", out), ("dqkv", dqkv), ("colsum", cs), ("saved", saved)):
            assert_bits_equal(f"rejected call wrote {name}", t, torch.full_like(t, NAN))

    dh_msg = "needs dh <= 128, dh % 8 == 0"
    attempt(12, "attention_fwd(bf16): " + dh_msg, "attention_bwd(bf16): " + dh_msg, dh_alloc=16)
    attempt(136, "attention_fwd(bf16): " + dh_msg, "attention_bwd(bf16): " + dh_msg)
    attempt(64, "attention_fwd(bf16): misaligned leading dimension", "attention_bwd(bf16): misaligned ld", ld_qkv_extra=4)
    small = "saved-state buffer smaller than fer_attention_saved_floats()"
    attempt(64, "attention_fwd: " + small, "attention_bwd: " + small, short_saved=1)
