"""Every dropout kernel under a live device step counter (csrc/step_seed.h), DESIGN.md section 2.11.

One identity per case, no numeric reference of its own:

    kernel(host seed s, counter registered and holding c)  ==  kernel(host seed step_seed(s, c), no counter)

bit for bit, on every output (A == B). The right-hand side is the eager path that sections 2.1 to 2.6 hold to
float64 element by element and show bit-reproducible, so the equality carries every bound there over to the path
a replayed fervit.graph.StepGraph runs, backward kernels included; and since both kernels of a dropout site
reduce to the same eager seed, the pairing of section 2.7 carries over too. dropmask.step_seed is the host
replica of the mix (tests/test_step_seed_cpu.py pins it).

Per case also: every output the mask reaches differs from C = kernel(s, no counter) (A != C: the case does drop,
the kernel does read the counter), and the counter tensor holds c after the calls (no kernel writes it).
c in {0, 1, 2^32 + 5}: a registered counter at 0 still mixes, and a 32-bit read of the counter fails the third.

CASES lists one case per kernel and instantiation that has a step_seed( call; SITE_KERNELS names the kernel
around each call in file order, and tests/test_step_seed_cpu.py checks both against the sources. Whoever adds a
call site adds its kernel there and a case here. A backward case runs its own forward first, under the same
counter and seed, for the tensors it needs."""
import collections
import math

import pytest
import torch

from dropmask import step_seed
from elemwise import assert_bits_equal
from fervit import ops
from fervit._lib import check, lib

DEV = "cuda"
P = 0.5
SEED = 0xC3A5_1F0E_9D27_64B1  # the one host seed: high and low word both non-zero
COUNTERS = (0, 1, 2 ** 32 + 5)
BF16, F32 = torch.bfloat16, torch.float32
DT = {"bf16": BF16, "fp32": F32}

# step_seed( occurrences per csrc/*.hip
SITES = {"gemm.hip": 6, "attention.hip": 10, "vit_edge.hip": 8, "layernorm.hip": 2, "convbn.hip": 2, "conv2d.hip": 2,
         "wplus.hip": 2, "optim.hip": 1, "attnpool.hip": 1}
# the __global__ function around each occurrence, in file order; a kernel with several is numbered
# (gemm_8ph_kernel: #1 the fixed-stride form, #2 the work-queue form)
SITE_KERNELS = {
    "gemm.hip": ["gemm_bf16_kernel", "gemm_ring_kernel", "gemm_8ph_kernel#1", "gemm_8ph_kernel#2",
                 "splitk_reduce_kernel", "gemm_f32_kernel"],
    "attention.hip": ["attn_fwd_bf16", "attn_fwd_pers", "attn_fwd_occ", "attn_bwd_fused_bf16", "attn_fwd_gen",
                      "attn_dq_gen", "attn_dkv_gen", "attn_f32_pv", "attn_f32_ds", "attn_f32_grads"],
    "layernorm.hip": ["ln_bwd_kernel", "ln_bwd8_kernel"],
    "vit_edge.hip": ["tokens_fwd4_kernel", "tokens_fwd8_kernel", "tokens_fwd_kernel", "tokens_bwd_kernel",
                     "tokens_bwd4_kernel", "tokens_bwd8_kernel", "head_fwd_kernel", "head_bwd_kernel"],
    "convbn.hip": ["bn_fwd_kernel", "bn_bwd_kernel"],
    "conv2d.hip": ["pool2_chdrop_fwd_kernel", "pool2_chdrop_bwd_kernel"],
    "wplus.hip": ["latent_augment_kernel", "latent_dir_draw_kernel"],
    "optim.hip": ["dropout_kernel"],
    "attnpool.hip": ["relu_dropout_kernel"],
}

# name -> (file, the SITE_KERNELS entries the case runs, factory). factory() -> run(seed) -> (masked, fixed):
# two dicts of outputs, those the keep mask reaches and those it does not (lse, statistics, an undropped dx).
Case = collections.namedtuple("Case", "file sites make")
CASES = {}


def case(name, file, *sites):
    def deco(make):
        assert name not in CASES, name
        CASES[name] = Case(file, sites, make)
        return make
    return deco


def rnd(*shape, dtype=F32, salt=0, scale=1.0):
    g = torch.Generator().manual_seed(977 + salt)
    return (torch.randn(*shape, generator=g) * scale).to(DEV, dtype)


def nan(*shape, dtype=F32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


class forced_persistent_mode:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        check(lib().fer_set_persistent_mode(self.mode), "set_persistent_mode")

    def __exit__(self, *exc):
        lib().fer_set_persistent_mode(0)


# ---------------------------------------------------------------------- csrc/gemm.hip
# bf16: M = 264, N = 136, K = 200 (tests/test_gpu_gemm_elementwise.py RAGGED: partial in M, N and K for every tile,
# more than one tile); fp32: 65 x 132 x 33; split-K: 136 x 72, K = 1032
GEMM_KINDS = {
    "drop": dict(),  # store + dropout: the generic epilogue
    "gate": dict(bias=True, act="gelu", pre="gate"),  # EPI_GATE: c and pre both masked
    "res": dict(bias=True, res=True),  # EPI_RES / EPI_RES2 (out-proj and fc2 forward)
    "gen": dict(bias=True, act="gelu", pre="plain", res=True, drop_extra=8),  # generic, drop_ld = N + 8
}


def gemm_run(M, N, K, dtype, kind, cfg=-1, mode=None, split=False, small_ws=False):
    from test_gpu_gemm_elementwise import forced_config, raw_gemm

    o = dict(dict(bias=False, act="none", pre=None, res=False, drop_extra=0), **GEMM_KINDS[kind])
    a, b = rnd(M, K, dtype=dtype), rnd(N, K, dtype=dtype, salt=1, scale=1 / math.sqrt(K))
    bias = rnd(N, salt=2) if o["bias"] else None
    res = rnd(M, N, dtype=dtype, salt=3) if o["res"] else None
    thr, dscale = ops.drop_args(P)

    def run(seed):
        c = nan(M, N, dtype=dtype)
        pre = nan(M, N, dtype=dtype) if o["pre"] else None
        with forced_config(cfg), forced_persistent_mode(mode or 0):
            if small_ws:  # the ABI with a workspace of 4 M N bytes: too small for two splits
                ws = torch.empty(M * N, dtype=F32, device=DEV)
                rc = raw_gemm(dtype=ops.dcode(a), A=a, lda=K, a_kc=1, B=b, ldb=K, b_kc=1, M=M, N=N, K=K, ws=ws, c=c,
                              ldc=N, bias=bias, act=ops.ACT[o["act"]], res=res, ldr=N, drop_thresh=thr,
                              drop_scale=dscale, seed=seed, drop_ld=N + o["drop_extra"])
                assert rc == 0, lib().fer_last_error().decode()
            else:
                ops.gemm(a, b, c, M=M, N=N, K=K, bias=bias, act=o["act"], pre=pre, res=res, dropout=P, seed=seed,
                         drop_ld=N + o["drop_extra"], pre_gate=o["pre"] == "gate", split_ws=split, ws_exact=split)
        masked, fixed = {"c": c}, {}
        if pre is not None:
            (masked if o["pre"] == "gate" else fixed)["pre"] = pre
        return masked, fixed
    return run


RAGGED = (264, 136, 200)
for _cfg, _site in ((3, "gemm_bf16_kernel"), (5, "gemm_ring_kernel"), (8, "gemm_8ph_kernel#2"), (11, "gemm_bf16_kernel")):
    for _kind in GEMM_KINDS:
        case(f"gemm-cfg{_cfg}-{_kind}", "gemm.hip", _site)(
            lambda cfg=_cfg, kind=_kind: gemm_run(*RAGGED, BF16, kind, cfg=cfg))
for _kind in GEMM_KINDS:  # fer_set_persistent_mode(1): the 8-phase kernel on the fixed stride
    case(f"gemm-cfg8-fixed-stride-{_kind}", "gemm.hip", "gemm_8ph_kernel#1")(
        lambda kind=_kind: gemm_run(*RAGGED, BF16, kind, cfg=8, mode=1))
    case(f"gemm-fp32-{_kind}", "gemm.hip", "gemm_f32_kernel")(lambda kind=_kind: gemm_run(65, 132, 33, F32, kind))
case("gemm-split-k-res", "gemm.hip", "splitk_reduce_kernel")(lambda: gemm_run(136, 72, 1032, BF16, "res", split=True))
case("gemm-split-k-small-ws-res", "gemm.hip", "gemm_bf16_kernel")(
    lambda: gemm_run(136, 72, 1032, BF16, "res", small_ws=True))


# ---------------------------------------------------------------------- csrc/attention.hip
def attention_run(dtype, N, H, dh, fwd_kernel=0, B=2):
    from test_gpu_attention_elementwise import forced_fwd, keep_words, real_key_words

    D = H * dh
    qkv, dout = rnd(B * N, 3 * D, dtype=dtype), rnd(B * N, D, dtype=dtype, salt=1)
    pers = dtype == BF16 and N <= 224 and dh <= 64  # the family that stores its keep words

    def run(seed):
        with forced_fwd(fwd_kernel):
            saved = ops.attention_saved(qkv, B, N, H, dh, dropout=P).fill_(float("nan"))
            out = ops.attention_fwd(qkv, nan(B * N, D, dtype=dtype), saved, B, N, H, dh, dropout=P, seed=seed)
            cs = nan(3 * D)
            dqkv = ops.attention_bwd(qkv, out, dout, saved, nan(B * N, 3 * D, dtype=dtype), B, N, H, dh, dropout=P,
                                     seed=seed, colsum=cs)
        masked = {"out": out, "dqkv": dqkv, "colsum": cs}
        if pers:
            masked["keep words of real keys"] = real_key_words(keep_words(saved, B, N, H), N).to(torch.int32)
        return masked, {"lse": saved[:B * H * N]}
    return run


case("attention-bf16-N100-persistent", "attention.hip", "attn_fwd_pers")(lambda: attention_run(BF16, 100, 2, 64, 1))
case("attention-bf16-N100-occupancy", "attention.hip", "attn_fwd_occ")(lambda: attention_run(BF16, 100, 2, 64, 2))
# N = 197: seven key blocks, the persistent form with its helper wave; the automatic choice there is the occupancy form
case("attention-bf16-N197-persistent", "attention.hip", "attn_fwd_pers")(lambda: attention_run(BF16, 197, 2, 64, 1))
case("attention-bf16-N197-automatic", "attention.hip", "attn_fwd_occ")(lambda: attention_run(BF16, 197, 2, 64))
case("attention-bf16-N37-dh24", "attention.hip", "attn_fwd_pers")(lambda: attention_run(BF16, 37, 3, 24))
case("attention-bf16-N250-fused", "attention.hip", "attn_fwd_bf16", "attn_bwd_fused_bf16")(
    lambda: attention_run(BF16, 250, 2, 64))
case("attention-bf16-N300-dh128-general", "attention.hip", "attn_fwd_gen", "attn_dq_gen", "attn_dkv_gen")(
    lambda: attention_run(BF16, 300, 2, 128))
case("attention-fp32-N37", "attention.hip", "attn_f32_pv", "attn_f32_ds", "attn_f32_grads")(
    lambda: attention_run(F32, 37, 2, 64))


# ---------------------------------------------------------------------- csrc/layernorm.hip
def layernorm_run(dtype, D, M=17):
    x, dy, res = rnd(M, D, dtype=dtype), rnd(M, D, dtype=dtype, salt=1), rnd(M, D, dtype=dtype, salt=2)
    w, b = 1.0 + 0.1 * rnd(D, salt=3), rnd(D, salt=4)
    mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    ops.layernorm_fwd(x, w, b, 1e-5, mean=mean, rstd=rstd)

    def run(seed):
        dxd, dg, db = nan(M, D, dtype=dtype), nan(D), nan(D)
        dx = ops.layernorm_bwd(dy, x, mean, rstd, w, dx=nan(M, D, dtype=dtype), res=res, dx_drop=dxd, dropout=P,
                               seed=seed, dgamma=dg, dbeta=db)
        return {"dx_drop": dxd}, {"dx": dx, "dgamma": dg, "dbeta": db}
    return run


case("layernorm_bwd-fp32-D64", "layernorm.hip", "ln_bwd_kernel")(lambda: layernorm_run(F32, 64))
case("layernorm_bwd-bf16-D12", "layernorm.hip", "ln_bwd_kernel")(lambda: layernorm_run(BF16, 12))  # D % 8 != 0
case("layernorm_bwd-bf16-D64", "layernorm.hip", "ln_bwd8_kernel")(lambda: layernorm_run(BF16, 64))


# ---------------------------------------------------------------------- csrc/vit_edge.hip
def tokens_run(dtype, D, B=8, n=7):
    emb, cls, pos = rnd(B * n, D, dtype=dtype), rnd(D, salt=1), rnd((n + 1) * D, salt=2)
    dt = rnd(B * (n + 1), D, dtype=dtype, salt=3)

    def run(seed):
        t = ops.tokens_fwd(emb, cls, pos, B, n, D, dropout=P, seed=seed)
        dcls, dpos = nan(D), nan((n + 1) * D)
        demb = ops.tokens_bwd(dt, B, n, D, dcls, dpos, False, dropout=P, seed=seed)
        return {"t": t, "demb": demb, "dcls": dcls, "dpos": dpos}, {}
    return run


# the widths of tests/test_gpu_edge_kernels.py: bf16 with D % 8 == 0 is 8-wide, D % 4 == 0 otherwise 4-wide, D = 6 scalar
case("tokens-bf16-D64-8wide", "vit_edge.hip", "tokens_fwd8_kernel", "tokens_bwd8_kernel")(lambda: tokens_run(BF16, 64))
case("tokens-bf16-D12-4wide", "vit_edge.hip", "tokens_fwd4_kernel", "tokens_bwd4_kernel")(lambda: tokens_run(BF16, 12))
case("tokens-fp32-D64-4wide", "vit_edge.hip", "tokens_fwd4_kernel", "tokens_bwd4_kernel")(lambda: tokens_run(F32, 64))
case("tokens-bf16-D6-scalar", "vit_edge.hip", "tokens_fwd_kernel", "tokens_bwd_kernel")(lambda: tokens_run(BF16, 6))
case("tokens-fp32-D6-scalar", "vit_edge.hip", "tokens_fwd_kernel", "tokens_bwd_kernel")(lambda: tokens_run(F32, 6))


def head_run(dtype, B=3, N=5, D=64, C=7):
    t = rnd(B * N, D, dtype=dtype)
    lnw, lnb, W, b = 1.0 + 0.1 * rnd(D, salt=1), rnd(D, salt=2), rnd(C, D, salt=3, scale=0.125), rnd(C, salt=4)
    dlogits = rnd(B, C, salt=5)

    def run(seed):
        logits, stats = ops.head_fwd(t, N, lnw, lnb, 1e-5, W, b, B, dropout=P, seed=seed)
        grads = [nan(D), nan(D), nan(C, D), nan(C)]
        dt = ops.head_bwd(t, N, lnw, lnb, W, stats, dlogits, B, grads, False, dropout=P, seed=seed)
        return ({"logits": logits, "dt": dt, "dln_w": grads[0], "dln_b": grads[1], "dW": grads[2]},
                {"stats": stats, "dbias": grads[3]})
    return run


case("head-bf16", "vit_edge.hip", "head_fwd_kernel", "head_bwd_kernel")(lambda: head_run(BF16))
case("head-fp32", "vit_edge.hip", "head_fwd_kernel", "head_bwd_kernel")(lambda: head_run(F32))


# ---------------------------------------------------------------------- csrc/convbn.hip, attnpool.hip, conv2d.hip
def batchnorm_run(dtype, with_res, M=37, C=24):
    x, dy = rnd(M, C, dtype=dtype), rnd(M, C, dtype=dtype, salt=1)
    res = rnd(M, C, dtype=dtype, salt=2) if with_res else None
    gamma, beta = 1.0 + 0.1 * rnd(C, salt=3), rnd(C, salt=4)

    def run(seed):
        rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        nbt = torch.zeros((), dtype=torch.int64, device=DEV)
        y, mean, rstd = ops.batchnorm_fwd(x, gamma, beta, rm, rv, nbt, True, res=res, relu=True, dropout=P, seed=seed)
        dg, db = nan(C), nan(C)
        dx, dres = ops.batchnorm_bwd(dy, x, mean, rstd, gamma, beta, True, res=res, relu=True, dropout=P, seed=seed,
                                     dres=nan(M, C, dtype=dtype) if with_res else None, dgamma=dg, dbeta=db)
        masked = {"y": y, "dx": dx, "dgamma": dg, "dbeta": db}
        if with_res:
            masked["dres"] = dres
        return masked, {"mean": mean, "rstd": rstd, "running_mean": rm, "running_var": rv}
    return run


def relu_dropout_run(dtype, M=37, C=24):
    x, dy = rnd(M, C, dtype=dtype), rnd(M, C, dtype=dtype, salt=1)

    def run(seed):
        return {"y": ops.relu_dropout_fwd(x, dropout=P, seed=seed),
                "dx": ops.relu_dropout_bwd(dy, x, dropout=P, seed=seed)}, {}
    return run


def pool2_chdrop_run(dtype, B=2, H=8, W=8, C=24):
    x, dy = rnd(B * H * W, C, dtype=dtype), rnd(B * (H // 2) * (W // 2), C, dtype=dtype, salt=1)

    def run(seed):
        return {"y": ops.pool2_chdrop_fwd(x, B, H, W, True, dropout=P, seed=seed),
                "dx": ops.pool2_chdrop_bwd(dy, x, B, H, W, True, dropout=P, seed=seed)}, {}
    return run


for _d in DT:
    for _r in (False, True):
        case(f"batchnorm-{_d}-{'res' if _r else 'nores'}", "convbn.hip", "bn_fwd_kernel", "bn_bwd_kernel")(
            lambda d=_d, r=_r: batchnorm_run(DT[d], r))
    case(f"relu_dropout-{_d}", "attnpool.hip", "relu_dropout_kernel")(lambda d=_d: relu_dropout_run(DT[d]))
    case(f"pool2_chdrop-{_d}", "conv2d.hip", "pool2_chdrop_fwd_kernel", "pool2_chdrop_bwd_kernel")(
        lambda d=_d: pool2_chdrop_run(DT[d]))


# ---------------------------------------------------------------------- csrc/optim.hip, wplus.hip
def dropout_run(dtype, n=1003):  # no multiple of 2, 4 or 8
    x = rnd(n, dtype=dtype)
    return lambda seed: ({"y": ops.dropout(x, P, seed)}, {})


for _d in DT:
    case(f"dropout-{_d}", "optim.hip", "dropout_kernel")(lambda d=_d: dropout_run(DT[d]))


@case("latent_augment", "wplus.hip", "latent_augment_kernel")
def latent_augment_run(B=5, LD=77):
    """Noise, per-sample scale and mask all on: an element the mask keeps carries the noise and scale draws, so
    all three sub-streams must derive from the mixed seed; the zero pattern is the mask stream alone."""
    x = rnd(B, LD)

    def run(seed):
        y = x.clone()
        check(lib().fer_latent_augment(y.data_ptr(), B, LD, 0.25, 0.5, 1.5, P, ops.seed64(seed), ops.stream()),
              "latent_augment")
        return {"y": y, "zeroed": (y == 0).to(torch.int32)}, {}
    return run


@case("latent_dir_draw", "wplus.hip", "latent_dir_draw_kernel")
def latent_dir_draw_run(n=1003):
    return lambda seed: ({"choice": ops.latent_dir_draw(n, 12, 0.25, seed)}, {})


# ---------------------------------------------------------------------- the test
def same_bits(a, b):
    try:
        assert_bits_equal("", a, b)
        return True
    except AssertionError:
        return False


@pytest.mark.gpu
@pytest.mark.parametrize("c", COUNTERS, ids=lambda c: f"c{c}")
@pytest.mark.parametrize("name", list(CASES))
def test_counter_path_is_the_eager_path_at_the_mixed_seed(name, c):
    run = CASES[name].make()
    counter = torch.tensor([c], dtype=torch.int64, device=DEV)  # the ABI's uint64_t
    try:
        check(lib().fer_set_step_counter(counter.data_ptr()), "set_step_counter")
        a_masked, a_fixed = run(SEED)
        torch.cuda.synchronize()
        held = int(counter.item())
        check(lib().fer_set_step_counter(None), "set_step_counter")
        b_masked, b_fixed = run(step_seed(SEED, c))
        c_masked, c_fixed = run(SEED)
    finally:
        check(lib().fer_set_step_counter(None), "set_step_counter")
        torch.cuda.synchronize()
    assert held == c, f"{name}: the counter holds {held} after the call, {c} before"
    assert a_masked and a_masked.keys() == b_masked.keys() and a_fixed.keys() == b_fixed.keys()
    for k, v in {**a_masked, **a_fixed}.items():
        assert not torch.isnan(v.float()).any().item(), f"{name} {k}: NaN (not fully written)"
        assert_bits_equal(f"{name} {k}: seed s under counter {c} against seed step_seed(s, {c}) without a counter",
                          v, {**b_masked, **b_fixed}[k])
    for k, v in a_masked.items():
        assert not same_bits(v, c_masked[k]), f"{name} {k}: counter {c} gives the bits of the unmixed seed"
    for k, v in a_fixed.items():
        assert_bits_equal(f"{name} {k}: an output no mask reaches", v, c_fixed[k])
