"""Float64 reference of the composed layers and the host replica of their dropout seeds and masks (DESIGN.md
section 2.7), shared by tests/test_gpu_layers_elementwise.py (the modules on the GPU) and
tests/test_layer_bound_cpu.py (a torch emulation of the bf16 path and its wrong variants, no GPU).

Every layer is ONE plain torch formula of its reference module; gradients come from torch.autograd. The formula
is evaluated through a `Numerics`: float64 (the reference), float32 torch (`emulate("fp32")`, the measurement of
c_fp32) or a bf16 emulation (`emulate("bf16")`): matrix operands are the bf16 shadow of the weights and every
tensor the native layer materialises in bf16, forward or backward, is rounded to bf16 where it is materialised
(`mat`: the forward value, `gmat`: the gradient that arrives at that point).

Masks are constant tensors holding 0 or 1/(1-p), built from tests/dropmask.py with the element-index
conventions the kernel tests pin: attention probabilities tests/attention_ref.py `attn_keep`, GEMM epilogues
`keep_mask(seed, (M, drop_ld))[:, :N]` (tests/test_gpu_gemm_elementwise.py), tokens the flat token tensor
(tests/test_gpu_edge_kernels.py). Seeds come from a private fervit.runtime._Seeds, never the global stream."""
import functools
import math
from dataclasses import dataclass
from typing import Tuple

import torch

from attention_ref import attn_keep
from dropmask import keep_mask, keep_mask_torch, step_seed
from elemwise import BF_ROUND, assert_close, measure_c
from fervit import runtime

F64 = torch.float64
GOLDEN = 0x9E3779B97F4A7C15


# ---------------------------------------------------------------------- seeds and masks
def site_seeds(seed, n):
    """The first n values fervit.runtime.next_seed() yields after fervit.manual_seed(seed)."""
    s = runtime._Seeds()
    s.base = (int(seed) * GOLDEN) & 0xFFFFFFFFFFFFFFFF
    return [s.next() for _ in range(n)]


def _keep(seed, shape, p, device):
    if str(device).startswith("cuda"):
        return keep_mask_torch(seed, shape, p, device=device)
    return keep_mask(seed, shape, p)


def epilogue_mask(seed, M, N, p, device="cpu", drop_ld=None):
    """GEMM epilogue / LayerNorm-backward dropout of an [M][N] tensor: element index row * drop_ld + col."""
    ld = N if drop_ld is None else drop_ld
    return _keep(seed, (M, ld), p, device)[:, :N].to(F64) / (1.0 - p)


def layer_masks(seeds, B, N, D, H, F, p, device="cpu"):
    """The four sites of a post-norm layer, in the order they draw: attention, out-proj, fc1, fc2."""
    if p <= 0:
        return {}
    M = B * N
    return {"attn": attn_keep(seeds[0], B, N, H, p, device=device).to(F64) / (1.0 - p),
            "out": epilogue_mask(seeds[1], M, D, p, device).view(B, N, D),
            "fc1": epilogue_mask(seeds[2], M, F, p, device).view(B, N, F),
            "fc2": epilogue_mask(seeds[3], M, D, p, device).view(B, N, D)}


def tokens_mask(seed, B, N, D, p, device="cpu"):
    return _keep(seed, (B * N * D,), p, device).view(B, N, D).to(F64) / (1.0 - p)


def keep_rates(masks):
    return {k: (m > 0).double().mean().item() for k, m in masks.items()}


# ---------------------------------------------------------------------- numerics
def bf_round(t):
    return t.to(torch.bfloat16).to(t.dtype)


class _RoundFwd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t):
        return bf_round(t)

    @staticmethod
    def backward(ctx, g):
        return g


class _RoundBwd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t):
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        return bf_round(g)


class _MaskMul(torch.autograd.Function):
    """t * fwd going forward, g * bwd coming back: the two kernels of one dropout site."""

    @staticmethod
    def forward(ctx, t, fwd, bwd):
        ctx.save_for_backward(bwd)
        return t * fwd

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0], None, None


class Numerics:
    """How a formula is evaluated: "f64", "f32" or "bf16" (see the module doc). `residual` and `gate` are the
    two places where a formula hands a sub-expression over whole, so that tests/test_layer_bound_cpu.py can
    derive wrong variants without a second copy of the formula; here they do nothing."""

    def __init__(self, kind):
        assert kind in ("f64", "f32", "bf16"), kind
        self.kind = kind
        self.bf = kind == "bf16"
        self.dt = F64 if kind == "f64" else torch.float32

    def leaf(self, t, grad=True):
        return t.detach().to(self.dt).clone().requires_grad_(grad)

    def w(self, W):
        """Matrix operand of a GEMM: the bf16 shadow on the bf16 path, else the master weight."""
        return _RoundFwd.apply(W) if self.bf else W

    def mat(self, t):
        return _RoundFwd.apply(t) if self.bf else t

    def gmat(self, t):
        return _RoundBwd.apply(t) if self.bf else t

    def drop(self, t, m):
        """m: None, a scaled mask, or (forward mask, backward mask)."""
        if m is None:
            return t
        if isinstance(m, tuple):
            return _MaskMul.apply(t, m[0].to(t.dtype), m[1].to(t.dtype))
        return t * m.to(t.dtype)

    def residual(self, t, site):
        return t

    def gate(self, lin, b, fn, site):
        return fn(lin + b)


REF = Numerics("f64")


def emulate(dtype):
    """Numerics of the native path in `dtype`: float32 torch for "fp32", the bf16 emulation for "bf16"."""
    return Numerics({"fp32": "f32", "bf16": "bf16"}[dtype])


# ---------------------------------------------------------------------- formulas
def _ln(t, w, b, eps):
    mu = t.mean(-1, keepdim=True)
    var = ((t - mu) ** 2).mean(-1, keepdim=True)
    return (t - mu) * torch.rsqrt(var + eps) * w + b


def _act(t, act):
    if act == "gelu":
        return 0.5 * t * (1.0 + torch.erf(t / math.sqrt(2.0)))
    assert act == "relu", act
    return torch.relu(t)


def _attention(qkv, H, mask, num):
    """softmax(q k^T / sqrt(dh)) [dropout] v over packed qkv [B][N][3 D] (q | k | v, heads inside each)."""
    B, N, D3 = qkv.shape
    D = D3 // 3
    q, k, v = qkv.view(B, N, 3, H, D // H).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) / math.sqrt(D // H)
    P = num.mat(num.drop(torch.softmax(s, -1), mask))
    return (P @ v).permute(0, 2, 1, 3).reshape(B, N, D)


def post_norm_layer(x, P, masks, p, act, eps, H, num=REF, pre=""):
    """nn.TransformerEncoderLayer(norm_first=False): x1 = LN1(x + drop(out_proj(attn(x)))),
    out = LN2(x1 + drop(lin2(drop(act(lin1 x1))))), dropout on the attention probabilities too. x [B][N][D];
    P maps EncoderLayer's parameter names (prefixed `pre`) to tensors; masks from layer_masks (ignored at p = 0)."""
    m = masks if p > 0 else {}
    g = lambda k: P[pre + k]  # noqa: E731
    x = num.gmat(x)  # dx
    qkv = num.gmat(num.mat(x @ num.w(g("self_attn.in_proj_weight")).t() + g("self_attn.in_proj_bias")))  # dqkv
    o = num.gmat(num.mat(_attention(qkv, H, m.get("attn"), num)))  # do
    a = num.gmat(o @ num.w(g("self_attn.out_proj.weight")).t() + g("self_attn.out_proj.bias"))  # dhh
    y = num.gmat(num.mat(num.residual(x, "attn") + num.drop(a, m.get("out"))))  # dy
    x1 = num.gmat(num.mat(_ln(y, g("norm1.weight"), g("norm1.bias"), eps)))  # dx1

    def ffn_in(t):
        return num.drop(_act(num.gmat(t), act), m.get("fc1"))  # gmat: dF

    f = num.mat(num.gate(x1 @ num.w(g("linear1.weight")).t(), g("linear1.bias"), ffn_in, "fc1"))
    u = num.gmat(f @ num.w(g("linear2.weight")).t() + g("linear2.bias"))  # dh2
    z = num.gmat(num.mat(num.residual(x1, "ffn") + num.drop(u, m.get("fc2"))))  # dz
    return num.mat(_ln(z, g("norm2.weight"), g("norm2.bias"), eps))


def pre_norm_block(x, P, eps, H, num=REF):
    """timm Block: x2 = x + proj(attn(LN1 x)); out = x2 + fc2(gelu(fc1(LN2 x2))). P: Block's parameter names."""
    x = num.gmat(x)
    h1 = num.gmat(num.mat(_ln(x, P["norm1.weight"], P["norm1.bias"], eps)))
    qkv = num.gmat(num.mat(h1 @ num.w(P["attn.qkv.weight"]).t() + P["attn.qkv.bias"]))
    o = num.gmat(num.mat(_attention(qkv, H, None, num)))
    x2 = num.gmat(num.mat(num.residual(x, "attn") + o @ num.w(P["attn.proj.weight"]).t() + P["attn.proj.bias"]))
    h2 = num.gmat(num.mat(_ln(x2, P["norm2.weight"], P["norm2.bias"], eps)))
    f = num.mat(num.gate(h2 @ num.w(P["mlp.fc1.weight"]).t(), P["mlp.fc1.bias"],
                         lambda t: _act(num.gmat(t), "gelu"), "fc1"))
    return num.mat(num.residual(x2, "ffn") + f @ num.w(P["mlp.fc2.weight"]).t() + P["mlp.fc2.bias"])


def adapter(x, P, num=REF):
    """AdapterModule: x + alpha * fc2(gelu(fc1 x)). P: AdapterModule's parameter names."""
    x = num.gmat(x)
    v = num.mat(num.gate(x @ num.w(P["adapter.0.weight"]).t(), P["adapter.0.bias"],
                         lambda t: _act(num.gmat(t), "gelu"), "fc1"))
    T = num.mat(v @ num.w(P["adapter.2.weight"]).t() + P["adapter.2.bias"])
    return num.mat(num.residual(x, "adapter") + P["alpha"] * T)


def patch_tokens(img, P, mask, p, patch, num=REF):
    """Conv2d(C, D, k = s = patch) as a GEMM over patches, CLS in front, + positions, dropout. img [B][C][H][W];
    P: ImageViT's parameter names."""
    B, C, Hh, Ww = img.shape
    gh, gw = Hh // patch, Ww // patch
    W = P["patch_embed.proj.weight"]
    D = W.shape[0]
    cols = img[:, :, :gh * patch, :gw * patch].reshape(B, C, gh, patch, gw, patch).permute(0, 2, 4, 1, 3, 5)
    cols = num.mat(cols.reshape(B, gh * gw, C * patch * patch))
    emb = num.gmat(num.mat(cols @ num.w(W.reshape(D, -1)).t() + P["patch_embed.proj.bias"]))  # demb
    t = torch.cat([P["cls_token"].expand(B, 1, D), emb], 1) + P["pos_embed"]
    return num.mat(num.drop(t, mask if p > 0 else None))


def head(t, P, eps, num=REF):
    """LayerNorm of the CLS rows, Linear (fp32 weights on every path, fp32 logits)."""
    c = _ln(num.gmat(t)[:, 0], P["norm.weight"], P["norm.bias"], eps)
    return c @ P["head.weight"].t() + P["head.bias"]


def image_vit(img, P, masks, p, patch, H, depth, num=REF, eps=1e-5):
    """patch_tokens -> depth x post_norm_layer -> head. masks: [tokens mask, layer_masks of layer 0, ...]."""
    t = patch_tokens(img, P, masks[0] if p > 0 else None, p, patch, num)
    for i in range(depth):
        t = post_norm_layer(t, P, masks[1 + i] if p > 0 else {}, p, "gelu", eps, H, num, pre=f"transformer.layers.{i}.")
    return head(t, P, eps, num)


# ---------------------------------------------------------------------- cases
POST_NORM_PARAMS = lambda D, F: {  # noqa: E731
    "self_attn.in_proj_weight": (3 * D, D), "self_attn.in_proj_bias": (3 * D,), "self_attn.out_proj.weight": (D, D),
    "self_attn.out_proj.bias": (D,), "linear1.weight": (F, D), "linear1.bias": (F,), "linear2.weight": (D, F),
    "linear2.bias": (D,), "norm1.weight": (D,), "norm1.bias": (D,), "norm2.weight": (D,), "norm2.bias": (D,)}
PRE_NORM_PARAMS = lambda D, F: {  # noqa: E731
    "norm1.weight": (D,), "norm1.bias": (D,), "attn.qkv.weight": (3 * D, D), "attn.qkv.bias": (3 * D,),
    "attn.proj.weight": (D, D), "attn.proj.bias": (D,), "norm2.weight": (D,), "norm2.bias": (D,),
    "mlp.fc1.weight": (F, D), "mlp.fc1.bias": (F,), "mlp.fc2.weight": (D, F), "mlp.fc2.bias": (D,)}
ADAPTER_PARAMS = lambda D, A: {  # noqa: E731
    "adapter.0.weight": (A, D), "adapter.0.bias": (A,), "adapter.2.weight": (D, A), "adapter.2.bias": (D,),
    "alpha": (1,)}
# packed q | k | v biases: the key third's true gradient is 0 (softmax is invariant to a shift of a row's scores)
KEY_BIAS = ("self_attn.in_proj_bias", "attn.qkv.bias")


def image_vit_params(C, patch, D, F, n_tok, depth, classes):
    s = {"cls_token": (1, 1, D), "pos_embed": (1, n_tok, D), "patch_embed.proj.weight": (D, C, patch, patch),
         "patch_embed.proj.bias": (D,)}
    for i in range(depth):
        s.update({f"transformer.layers.{i}.{k}": v for k, v in POST_NORM_PARAMS(D, F).items()})
    s.update({"norm.weight": (D,), "norm.bias": (D,), "head.weight": (classes, D), "head.bias": (classes,)})
    return s


def make_params(shapes, gen):
    """Non-trivial values: matrices randn / sqrt(fan_in), LayerNorm weights 1 + 0.1 randn, every bias, CLS and
    position 0.1 .. 0.2 randn."""
    P = {}
    for k, s in shapes.items():
        r = torch.randn(*s, generator=gen)
        if k.endswith("alpha"):
            P[k] = torch.full(s, 0.37)
        elif len(s) >= 2 and k.endswith("weight"):
            P[k] = r / math.sqrt(math.prod(s[1:]))
        elif "norm" in k and k.endswith("weight"):
            P[k] = 1.0 + 0.1 * r
        elif k in ("cls_token", "pos_embed"):
            P[k] = 0.2 * r
        else:
            P[k] = 0.1 * r
    return P


@dataclass(frozen=True)
class Case:
    """One run of one layer kind. `seed`: what fervit.manual_seed gets before the first forward; `passes`: forward
    + backward runs without reseeding (gradients add up)."""
    kind: str  # post_norm | pre_norm | adapter | image_vit
    B: int
    N: int
    D: int
    H: int
    F: int
    act: str = "gelu"
    p: float = 0.0
    seed: int = 1
    passes: int = 1
    alpha: float = 0.37
    dtypes: Tuple[str, ...] = ("fp32", "bf16")

    @property
    def id(self):
        s = f"{self.kind}-B{self.B}N{self.N}D{self.D}H{self.H}F{self.F}-{self.act}-p{self.p}-s{self.seed}"
        s += f"-x{self.passes}" if self.passes > 1 else ""
        return s + (f"-a{self.alpha}" if self.kind == "adapter" else "")


SMALL = [(5, 19, 96, 4, 192), (7, 37, 96, 4, 192)]
VITB = (2, 197, 768, 12, 3072)
POST_NORM_CASES = (
    [Case("post_norm", *s, act=a, p=0.1, seed=3 + i) for i, s in enumerate(SMALL) for a in ("gelu", "relu")]
    + [Case("post_norm", *VITB, act="gelu", p=0.1, seed=5, dtypes=("bf16",))]
    + [Case("post_norm", *SMALL[1], act="gelu", p=0.0)]  # p = 0 in train mode, and eval mode
    + [Case("post_norm", *SMALL[1], act="gelu", p=0.5, seed=6)]
    + [Case("post_norm", *SMALL[0], act="gelu", p=0.1, seed=7, passes=2)])
PRE_NORM_CASES = [Case("pre_norm", *s) for s in SMALL]
ADAPTER_CASES = [Case("adapter", B, N, D, 1, 24, alpha=al) for B, N, D, _, _ in SMALL for al in (0.37, 0.0)]
# ImageViT(img_size=48, patch_size=16, embed_dim=96, depth=2, heads=4, mlp_dim=192, dropout=0.1), B = 5; the second
# case is the second forward without reseeding (seeds 10 to 18)
IMG = dict(img=48, patch=16, C=3, depth=2, classes=7)
IMAGE_VIT_CASES = [Case("image_vit", 5, 10, 96, 4, 192, p=0.1, seed=11),
                   Case("image_vit", 5, 10, 96, 4, 192, p=0.1, seed=11, passes=2)]
CASES = {"post_norm": POST_NORM_CASES, "pre_norm": PRE_NORM_CASES, "adapter": ADAPTER_CASES,
         "image_vit": IMAGE_VIT_CASES}


@functools.lru_cache(maxsize=None)
def case_data(case):
    """(x, dout, P) float32 on the CPU; x and dout hold bf16-representable values, so both precisions and the
    reference read the same numbers."""
    gen = torch.Generator().manual_seed(1000 * case.N + case.D + case.F)
    rb = lambda *s: torch.randn(*s, generator=gen).to(torch.bfloat16).float()  # noqa: E731
    if case.kind == "image_vit":
        shapes = image_vit_params(IMG["C"], IMG["patch"], case.D, case.F, case.N, IMG["depth"], IMG["classes"])
        P = make_params(shapes, gen)
        return rb(case.B, IMG["C"], IMG["img"], IMG["img"]), rb(case.B, IMG["classes"]), P
    shapes = {"post_norm": POST_NORM_PARAMS, "pre_norm": PRE_NORM_PARAMS, "adapter": ADAPTER_PARAMS}[case.kind]
    P = make_params(shapes(case.D, case.F), gen)
    if case.kind == "adapter":
        P["alpha"] = torch.full((1,), case.alpha)
    return rb(case.B, case.N, case.D), rb(case.B, case.N, case.D), P


def case_masks(case, pas, device="cpu"):
    """The masks of pass `pas` (0-based) of a case: layer_masks for post_norm, [tokens, layer 0, layer 1] for
    image_vit, None without dropout."""
    if case.p <= 0 or case.kind in ("pre_norm", "adapter"):
        return None
    B, N, D, H, F, p = case.B, case.N, case.D, case.H, case.F, case.p
    if case.kind == "post_norm":
        s = site_seeds(case.seed, 4 * (pas + 1))[4 * pas:]
        return layer_masks(s, B, N, D, H, F, p, device)
    per = 1 + 4 * IMG["depth"]
    return image_vit_masks(case, site_seeds(case.seed, per * (pas + 1))[per * pas:], device)


def image_vit_masks(case, s, device="cpu"):
    """[tokens, layer 0, ...] masks of an image_vit case from the 1 + 4 * depth seeds of one pass, in draw order."""
    B, N, D, H, F, p = case.B, case.N, case.D, case.H, case.F, case.p
    assert len(s) == 1 + 4 * IMG["depth"]
    return [tokens_mask(s[0], B, N, D, p, device)] + [layer_masks(s[1 + 4 * i:5 + 4 * i], B, N, D, H, F, p, device)
                                                       for i in range(IMG["depth"])]


def replay_masks(case, drawn, replay, device="cpu"):
    """The masks of replay `replay` (1, 2, ...) of an image_vit step captured by fervit.graph.StepGraph after
    `drawn` host seeds (those of the eager warm-up steps): the captured launches keep the host seeds drawn + 1 ..
    drawn + 9, and every kernel mixes the device step counter into its seed (csrc/step_seed.h). The counter is
    advanced by the first node of the graph, so replay r runs with the counter at r."""
    per = 1 + 4 * IMG["depth"]
    host = site_seeds(case.seed, drawn + per)[drawn:]
    return image_vit_masks(case, [step_seed(h, replay) for h in host], device)


def forward(case, x, P, masks, num, eps=None):
    if case.kind == "post_norm":
        return post_norm_layer(x, P, masks or {}, case.p, case.act, 1e-5 if eps is None else eps, case.H, num)
    if case.kind == "pre_norm":
        return pre_norm_block(x, P, 1e-6, case.H, num)
    if case.kind == "adapter":
        return adapter(x, P, num)
    return image_vit(x, P, masks, case.p, IMG["patch"], case.H, IMG["depth"], num)


def run_case(case, num, device="cpu", masks_of=case_masks, accumulate=True):
    """Outputs and gradients of a case under `num`: {"out": last pass's output, "dx", <parameter name>: gradient};
    with passes > 1 the parameter gradients are the sum over the passes (accumulate=False: the last pass alone,
    the overwriting variant) and out / dx those of the last pass."""
    x0, dout0, P0 = case_data(case)
    P = {k: num.leaf(v.to(device)) for k, v in P0.items()}
    res = {}
    for pas in range(case.passes):
        x = num.leaf(x0.to(device), grad=case.kind != "image_vit")
        out = forward(case, x, P, masks_of(case, pas, device), num)
        if not accumulate:
            for v in P.values():
                v.grad = None
        out.backward(dout0.to(device).to(out.dtype))
        res["out"] = out.detach()
        if x.grad is not None:
            res["dx"] = x.grad
    res.update({k: v.grad for k, v in P.items()})
    return res


# ---------------------------------------------------------------------- scales, constants, comparison
def scale_of(name, ref):
    """scale_i = |ref_i| + rms(ref_T); the key third of a packed qkv bias (true gradient 0) takes the rms of the
    query third."""
    ref = ref.double()
    sc = ref.abs() + ref.pow(2).mean().sqrt()
    if name.endswith(KEY_BIAS):
        D = ref.numel() // 3
        sc = sc.clone()
        sc[D:2 * D] = ref[D:2 * D].abs() + ref[:D].pow(2).mean().sqrt()
    return sc


def out_round(dtype):
    return BF_ROUND if dtype == "bf16" else 0.0


def pairs(got, ref, dtype):
    o = out_round(dtype)
    return [(got[k], ref[k], scale_of(k, ref[k])) + ((o * ref[k].double().abs(),) if o else ()) for k in ref]


@functools.lru_cache(maxsize=None)
def c_table(kind, act="gelu"):
    """{dtype: c} of one layer kind: measure_c (x 4, floor 16) of float32 torch, and of the bf16 emulation with
    out_round = 2^-8, against float64 over every case of the kind the GPU test runs in that dtype. Never from a
    kernel. The post-norm layer has one constant per activation: ReLU's gate is a step, so a pre-activation that
    bf16 rounding moves across 0 changes a weight-gradient element by a whole term of its sum, and one constant
    for both would hand GELU that slack."""
    ps = {"fp32": [], "bf16": []}
    for case in (c for c in CASES[kind] if c.act == act):
        ref = run_case(case, REF)
        for dtype in case.dtypes:
            ps[dtype] += pairs(run_case(case, emulate(dtype)), ref, dtype)
    return {dtype: measure_c(f"layer {kind} {act}", dtype, ps[dtype]) for dtype in ps}


@functools.lru_cache(maxsize=None)
def replay_c_table(case, drawn, replays):
    """{dtype: (c of the replayed step, its own CPU measurement)} for tests/test_gpu_graph_dropout.py: c_table of
    the kind (measured with the eager masks), or, where the same CPU measurement with the masks of replays 1 ..
    `replays` (replay_masks) comes out larger, that one (measure_c: x 4, floor 16). Never from a kernel."""
    table = c_table(case.kind, case.act)
    ps = {dtype: [] for dtype in case.dtypes}
    for r in range(1, replays + 1):
        masks_of = lambda c, pas, device, r=r: replay_masks(c, drawn, r, device)  # noqa: E731
        ref = run_case(case, REF, masks_of=masks_of, accumulate=False)
        for dtype in case.dtypes:
            ps[dtype] += pairs(run_case(case, emulate(dtype), masks_of=masks_of, accumulate=False), ref, dtype)
    own = {dtype: measure_c(f"layer {case.kind} replayed", dtype, ps[dtype]) for dtype in ps}
    return {dtype: (max(table[dtype], own[dtype]), own[dtype]) for dtype in ps}


def compare(tag, got, ref, c, dtype, worst=None):
    """assert_close on every tensor of `ref` (all of them must be in `got`); returns {name: worst err / bound}."""
    w = {}
    for k, r in ref.items():
        assert k in got and got[k] is not None, f"{tag}: no {k}"
        w[k] = assert_close(f"{tag} {k}", got[k], r, scale_of(k, r), c, out_round(dtype))
    if worst is not None:
        for k, v in w.items():
            worst[k] = max(worst.get(k, 0.0), v)
    return w
