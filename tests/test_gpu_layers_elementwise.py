"""The composed layers, through their modules, against the float64 formulas of tests/layer_ref.py, element by
element: output, input gradient and every parameter gradient of EncoderLayer (dropout
on: the masks both kernels of each site rebuild are predicted on the host from the seed stream), Block,
AdapterModule and a two-layer ImageViT. FlatParams, the bf16 shadow, the weight-gradient stream and the
deferred-reduction window are the real ones.

|got - ref| <= out_round |ref| + c 2^-23 (|ref_i| + rms(ref_T)), c per layer kind from the CPU runs of float32
torch and of the bf16 emulation against float64 (layer_ref.c_table; tests/test_layer_bound_cpu.py shows that
gate sound and that seven ways of breaking the pairing fail it). The reference runs on the GPU in double."""
import functools

import pytest
import torch

import fervit
import layer_ref as L
from elemwise import assert_bits_equal
from fervit import layers, runtime
from fervit._lib import check, lib
from fervit.blocks import AdapterModule, Block, EncoderLayer
from models_fer_vit.image_vit import ImageViT

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = ("fp32", "bf16")
ONE_PASS = [c for c in L.POST_NORM_CASES if c.p > 0 and c.passes == 1]
NO_DROP = next(c for c in L.POST_NORM_CASES if c.p == 0)
TWO_PASS = next(c for c in L.POST_NORM_CASES if c.passes == 2)
SMALL_01 = next(c for c in L.POST_NORM_CASES if c.p == 0.1 and c.passes == 1)


def by_dtype(cases):
    return [pytest.param(c, d, id=f"{c.id}-{d}") for c in cases for d in c.dtypes]


@pytest.fixture(autouse=True)
def eager_seed_stream():
    """Eager steps: no device step counter mixed into the seeds (fervit.graph sets one while it captures)."""
    check(lib().fer_set_step_counter(None), "set_step_counter")
    yield
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def ref(case):
    return L.run_case(case, L.REF, device=DEV)


def build(case, dtype, train=True, dropout=None):
    p = case.p if dropout is None else dropout
    if case.kind == "post_norm":
        m = EncoderLayer(case.D, case.H, case.F, dropout=p, activation=case.act)
    elif case.kind == "pre_norm":
        m = Block(case.D, case.H, mlp_ratio=case.F / case.D)
    elif case.kind == "adapter":
        m = AdapterModule(case.D, case.F)
    else:
        m = ImageViT(img_size=L.IMG["img"], patch_size=L.IMG["patch"], embed_dim=case.D, depth=L.IMG["depth"],
                     heads=case.H, mlp_dim=case.F, dropout=p)
    P = L.case_data(case)[2]
    named = dict(m.named_parameters())
    assert set(named) == set(P), set(named) ^ set(P)
    with torch.no_grad():
        for k, v in named.items():
            v.copy_(P[k])
    m = m.to(DEV)
    m.set_precision(dtype)
    return m.train(train)


def run(m, case, dtype, passes=1, between=None):
    """fervit.manual_seed(case.seed), then `passes` forward + backward runs (no zero_grad, no reseeding)."""
    x0, dout0, _ = L.case_data(case)
    image = case.kind == "image_vit"
    dt = torch.float32 if image or dtype == "fp32" else torch.bfloat16
    fervit.manual_seed(case.seed)
    for pas in range(passes):
        x = x0.to(DEV).to(dt).requires_grad_(not image)
        out = m(x)
        out.backward(dout0.to(DEV).to(out.dtype))
        if between is not None and pas + 1 < passes:
            between(m)
    torch.cuda.synchronize()
    got = {k: v.grad for k, v in m.named_parameters()}
    got["out"] = out.detach()
    if not image:
        got["dx"] = x.grad
    return got


def check_case(tag, got, want, case, dtype):
    c = L.c_table(case.kind, case.act)[dtype]
    w = L.compare(f"{tag} {dtype}", got, want, c, dtype)
    k = max(w, key=w.get)
    print(f"worst err/bound {tag} {dtype}: {w[k]:.3f} ({k}), c = {c:.1f}")


# ---------------------------------------------------------------------- EncoderLayer
@pytest.mark.parametrize("case,dtype", by_dtype(ONE_PASS))
def test_encoder_layer_dropout(case, dtype):
    """p = 0.1 (one case 0.5): 95 rows (less than one tile), 259 rows (crosses row tiles, odd N), gelu and relu;
    ViT-B geometry at 394 rows in bf16."""
    check_case(case.id, run(build(case, dtype), case, dtype), ref(case), case, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ["train_p0", "eval_p01"])
def test_encoder_layer_without_masks(mode, dtype):
    """Dropout 0 in train mode, and dropout 0.1 in eval mode: no seed is drawn and the result is the mask-free
    reference."""
    case = NO_DROP
    m = build(case, dtype, train=mode == "train_p0", dropout=0.0 if mode == "train_p0" else 0.1)
    got = run(m, case, dtype)
    assert runtime.SEEDS.counter == 0, "a seed was drawn"
    check_case(f"{case.id} {mode}", got, ref(case), case, dtype)


def test_encoder_layer_split_k_weight_gradients(monkeypatch):
    """bf16 with the grouped weight-gradient launch off: the per-weight split-K GEMMs (ViT-B's path) at 95 rows."""
    monkeypatch.setattr(layers, "WGRAD_GROUP_MAX_M", 0)
    case = SMALL_01
    check_case(f"{case.id} split-K", run(build(case, "bf16"), case, "bf16"), ref(case), case, "bf16")


# ---------------------------------------------------------------------- accumulation and _targets
@pytest.mark.parametrize("dtype", DTYPES)
def test_two_backwards_accumulate(dtype):
    """Two passes, no zero_grad, fresh masks on the second (seeds 5 to 8): the float64 sum of both."""
    case = TWO_PASS
    check_case(case.id, run(build(case, dtype), case, dtype, passes=2), ref(case), case, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_backwards_mixed_targets(dtype):
    """linear1.weight.grad and norm2.bias.grad set to None between the passes (the branch of _targets that
    zeroes): those two hold the second pass alone, the rest the sum."""
    case = TWO_PASS
    fresh = ("linear1.weight", "norm2.bias")

    def drop_two(m):
        named = dict(m.named_parameters())
        for k in fresh:
            named[k].grad = None

    want = dict(ref(case))
    last = L.run_case(case, L.REF, device=DEV, accumulate=False)
    for k in fresh:
        want[k] = last[k]
    check_case(f"{case.id} mixed", run(build(case, dtype), case, dtype, passes=2, between=drop_two), want, case, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_frozen_parameters(dtype):
    """requires_grad = False on self_attn.in_proj_weight and linear2.bias: no .grad for them, every other gradient
    and dx the bits of the all-trainable run."""
    case = SMALL_01
    frozen = ("self_attn.in_proj_weight", "linear2.bias")
    full = {k: v.clone() for k, v in run(build(case, dtype), case, dtype).items()}
    m = build(case, dtype)
    named = dict(m.named_parameters())
    for k in frozen:
        named[k].requires_grad_(False)
    got = run(m, case, dtype)
    for k, v in got.items():
        if k in frozen:
            assert v is None, f"{k} is frozen but has a gradient"
        else:
            assert_bits_equal(f"frozen run {dtype} {k}", v, full[k])


# ---------------------------------------------------------------------- Block, AdapterModule
@pytest.mark.parametrize("case,dtype", by_dtype(L.PRE_NORM_CASES))
def test_block(case, dtype):
    """timm Block, mlp_ratio 2, eps 1e-6, no dropout."""
    check_case(case.id, run(build(case, dtype), case, dtype), ref(case), case, dtype)


@pytest.mark.parametrize("case,dtype", by_dtype(L.ADAPTER_CASES))
def test_adapter(case, dtype):
    """adapter_dim 24, alpha 0.37 and 0 (at 0 only alpha's gradient and the residual are non-zero)."""
    check_case(case.id, run(build(case, dtype), case, dtype), ref(case), case, dtype)


# ---------------------------------------------------------------------- ImageViT
@pytest.mark.parametrize("case,dtype", by_dtype(L.IMAGE_VIT_CASES))
def test_image_vit(case, dtype):
    """Logits and every parameter gradient against patch_tokens -> 2 x post_norm_layer -> head with the 1 + 4 + 4
    predicted seeds (tokens first, then attention, out-proj, fc1, fc2 per layer; the head draws none). The
    two-pass case runs a second forward + backward without reseeding: its logits come from seeds 10 to 18 and
    the gradients are the sum of both passes."""
    m = build(case, dtype)
    got = run(m, case, dtype, passes=case.passes)
    assert runtime.SEEDS.counter == 9 * case.passes
    check_case(case.id, got, ref(case), case, dtype)
