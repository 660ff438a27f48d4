"""fervit.explain on whole models (GPU): attention maps of the small ImageViT against the CPU oracle's
in-proj + explicit softmax on the same state_dict, bf16 maps against fp32 maps, and for every model
family: one map per layer of the right size, CLS-only rows bit-equal to row 0, logits untouched by
the tap, rollout against rollout_reference, cls_saliency shapes, and the eval / no-grad contract.

Gates: the caps of tests/test_gpu_attention_probs.py (1e-4 fp32, 2e-2 bf16: here the layer INPUTS
carry the model's own error, so the kernel-level gates do not apply) and the rollout gate of
tests/test_gpu_attention_rollout.py."""
import math

import pytest
import torch

import vit_oracle as O
from cases import CASES, case_inputs, fixture_state_dict, load_fixture
from detparams import det_directions

pytestmark = pytest.mark.gpu

DEV = "cuda"
FP32_CAP, BF16_CAP = 1e-4, 2e-2
ROLLOUT_GATE = 4 * 2.5e-8  # tests/test_gpu_attention_rollout.py


def image_vit_48():
    from models_fer_vit.image_vit import ImageViT

    m = ImageViT(**CASES["image_vit_48"]["ctor"])
    sd = fixture_state_dict(load_fixture("image_vit_48"))
    m.load_state_dict(sd)
    return m.to(DEV), sd, case_inputs("image_vit_48")[0]


def oracle_maps(x, sd):
    """[L, B, H, N, N] fp64: every encoder layer's softmax(q k^T / sqrt(dh)) from the oracle's packed
    in-proj on that layer's input (oracle/vit_oracle.py image_vit_forward, layer by layer)."""
    a = CASES["image_vit_48"]["ctor"]
    p = {k: v.double() for k, v in sd.items()}
    B, H = x.shape[0], a["heads"]
    t = O.patch_embed(x.double(), p["patch_embed.proj.weight"], p["patch_embed.proj.bias"], a["patch_size"])
    t = torch.cat([p["cls_token"].expand(B, -1, -1), t], 1) + p["pos_embed"]
    maps = []
    for i in range(a["depth"]):
        pre = f"transformer.layers.{i}."
        N, D = t.shape[1], t.shape[2]
        qkv = t @ p[pre + "self_attn.in_proj_weight"].t() + p[pre + "self_attn.in_proj_bias"]
        q, k, _ = (u.reshape(B, N, H, D // H).permute(0, 2, 1, 3) for u in qkv.split(D, dim=-1))
        maps.append(torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(D // H), dim=-1))
        t = O.encoder_layer_postnorm(t, p, pre, H, "gelu")
    return torch.stack(maps)


def test_image_vit_maps_match_the_oracle_fp32_and_bf16():
    from fervit.explain import attention_maps

    m, sd, x = image_vit_48()
    a = CASES["image_vit_48"]["ctor"]
    ref = oracle_maps(x, sd)
    m.set_precision("fp32")
    f32 = attention_maps(m, x.to(DEV), average_heads=False)
    assert f32.shape == (a["depth"], x.shape[0], a["heads"], 10, 10) and f32.dtype == torch.float32
    e32 = (f32.cpu().double() - ref).abs().max().item()
    m.set_precision("bf16")
    b16 = attention_maps(m, x.to(DEV), average_heads=False)
    e16 = (b16 - f32).abs().max().item()
    print(f"explain-measure image_vit_48 fp32-vs-oracle {e32:.3e} bf16-vs-fp32 {e16:.3e}")
    assert e32 <= FP32_CAP, e32
    assert e16 <= BF16_CAP, e16
    avg = attention_maps(m, x.to(DEV))
    assert (avg - b16.mean(2)).abs().max().item() <= 1e-6


def _hybrid(seq_len=18, adapter_dim=32):
    from models_fer_vit.hybrid_latent_vit import HybridLatentViT

    return HybridLatentViT(latent_dim=64, seq_len=seq_len, pretrained_model_name="vit_tiny_patch16_224", num_classes=7,
                           use_pretrained=False, adapter_dim=adapter_dim)


def _family(name):
    """(model on the device, input, layers, tokens N) -- the small configurations the other GPU tests build."""
    torch.manual_seed(3)
    g = torch.Generator().manual_seed(5)
    if name == "image_vit":
        m, _, x = image_vit_48()
        return m, x.to(DEV), 6, 10
    if name == "latent_vit":
        from models_fer_vit.latent_vit import LatentViT

        return LatentViT(depth=2).to(DEV), torch.randn(4, 18, 512, generator=g).to(DEV), 2, 19
    if name == "latent_vit_v2":
        from models_fer_vit.latent_vit_v2 import LatentViTv2

        m = LatentViTv2(**CASES["latent_vit_v2_lwn"]["ctor"])  # heads = 4: dh = 128
        return m.to(DEV), torch.randn(4, 18, 512, generator=g).to(DEV), 2, 19
    if name == "hybrid_adapters":
        return _hybrid().to(DEV), torch.randn(4, 18, 64, generator=g).to(DEV), 12, 19
    if name == "hybrid_plain":
        return _hybrid(adapter_dim=None).to(DEV), torch.randn(4, 18, 64, generator=g).to(DEV), 12, 19
    if name in ("expression_aware", "expression_aware_concat"):
        from models_fer_vit.expression_aware_vit import ExpressionAwareViT
        from models_fer_vit.latent_decomposer import LatentDecomposer

        dirs = det_directions(7, 18, 64)
        dec = LatentDecomposer({i: dirs[i] for i in range(7)}, seq_len=18, latent_dim=64)
        if name == "expression_aware":
            m = ExpressionAwareViT(dec, _hybrid())
            return m.to(DEV), torch.randn(4, 18, 64, generator=g).to(DEV), 12, 19
        m = ExpressionAwareViT(dec, _hybrid(seq_len=36), output_mode="concat")
        return m.to(DEV), torch.randn(4, 18, 64, generator=g).to(DEV), 12, 37
    raise ValueError(name)


FAMILIES = ["image_vit", "latent_vit", "latent_vit_v2", "hybrid_adapters", "hybrid_plain", "expression_aware",
            "expression_aware_concat"]


@pytest.mark.parametrize("name", FAMILIES)
def test_every_family_maps_rollout_and_untouched_logits(name):
    from fervit import layers
    from fervit.explain import attention_maps, attention_rollout, capture_attention, cls_saliency, rollout_reference

    m, x, depth, N = _family(name)
    B = x.shape[0]
    m.train()
    maps = attention_maps(m, x)
    assert m.training and layers.ATTN_TAP is None  # mode restored, tap removed
    assert maps.shape == (depth, B, N, N) and maps.dtype == torch.float32
    assert (maps.sum(-1) - 1).abs().max().item() <= 4 * N * 2.0 ** -23
    cls = attention_maps(m, x, queries="cls")
    assert cls.shape == (depth, B, 1, N) and torch.equal(cls, maps[:, :, :1])
    some = attention_maps(m, x, layers={0, depth - 1})
    assert torch.equal(some, maps[[0, depth - 1]])
    # the tap changes nothing in the forward
    m.eval()
    with torch.no_grad():
        plain = m(x)
        with capture_attention() as got:
            tapped = m(x)
    assert len(got) == depth and torch.equal(plain, tapped)
    assert torch.equal(torch.stack(got), maps)
    # rollout: device chain of vector-matrix products against the fp64 definition
    r = attention_rollout(m, x)
    ref = rollout_reference(maps.cpu(), 0.5)
    err = (r.cpu().double() - ref).abs().max().item()
    print(f"explain-measure {name} rollout {err:.3e}")
    assert r.shape == (B, N) and err <= ROLLOUT_GATE, err
    sal = cls_saliency(m, x)
    assert sal.shape == ((B, 3, 3) if name == "image_vit" else (B, N - 1))
    assert sal.min().item() >= 0 and (sal.reshape(B, -1).sum(1) - 1).abs().max().item() <= 1e-5


def _train_step(prec):
    """One seeded training step of a small ImageViT with dropout; the updated flat parameters."""
    import fervit
    from fervit.optim import FusedAdamW
    from models_fer_vit.image_vit import ImageViT

    g = torch.Generator().manual_seed(5)
    x = torch.randn(8, 3, 48, 48, generator=g).to(DEV)
    y = torch.randint(0, 7, (8,), generator=g).to(DEV)
    torch.manual_seed(0)
    m = ImageViT(img_size=48, patch_size=16, embed_dim=384, depth=2, heads=8, mlp_dim=1536, dropout=0.1)
    m = m.to(DEV).set_precision(prec)
    opt = FusedAdamW(m.parameters(), lr=1e-3, weight_decay=0.05, model=m)
    fervit.manual_seed(11)
    opt.zero_grad()
    loss = torch.nn.functional.cross_entropy(m(x), y)
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    return m, x, loss.detach().clone(), m.fer_flat().data.clone()


def test_maps_are_eval_no_grad_only_and_training_is_unaffected():
    from fervit import layers
    from fervit.explain import capture_attention

    _, _, loss0, flat0 = _train_step("bf16")
    m, x, _, _ = _train_step("bf16")
    m.train()
    with pytest.raises(RuntimeError, match="eval / no-grad"):  # train mode: gradients recorded, dropout on
        with capture_attention():
            m(x)
    assert layers.ATTN_TAP is None
    m.eval()
    with pytest.raises(RuntimeError, match="eval / no-grad"):  # eval mode, grad enabled
        with capture_attention():
            m(x)
    assert layers.ATTN_TAP is None
    m.train()
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="eval / no-grad"):  # no grad, but attention dropout on
            with capture_attention():
                m(x)
    assert layers.ATTN_TAP is None
    # a plain training step afterwards is the step taken before the attempts, bit for bit
    _, _, loss1, flat1 = _train_step("bf16")
    assert torch.equal(loss0, loss1) and torch.equal(flat0, flat1)
