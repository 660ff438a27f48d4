"""CPU checks of the pre-norm skinny plan: the float64 reference of fer_skinny_adapter
(tests/skinny_adapter_ref.py) against the oracle's adapter, its error bound against a float32 torch composition
with the kernel's two rounding points, the ABI declarations, and what InferenceSession's _Plan recognises of the
HybridLatentViT / ExpressionAwareViT family on CPU-built models."""
import os
import re

import pytest
import torch

import skinny_adapter_ref as R
import vit_oracle as O
from detparams import det_directions
from elemwise import BF_ROUND, assert_close, measure_c

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_matches_the_oracle_adapter():
    """adapter_ref against oracle.adapter on unrounded float64 operands (both are exact up to float64
    rounding), and its scale terms are positive."""
    g = torch.Generator().manual_seed(1)
    M, D, A = 19, 96, 48
    x = torch.randn(M, D, generator=g, dtype=torch.float64)
    p = {"adapter.0.weight": torch.randn(A, D, generator=g, dtype=torch.float64) / D ** 0.5,
         "adapter.0.bias": 0.2 * torch.randn(A, generator=g, dtype=torch.float64),
         "adapter.2.weight": torch.randn(D, A, generator=g, dtype=torch.float64) / A ** 0.5,
         "adapter.2.bias": 0.2 * torch.randn(D, generator=g, dtype=torch.float64),
         "alpha": torch.tensor([0.375], dtype=torch.float64)}  # exact in fp32
    want = O.adapter(x, p, "")
    ref, scale, sacc, carry = R.adapter_ref(x, p["adapter.0.weight"], p["adapter.0.bias"], p["adapter.2.weight"],
                                            p["adapter.2.bias"], 0.375)
    assert (ref - want).abs().max().item() <= 1e-13 * want.abs().max().item()
    assert (scale > 0).all() and (sacc > 0).all() and (carry > 0).all()


@pytest.mark.parametrize("D,A", R.DRS)
@pytest.mark.parametrize("M", R.MS)
def test_the_bound_holds_for_a_float32_composition_with_the_kernels_roundings(M, D, A):
    """From the reference alone: float32 torch with H and the result rounded to bf16 lies inside the bound the
    GPU test applies, for every case of that test, so the bound is satisfiable; and without the two roundings
    the fp32 composition is inside c * 2^-23 * scale plus the carried first-product term."""
    t = R.operands(M, D, A)
    for alpha in R.ALPHAS:
        ref, scale, sacc, carry = R.adapter_ref(t.X, t.W1, t.b1, t.W2, t.b2, alpha)
        c = measure_c("skinny_adapter", f"M={M} D={D} R={A} alpha={alpha}",
                      [(R.adapter_f32(t.X, t.W1, t.b1, t.W2, t.b2, alpha), ref, scale)])
        extra = R.adapter_extra(alpha, sacc, carry, c)
        name = f"adapter M={M} D={D} R={A} alpha={alpha}"
        got = R.adapter_f32(t.X, t.W1, t.b1, t.W2, t.b2, alpha, round_h=True, round_out=True)
        assert_close(name, got, ref, scale, c, BF_ROUND, extra)
        if alpha == 0.0:
            assert torch.equal(got, t.X)
            assert (extra == 0).all()


def test_skinny_adapter_is_declared_and_bound():
    from fervit._lib import SIGNATURES

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fervit.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+fer_skinny_adapter\s*\(", hdr)
    res, args = SIGNATURES["fer_skinny_adapter"]
    proto = re.search(r"fer_skinny_adapter\s*\(([^()]*)\)", hdr).group(1)
    assert len(args) == len(proto.split(",")) == 15
    from fervit import ops

    assert callable(ops.skinny_adapter)


# ---------------------------------------------------------------------- _Plan on CPU-built models
def _hybrid(size, adapter_dim, seq_len=18, latent=64):
    from models_fer_vit.hybrid_latent_vit import HybridLatentViT

    return HybridLatentViT(latent_dim=latent, seq_len=seq_len, pretrained_model_name=f"vit_{size}_patch16_224",
                           num_classes=7, use_pretrained=False, adapter_dim=adapter_dim).eval()


def _plan(m):
    from fervit.infer import _Plan

    return _Plan(m)


@pytest.mark.parametrize("adapter_dim", [None, 32, 64])
@pytest.mark.parametrize("size,D", [("tiny", 192), ("small", 384), ("base", 768)])
def test_plan_recognises_the_hybrid(size, D, adapter_dim):
    m = _hybrid(size, adapter_dim)
    p = _plan(m)
    assert p.why is None, p.why
    assert p.prenorm and p.kind is not None
    assert p.N == 19 and p.sample_shape == (18, 64)
    assert len(p.blocks) == 12 and p.blocks[0].norm1.weight.shape == (D,)
    assert (p.adapters is None) == (adapter_dim is None)
    assert p.head_ln is m.head[0] and p.head_lin is m.head[2]
    assert p.decompose is None and p.spec is None


@pytest.mark.parametrize("output_mode,tokens", [("expr_only", 18), ("concat", 36)])
def test_plan_recognises_expression_aware_vit(output_mode, tokens):
    from models_fer_vit.expression_aware_vit import ExpressionAwareViT
    from models_fer_vit.latent_decomposer import LatentDecomposer

    dirs = det_directions(7, 18, 64)
    dec = LatentDecomposer({i: dirs[i] for i in range(7)}, seq_len=18, latent_dim=64)
    spe = output_mode == "expr_only"
    m = ExpressionAwareViT(dec, _hybrid("tiny", 32, seq_len=tokens), output_mode=output_mode, use_spe=spe,
                           use_leam=spe).eval()
    p = _plan(m)
    assert p.why is None, p.why
    assert p.prenorm and p.core is m.vit
    assert p.N == tokens + 1 and p.sample_shape == (18, 64)
    assert p.decompose is not None and (p.spec is not None) == spe


def test_plan_names_the_adapter_width():
    p = _plan(_hybrid("tiny", 24))
    assert p.why is not None and "adapter width 24" in p.why


def test_plan_keeps_post_norm_in_the_message_for_other_models():
    from fervit.blocks import Block
    from fervit.module import FerModule

    class PreNorm(FerModule):
        def __init__(self):
            super().__init__()
            self.block = Block(256, 4)

        def forward(self, x):
            return self.block(x)[:, 0].float()

    p = _plan(PreNorm().eval())
    assert p.kind is None and "post-norm" in p.why


def test_post_norm_models_plan_as_before():
    from models_fer_vit.latent_vit import LatentViT

    p = _plan(LatentViT(depth=1, embed_dim=64, heads=4, mlp_dim=128, latent_dim=64).eval())
    assert p.why is None and p.kind == "latent" and not p.prenorm
