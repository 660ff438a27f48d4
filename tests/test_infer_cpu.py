"""CPU checks of the low-latency inference feature: the float64 reference of fer_skinny_linear
(tests/skinny_ref.py) against a float32 torch composition under every flag combination, the seeded ReLU
operands of the GPU test, the ABI declarations, and InferenceSession's refusal of a CPU model."""
import os
import re

import pytest
import torch

import skinny_ref as R
from elemwise import assert_close, measure_c

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("f", R.FLAGS, ids=R.flag_id)
def test_reference_matches_float32_torch(f):
    """skinny_ref against F.layer_norm / F.linear / F.relu / F.gelu / add in float32 on the same inputs, per
    element within tests/elemwise.py's bound with no output rounding: |f32 - ref| <= 16 * 2^-23 * scale (16:
    measure_c's floor, i.e. float32 arithmetic is at most 16 units of 2^-23 * scale away)."""
    for M, K, N in ((1, 64, 8), (19, 512, 96), (33, 384, 40)):
        t = R.case(M, K, N, f)
        kw = R.call_args(t, f)
        ref, scale, pre, sacc = R.skinny_ref(t.A, t.W, parts=True, **kw)
        got = R.skinny_f32(t.A, t.W, **kw)
        assert ref.shape == (M, N) and (scale > 0).all()
        if f.act == "relu":
            live = R.relu_live(pre, sacc, kw["bias"], 16.0, f.ln_a)
            assert live.all()
        assert_close(f"{R.flag_id(f)} M={M} K={K} N={N}", got, ref, scale, 16.0, 0.0)


@pytest.mark.parametrize("K,N", R.KNS)
def test_relu_operands_stay_clear_of_zero(K, N):
    """The GPU test leaves out ReLU outputs whose pre-activation lies within its own bound of zero and asserts
    that this is at most 0.1 % of a case. Here the float64 reference alone shows the seeded operands stay within
    that for every shape and ReLU flag combination, with c as the GPU test measures it (on the float32
    composition), and that both branches of the ReLU are taken."""
    for M in R.MS:
        for f in (f for f in R.FLAGS if f.act == "relu"):
            t = R.case(M, K, N, f)
            kw = R.call_args(t, f)
            ref, scale, pre, sacc = R.skinny_ref(t.A, t.W, parts=True, **kw)
            c = measure_c("skinny", R.flag_id(f), [(R.skinny_f32(t.A, t.W, **kw), ref, scale)])
            live = R.relu_live(pre, sacc, kw["bias"], c, f.ln_a)
            assert (~live).sum().item() <= 1e-3 * live.numel(), (M, K, N, R.flag_id(f))
            assert (pre[live] > 0).any() and (pre[live] < 0).any()


def test_skinny_linear_is_declared_and_bound():
    from fervit._lib import SIGNATURES

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fervit.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+fer_skinny_linear\s*\(", hdr)
    assert "fer_skinny_linear" in SIGNATURES
    res, args = SIGNATURES["fer_skinny_linear"]
    proto = re.search(r"fer_skinny_linear\s*\(([^()]*)\)", hdr).group(1)
    assert len(args) == len(proto.split(","))
    from fervit import ops

    assert callable(ops.skinny_linear)


def test_session_refuses_a_cpu_model():
    from fervit.infer import InferenceSession
    from models_fer_vit.latent_vit import LatentViT

    m = LatentViT(depth=1, embed_dim=64, heads=4, mlp_dim=128, latent_dim=64).eval()
    with pytest.raises(RuntimeError, match="CPU"):
        InferenceSession(m, batch_size=1)
    with pytest.raises(ValueError):
        InferenceSession(m, batch_size=1, skinny="maybe")
