"""InferenceSession (fervit/infer.py) on the committed fixtures: the graph-only plan is the eager eval
forward bit for bit, the skinny plan stays inside the project's bf16 logits gates against the reference, and
the session's behaviour (static buffers, predict, errors, weight refresh)."""
import numpy as np
import pytest
import torch

from cases import CASES, case_inputs, fixture_state_dict, load_fixture
from elemwise import assert_bits_equal

pytestmark = pytest.mark.gpu

MODELS = ["latent_vit", "latent_vit_v2_all", "image_vit_48"]
# tests/test_gpu_models.py BF16_GATES[name][0]: the project's bf16 logits gate against the reference
LOGIT_GATES = {"latent_vit": 0.032, "latent_vit_v2_all": 0.058, "image_vit_48": 0.044}


def build(name, prec):
    from models_fer_vit.image_vit import ImageViT
    from models_fer_vit.latent_vit import LatentViT
    from models_fer_vit.latent_vit_v2 import LatentViTv2

    c = CASES[name]
    cls = {"image_vit": ImageViT, "latent_vit": LatentViT, "latent_vit_v2": LatentViTv2}[c["kind"]]
    m = cls(**c["ctor"])
    fx = load_fixture(name)
    m.load_state_dict(fixture_state_dict(fx))
    return m.cuda().set_precision(prec).eval(), fx


def eager(m, x):
    with torch.no_grad():
        return m(x).float().clone()


def session(*a, **kw):
    from fervit.infer import InferenceSession

    return InferenceSession(*a, **kw)


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
@pytest.mark.parametrize("name", MODELS)
def test_graph_only_is_the_eager_forward(name, prec):
    m, fx = build(name, prec)
    x = case_inputs(name)[0].cuda()
    want = eager(m, x)
    with session(m, batch_size=x.shape[0], skinny="off") as s:
        assert not s.skinny
        got = s.run(x).clone()
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert_bits_equal(f"{name} {prec}: session against eager", got, want)
    if prec == "fp32":
        assert np.abs(got.cpu().numpy() - fx["logits_eval"]).max() < 1e-3


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", MODELS)
def test_skinny_plan_against_the_reference(name, B):
    m, fx = build(name, "bf16")
    x = case_inputs(name)[0][:B].cuda()
    ref = fx["logits_eval"][:B]
    with session(m, batch_size=B, skinny="on") as s:
        assert s.skinny
        got = s.run(x).cpu().numpy()
    err = np.abs(got - ref).max()
    err_eager = np.abs(eager(m, x).cpu().numpy() - ref).max()
    print(f"skinny {name} B={B}: max|logits - ref| = {err:.4f} (eager bf16 {err_eager:.4f}, gate {LOGIT_GATES[name]})")
    assert err < LOGIT_GATES[name]
    top2 = np.sort(ref, axis=1)[:, -2:]
    sure = (top2[:, 1] - top2[:, 0]) > 0.2
    assert (got.argmax(1)[sure] == ref.argmax(1)[sure]).all()


@pytest.mark.parametrize("skinny", ["off", "on"])
def test_inputs_outputs_and_predict(skinny):
    m, _ = build("latent_vit", "bf16")
    x = case_inputs("latent_vit")[0].cuda()
    xa, xb = x[:2], x[2:4]
    with session(m, batch_size=2, skinny=skinny) as s:
        a1 = s.run(xa).clone()
        b1 = s.run(xb.cpu()).clone()  # a host tensor
        a2 = s.run(xa).clone()
        pred, probs = s.predict(xb)
        assert_bits_equal("the same input twice", a1, a2)
        assert_bits_equal("predict's probabilities", probs, torch.softmax(b1, dim=1))
        assert (pred == b1.argmax(dim=1)).all()
        if skinny == "off":
            assert_bits_equal("first input", a1, eager(m, xa))
            assert_bits_equal("second input", b1, eager(m, xb))
        else:
            # each input's own result: against eager bf16 both are within twice the bf16 gate, and the two differ
            for got, xi in ((a1, xa), (b1, xb)):
                assert (got - eager(m, xi)).abs().max().item() < 2 * LOGIT_GATES["latent_vit"]
            assert (a1 - b1).abs().max().item() > 0
            with session(m, batch_size=2, skinny="on") as s2:
                assert_bits_equal("a fresh session on the second input", s2.run(xb), b1)


def test_errors_name_their_cause():
    from fervit import layers

    m, _ = build("latent_vit", "bf16")
    with pytest.raises(RuntimeError, match="rows exceeds"):
        session(m, batch_size=4, skinny="on")  # 4 * 19 = 76 rows
    with session(m, batch_size=1) as s:
        with pytest.raises(RuntimeError, match="input shape"):
            s.run(torch.zeros(2, 18, 512, device="cuda"))
        m.train()
        with pytest.raises(RuntimeError, match=r"train\(\) mode"):
            s.run(torch.zeros(1, 18, 512, device="cuda"))
        with pytest.raises(RuntimeError, match=r"train\(\) mode"):
            session(m, batch_size=1)
        m.eval()
    m32, _ = build("latent_vit", "fp32")
    with pytest.raises(RuntimeError, match="fp32"):
        session(m32, batch_size=1, skinny="on")
    for tap in ("ATTN_TAP", "TOKEN_TAP"):
        setattr(layers, tap, lambda *a: None)
        try:
            with pytest.raises(RuntimeError, match="tap"):
                session(m, batch_size=1)
        finally:
            setattr(layers, tap, None)


def test_skinny_on_refuses_a_pre_norm_model():
    from fervit.blocks import Block
    from fervit.module import FerModule

    class PreNorm(FerModule):
        def __init__(self):
            super().__init__()
            self.block = Block(256, 4)

        def forward(self, x):
            return self.block(x)[:, 0].float()

    m = PreNorm().cuda().eval()
    with pytest.raises(RuntimeError, match="post-norm"):
        session(m, batch_size=1, skinny="on", input_shape=(10, 256))
    x = torch.randn(1, 10, 256, device="cuda")
    with session(m, batch_size=1, input_shape=(10, 256)) as s:  # "auto" runs it graph-only
        assert not s.skinny
        assert_bits_equal("pre-norm block, graph-only", s.run(x), eager(m, x))


@pytest.mark.parametrize("skinny", ["off", "on"])
def test_refresh_after_load_state_dict(skinny):
    m, _ = build("latent_vit", "bf16")
    x = case_inputs("latent_vit")[0][:1].cuda()
    with session(m, batch_size=1, skinny=skinny) as s:
        before = s.run(x).clone()
        sd = {k: v + 0.01 * torch.sign(v) for k, v in m.state_dict().items()}
        m.load_state_dict(sd)
        assert_bits_equal("a snapshot until refresh()", s.run(x), before)
        s.refresh()
        after = s.run(x).clone()
        assert (after - before).abs().max().item() > 0
        with session(m, batch_size=1, skinny=skinny) as fresh:
            assert_bits_equal("refreshed session against a fresh one on the new weights", after, fresh.run(x))
        if skinny == "off":
            assert_bits_equal("refreshed session against eager on the new weights", after, eager(m, x))
        else:
            # two bf16 evaluations of one function, each within the bf16 gate of its exact value
            assert (after - eager(m, x)).abs().max().item() < 2 * LOGIT_GATES["latent_vit"]
        assert s.captures == 1  # nothing moved: no recapture
