"""Evaluation on whole models (GPU): fervit.explain.final_tokens / token_similarity and
eval.evaluate_model on LatentViT (depth 2) and the 48 px ImageViT with the deterministic weights of
tests/golden/detparams.py.

token_similarity is held to the kernel bound of tests/test_gpu_token_cosine.py (c 2^-23 scale against float64
torch cosine on the tokens the tap handed out), probabilities to the softmax bound of
tests/test_gpu_cls_metrics.py; predictions are exact; the meter's accuracy and f1_macro agree with
train.common.run_evaluate (sklearn on the host) to 1e-12."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import metrics_ref as R
from detparams import det_input, det_labels, det_state_dict
from elemwise import assert_close, measure_c

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = 2.0 ** -149


def build(name):
    """(model on the device with detparams weights, input shape, tokens N, width D)."""
    if name == "latent_vit":
        from models_fer_vit.latent_vit import LatentViT

        m, shape, N, D = LatentViT(depth=2, dropout=0.0), (18, 512), 19, 512
    else:
        from models_fer_vit.image_vit import ImageViT

        m = ImageViT(img_size=48, patch_size=16, embed_dim=384, depth=2, heads=8, mlp_dim=1536, dropout=0.0)
        shape, N, D = (3, 48, 48), 10, 384
    m.load_state_dict(det_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()]))
    return m.to(DEV), shape, N, D


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
@pytest.mark.parametrize("name", ["latent_vit", "image_vit_48"])
def test_final_tokens_and_token_similarity(name, prec):
    from fervit import layers
    from fervit.explain import final_tokens, token_similarity

    m, shape, N, D = build(name)
    m.set_precision(prec)
    B = 4
    x = det_input("eval:" + name, (B, *shape)).to(DEV)
    m.train()
    t = final_tokens(m, x)
    assert m.training and layers.TOKEN_TAP is None  # mode restored, tap removed
    assert t.shape == (B, N, D) and t.dtype == (torch.bfloat16 if prec == "bf16" else torch.float32)
    cls, tok = token_similarity(m, x)
    assert cls.shape == (B, N - 1) and tok.shape == (B, N - 1, N - 1) and cls.dtype == tok.dtype == torch.float32
    v = t.float().cpu()
    rcls, rtok, scls, stok = R.cosine_ref(v.numpy(), 1e-8)
    d = v.double()
    want_cls = torch.cosine_similarity(d[:, :1], d[:, 1:], dim=2)
    want_tok = torch.cosine_similarity(d[:, 1:].unsqueeze(2), d[:, 1:].unsqueeze(1), dim=3)
    assert np.abs(rcls - want_cls.numpy()).max() <= 1e-14 and np.abs(rtok - want_tok.numpy()).max() <= 1e-14
    f_cls = torch.cosine_similarity(v[:, :1], v[:, 1:], dim=2)
    f_tok = torch.cosine_similarity(v[:, 1:].unsqueeze(2), v[:, 1:].unsqueeze(1), dim=3)
    c = measure_c(f"token_similarity {name}", prec, [(f_cls, rcls, scls), (f_tok, rtok, stok)])
    assert_close(f"{name} {prec} cls_sim", cls, want_cls, scls, c, 0.0)
    assert_close(f"{name} {prec} tok_sim", tok, want_tok, stok, c, 0.0)
    # the tap changes nothing in the forward
    m.eval()
    with torch.no_grad():
        plain = m(x)
        layers.TOKEN_TAP = lambda tt, cfg: None
        try:
            tapped = m(x)
        finally:
            layers.TOKEN_TAP = None
    assert torch.equal(plain, tapped)


def test_the_token_tap_is_eval_no_grad_and_outside_capture_only():
    from fervit import layers

    m, shape, N, D = build("latent_vit")
    x = det_input("eval:latent_vit", (4, *shape)).to(DEV)
    seen = []
    layers.TOKEN_TAP = lambda t, cfg: seen.append(t)
    try:
        m.train()
        with pytest.raises(RuntimeError, match="eval / no-grad"):  # train mode: gradients recorded
            m(x)
        m.eval()
        with pytest.raises(RuntimeError, match="eval / no-grad"):  # eval mode, grad enabled
            m(x)
        with torch.no_grad():
            m(x)  # eval, no grad: allowed (and the warm-up of the capture below)
            assert len(seen) == 1
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with pytest.raises(RuntimeError, match="eval / no-grad"):  # under capture
                with torch.cuda.graph(g):
                    m(x)
        torch.cuda.synchronize()
        assert len(seen) == 1
    finally:
        layers.TOKEN_TAP = None


CHILD = r"""
import json, sys
sys.path[:0] = [{pkg!r}, {golden!r}, {tests!r}]
import torch
from detparams import det_input
from test_gpu_eval_models import build
out = {{}}
for name in ("latent_vit", "image_vit_48"):
    m, shape, N, D = build(name)
    m.eval()
    x = det_input("eval:" + name, (4, *shape)).cuda()
    with torch.no_grad():
        before = m(x).clone()
    assert "fervit.explain" not in sys.modules
    from fervit import layers
    assert layers.TOKEN_TAP is None
    import fervit.explain as E
    cls, tok = E.token_similarity(m, x)
    with torch.no_grad():
        after = m(x)
    out[name] = [bool(torch.equal(before, after)), layers.TOKEN_TAP is None, list(cls.shape)]
    del sys.modules["fervit.explain"]
print("RESULT " + json.dumps(out))
"""


def test_logits_with_the_tap_unset_equal_a_run_before_explain_was_imported():
    """A fresh process (this one may have imported fervit.explain long ago): logits before the import, then
    the import and a tapped forward, then logits again: bit-identical."""
    code = CHILD.format(pkg=os.path.join(ROOT, "fer-vit_amd"), golden=os.path.join(ROOT, "tests", "golden"),
                        tests=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    out = json.loads(line[len("RESULT "):])
    assert out == {"latent_vit": [True, True, [4, 18]], "image_vit_48": [True, True, [4, 9]]}, out


@pytest.mark.parametrize("name", ["latent_vit", "image_vit_48"])
def test_evaluate_model_over_a_loader_with_a_short_last_batch(name):
    from eval.evaluate_model import classification_summary, evaluate_model
    from fervit.loss import CrossEntropyLoss
    from fervit.metrics import ClassificationMeter
    from train.common import run_evaluate

    m, shape, N, D = build(name)
    xs = det_input("evalloader:" + name, (19, *shape))
    ys = det_labels("evalloader:" + name, 19)
    loader = [(xs[0:8], ys[0:8]), (xs[8:16], ys[8:16]), (xs[16:19], ys[16:19])]
    meter = ClassificationMeter(7, DEV)
    res = evaluate_model(m, loader, DEV, meter)
    assert set(res) == {"predictions", "labels", "probabilities"}
    assert res["predictions"].dtype == np.int64 and res["probabilities"].dtype == np.float32
    assert res["probabilities"].shape == (19, 7) and np.array_equal(res["labels"], ys.numpy())
    with torch.no_grad():
        logits = torch.cat([m(x.to(DEV)) for x, _ in loader]).float().cpu()
    assert res["predictions"].tolist() == logits.argmax(1).tolist()
    ref, scale = R.softmax_ref(logits.numpy())
    c = measure_c(f"evaluate_model softmax {name}", "fp32", [(torch.softmax(logits, 1), ref, scale, TINY)])
    assert_close(f"{name} probabilities", torch.from_numpy(res["probabilities"]), ref, scale, c, 0.0, extra=TINY)
    got = meter.compute()
    want = run_evaluate(m, loader, CrossEntropyLoss(), DEV)
    assert got["n"] == 19 and got["skipped"] == 0
    assert abs(got["accuracy"] - want["accuracy"]) <= 1e-12 and abs(got["f1_macro"] - want["f1_macro"]) <= 1e-12
    assert abs(got["f1_weighted"] - want["f1_weighted"]) <= 1e-12
    assert want["predictions"] == res["predictions"].tolist()
    s = classification_summary(meter, ["Angry", "Disgust", "Fear", "Happy", "Neutral", "Sad", "Surprise"])
    assert s["test_dataset_size"] == 19 and s["accuracy"] == got["accuracy"]
    assert s["classification_report"]["macro avg"]["f1-score"] == got["f1_macro"]
    json.dumps(s)  # what the reference writes to evaluation_results.json
    # a second pass without a meter of the caller's gives the same arrays
    res2 = evaluate_model(m, loader, DEV)
    assert all(np.array_equal(res[k], res2[k]) for k in res)
