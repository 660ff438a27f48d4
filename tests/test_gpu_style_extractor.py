"""The native AFS StyleExtractor against the fixture recorded from the reference
(tests/golden/afs_style_extractor.npz: the trainer's three forwards and one backward at B = 4) and against
the restated arithmetic of tests/afs_ref.py.

fp32 path, the gate of the fp32 LatentCNN model tests: outputs within 1e-3, loss within 1e-4, every
gradient checksum within 2e-3 relative, buffers rtol 1e-5 / atol 1e-6, one FusedAdamW step within 2e-6.
bf16 path: see BF16_MEASURED below."""
import numpy as np
import pytest
import torch

import afs_ref as R
from cnn_ref import check_grads, sample_idx

pytestmark = pytest.mark.gpu
DEV = "cuda"

# max |bf16 output - fp32 output| of the three-call step at the fixture's state, measured once on an MI355X:
# out_src 0.0198, out_tgt 0.0207, out_new 0.0334 (outputs are O(1), max |out_new| = 2.8; five bf16-stored
# stages behind each output). The gate is twice the largest.
BF16_MEASURED = 0.0334
BF16_GATE = 2 * BF16_MEASURED


def build(prec="fp32", **kw):
    from afs import StyleExtractor

    fx = R.load_fixture()
    sd, w_src, w_tgt = R.fixture_inputs(fx)
    m = StyleExtractor(**kw)
    if not kw:
        m.load_state_dict(sd)
    m = m.to(DEV).set_precision(prec)
    return m, fx, sd, w_src.to(DEV), w_tgt.to(DEV)


@pytest.fixture(scope="module")
def fp32_step():
    """The three-call step in fp32, shared by the tests that only read it."""
    from fervit.optim import FusedAdamW

    m, fx, sd, w_src, w_tgt = build("fp32")
    m.train()
    s, t, n, loss = R.train_step(m, w_src, w_tgt)
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    bufs = {k: v.detach().clone() for k, v in m.named_buffers()}
    opt = FusedAdamW(m.parameters(), lr=1e-3, weight_decay=0.05, model=m)
    opt.step()
    torch.cuda.synchronize()
    return dict(m=m, fx=fx, sd=sd, w_src=w_src, outs=(s.detach(), t.detach(), n.detach()), loss=loss.item(),
                grads=grads, bufs=bufs)


def test_fp32_outputs_loss_and_gradients_match_the_fixture(fp32_step):
    fx = fp32_step["fx"]
    for got, key in zip(fp32_step["outs"], ("out_src", "out_tgt", "out_new")):
        err = np.abs(got.float().cpu().numpy() - fx[key]).max()
        print(f"fp32 {key}: max error {err:.3e}")
        assert err < 1e-3, key
    assert abs(fp32_step["loss"] - float(fx["loss"])) < 1e-4
    check_grads(fp32_step["grads"], fx, rel=2e-3)


def test_buffers_after_the_three_call_step(fp32_step):
    fx = fp32_step["fx"]
    assert len(fp32_step["bufs"]) == 108
    for k, v in fp32_step["bufs"].items():
        want = torch.from_numpy(fx["buf:" + k])
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(want) == 3, k
        else:
            assert torch.allclose(v.cpu(), want, rtol=1e-5, atol=1e-6), k


def test_fused_adamw_step_matches_the_fixture_and_afs_ref(fp32_step):
    """Sampled parameters after one FusedAdamW step against (a) the reference followed by torch.optim.AdamW
    (the fixture) and (b) afs_ref in float32 on the CPU followed by torch.optim.AdamW, flat atol 2e-6. First
    step: p (1 - lr wd) - lr g / (|g| + eps); a 2e-3 relative gradient error moves it by << 1e-6."""
    fx, sd = fp32_step["fx"], fp32_step["sd"]
    P = {k: v.clone().requires_grad_() for k, v in sd.items() if v.dtype.is_floating_point and "running" not in k}
    buf = {k: v.clone() for k, v in sd.items() if k not in P}
    w_src, w_tgt = R.fixture_inputs(fx)[1:]
    loss = R.train_step(lambda w: R.forward(P, w, True, buf=buf), w_src, w_tgt)[3]
    loss.backward()
    torch.optim.AdamW(list(P.values()), lr=1e-3, weight_decay=0.05).step()
    top = float(fx["grad_l2"].max())
    now = dict(fp32_step["m"].named_parameters())
    # The flat 2e-6 gate presumes |g| >> Adam's eps = 1e-8: the step's sensitivity is lr eps / (|g| + eps)^2 per
    # unit of gradient error, which at |g| ~ eps turns float32 rounding of the gradient into 1e-6-sized moves
    # (float32 torch on the CPU is itself 4.7e-7 off the fixture at the |g| = 7.6e-9 sample of
    # blocks.15.highways.0.nonlinear.1.bias). Samples with |g| < G_MIN = 1e-6 (100 eps) are therefore not compared
    # with the two references; they are held to the same 2e-6 against Adam's formula applied, in float64, to
    # the native gradient itself. About 4 % of the fixture's samples are that small.
    G_MIN, lr, wd, eps = 1e-6, 1e-3, 0.05, 1e-8
    compared = small = 0
    for k, l2, samp, gref in zip(fx["grad_keys"].tolist(), fx["grad_l2"], fx["adamw_samples"], fx["grad_samples"]):
        if l2 < 1e-4 * top:
            continue  # a bias in front of a train-mode BatchNorm: its gradient is rounding noise, Adam amplifies it
        idx = sample_idx(k, now[k].numel())
        got = now[k].detach().reshape(-1)[idx].double().cpu().numpy()
        big = np.abs(gref[: len(idx)]) >= G_MIN
        mine = P[k].detach().reshape(-1)[idx].double().numpy()
        np.testing.assert_allclose(got[big], samp[: len(idx)][big], atol=2e-6, rtol=0, err_msg=k + " (fixture)")
        np.testing.assert_allclose(got[big], mine[big], atol=2e-6, rtol=0, err_msg=k + " (afs_ref)")
        g = fp32_step["grads"][k].reshape(-1)[idx].double().cpu().numpy()
        p0 = sd[k].reshape(-1)[idx].double().numpy()
        formula = p0 * (1 - lr * wd) - lr * g / (np.abs(g) + eps)
        np.testing.assert_allclose(got[~big], formula[~big], atol=2e-6, rtol=0, err_msg=k + " (Adam on the native g)")
        compared += int(big.sum())
        small += int((~big).sum())
    print(f"adamw samples: {compared} against the references, {small} below |g| = {G_MIN:g} against the formula")
    assert compared >= 0.9 * (compared + small) and compared > 2000


def test_eval_output_matches_the_fixture():
    m, fx, sd, w_src, _ = build("fp32")
    ev = dict(sd)
    ev.update({k[4:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("buf:")})
    m.load_state_dict(ev)
    m.eval()
    with torch.no_grad():
        got = m(w_src)
    assert np.abs(got.cpu().numpy() - fx["out_eval"]).max() < 1e-3
    assert all(int(v) == 3 for k, v in m.named_buffers() if k.endswith("num_batches_tracked"))


def test_bf16_step_within_twice_the_measured_error(fp32_step):
    m, fx, sd, w_src, w_tgt = build("bf16")
    m.train()
    outs = R.train_step(m, w_src, w_tgt)
    outs[3].backward()
    for got, ref, key in zip(outs[:3], fp32_step["outs"], ("out_src", "out_tgt", "out_new")):
        err = (got.float() - ref.float()).abs().max().item()
        print(f"bf16-measure {key}: max |bf16 - fp32| = {err:.4f}")
        assert err <= BF16_GATE, (key, err)
    assert all(torch.isfinite(p.grad).all() for p in m.parameters())
    # the gradient of the largest parameter group agrees in direction with the fp32 one
    for k in ("blocks.0.down.weight", "blocks.17.up.weight", "blocks.9.highways.1.gate.weight"):
        a, b = dict(m.named_parameters())[k].grad.reshape(-1), fp32_step["grads"][k].reshape(-1)
        assert torch.nn.functional.cosine_similarity(a, b, dim=0).item() > 0.99, k


def test_state_dict_round_trip_under_the_reference_keys(fp32_step):
    from afs import StyleExtractor

    m, fx = fp32_step["m"], fp32_step["fx"]
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    assert list(sd) == fx["sd_keys"].tolist()
    m2 = StyleExtractor()
    m2.load_state_dict(sd)
    m2 = m2.to(DEV).set_precision("fp32").eval()
    m.eval()
    with torch.no_grad():
        assert torch.equal(m(fp32_step["w_src"]), m2(fp32_step["w_src"]))
    m.train()


@pytest.mark.parametrize("prec,tol", [("fp32", 1e-4), ("bf16", 0.06)])
@pytest.mark.parametrize("act", ["lrelu", "relu"])
def test_style_block_and_highway_layer_alone(act, prec, tol):
    """One group through the same kernels, against afs_ref in float64 (outputs are O(1); bf16: five stored
    stages at 2^-8 each, as in the model gate)."""
    from afs.style_extractor import HighwayLayer, StyleBlock

    torch.manual_seed(1)
    blk = StyleBlock(64, 32, 2, act).to(DEV).set_precision(prec).train()
    x = torch.randn(5, 64, device=DEV, requires_grad=True)
    sd = {"blocks.0." + k: v.detach().double().cpu() for k, v in blk.state_dict().items()}
    y = blk(x)
    y.sum().backward()
    xr = x.detach().double().cpu().requires_grad_()
    buf = {k: v.clone() for k, v in sd.items() if "running" in k or "num_batches" in k}
    yr = R.forward(sd, xr[:, None], True, act=act, buf=buf)[:, 0]
    yr.sum().backward()
    assert (y.detach().double().cpu() - yr.detach()).abs().max().item() < tol
    assert (x.grad.double().cpu() - xr.grad).abs().max().item() < tol * 10
    assert torch.allclose(blk.highways[1].nonlinear[1].running_var.double().cpu(),
                          buf["blocks.0.highways.1.nonlinear.1.running_var"], rtol=tol, atol=tol)
    assert int(blk.highways[0].nonlinear[1].num_batches_tracked) == 1 and blk.down.weight.grad is not None
    hw = HighwayLayer(32, act).to(DEV).set_precision(prec).train()
    h = torch.randn(6, 32, device=DEV)
    yh = hw(h)
    p = {k: v.detach().double().cpu() for k, v in hw.state_dict().items()}
    pre = [R.linear(h.double().cpu()[None], p[n + ".weight"][None], p[n + ".bias"][None])
           for n in ("nonlinear.0", "linear", "gate")]
    want = R.highway(*pre, p["nonlinear.1.weight"][None], p["nonlinear.1.bias"][None], None, None, True, act=act)[0][0]
    assert yh.shape == (6, 32) and (yh.double().cpu() - want).abs().max().item() < tol


def test_training_with_one_sample_raises_as_batchnorm_does():
    from afs import StyleExtractor

    m = StyleExtractor(n_layers=2, latent_dim=64, mid_dim=32).to(DEV).train()
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        m(torch.zeros(1, 2, 64, device=DEV))
    m.eval()
    assert m(torch.zeros(1, 2, 64, device=DEV)).shape == (1, 2, 64)


def test_a_frozen_block_receives_no_gradient():
    from afs import StyleExtractor

    torch.manual_seed(2)
    m = StyleExtractor(n_layers=3, latent_dim=64, mid_dim=32).to(DEV).set_precision("fp32").train()
    ref = StyleExtractor(n_layers=3, latent_dim=64, mid_dim=32)
    ref.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
    ref = ref.to(DEV).set_precision("fp32").train()
    for p in m.blocks[1].parameters():
        p.requires_grad_(False)
    x = torch.randn(4, 3, 64, device=DEV)
    for mod in (m, ref):
        mod(x).square().sum().backward()
    for (k, p), q in zip(m.named_parameters(), ref.parameters()):
        if k.startswith("blocks.1."):
            assert p.grad is None, k
        else:
            assert torch.equal(p.grad, q.grad), k


def test_launch_count_does_not_depend_on_the_number_of_layers(monkeypatch):
    """libfervit launches per forward and per backward, counted where ops.py checks each call's status."""
    from afs import StyleExtractor
    from fervit import ops

    count = [0]
    real = ops.check

    def counting(rc, what=""):
        count[0] += 1
        return real(rc, what)

    seen = {}
    for L in (2, 18):
        m = StyleExtractor(n_layers=L, latent_dim=64, mid_dim=32).to(DEV).train()
        x = torch.randn(4, L, 64, device=DEV)
        m(x).sum().backward()  # the first pass also builds the bf16 shadow
        with monkeypatch.context() as mp:
            mp.setattr(ops, "check", counting)
            count[0] = 0
            y = m(x)
            fwd = count[0]
            y.sum().backward()
            seen[L] = (fwd, count[0] - fwd)
    print("launches (forward, backward):", seen)
    assert seen[2] == seen[18] and seen[2][0] <= 8 and seen[2][1] <= 12
