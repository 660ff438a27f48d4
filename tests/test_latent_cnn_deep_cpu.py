"""CPU checks of LatentCNNDeep: the constructor's state_dict (keys, shapes, dtypes, parameter count),
attributes and initialisation against the fixture recorded from the reference
(tests/golden/make_cnn_deep_golden.py), and tests/cnn_deep_ref.py -- the plain-torch restatement the GPU
tests compare the kernels with -- against the same fixture and against float64 autograd."""
import pytest
import torch
import torch.nn as nn

import cnn_deep_ref as D
import cnn_ref as R
from models_fer_vit.latent_cnn import LatentCNNDeep, LatentConv1D, LatentResBlock1D, create_latent_cnn

COUNTS = (81, 5_913_608)


def test_state_dict_matches_the_reference():
    fx = R.load_fixture("deep")
    m = create_latent_cnn("deep")
    sd = m.state_dict()
    assert list(sd.keys()) == fx["sd_keys"].tolist()
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == fx["sd_shapes"].tolist()
    assert [str(v.dtype) for v in sd.values()] == fx["sd_dtypes"].tolist()
    n = sum(p.numel() for p in m.parameters())
    assert (len(sd), n) == COUNTS and n == int(fx["n_params"])
    assert fx["ln_prefixes"].tolist() == ["input_proj.1."]
    nbt = [k for k in sd if k.endswith("num_batches_tracked")]
    assert len(nbt) == 12 and all(sd[k].dtype == torch.int64 and sd[k].dim() == 0 for k in nbt)
    assert {k for k, _ in m.named_buffers()} == {k for k in sd if "running_" in k or k.endswith("tracked")}
    assert tuple(sd["attention.0.weight"].shape) == (1, 512, 1) and tuple(sd["attention.0.bias"].shape) == (1,)


def test_fixture_meets_the_recording_rules():
    fx = R.load_fixture("deep")
    assert fx["logits"].shape == (4, 7) and fx["attn"].shape == (4, 18)
    assert min(fx["margin"].min(), fx["margin_eval"].min()) >= 1e-2
    assert fx["attn"].max(1).min() >= 2.0 / 18 and abs(fx["attn"].sum(1) - 1).max() < 1e-5


def test_constructor_attributes():
    m = create_latent_cnn("deep", dropout=0.25)
    assert isinstance(m, LatentCNNDeep) and (m.latent_dim, m.seq_len) == (512, 18)
    assert [n for n, _ in m.named_children()] == ["input_proj", "conv_block1", "conv_block2", "conv_block3",
                                                  "attention", "classifier"]
    assert [type(c) for c in m.input_proj] == [nn.Linear, nn.LayerNorm, nn.ReLU, nn.Dropout]
    assert m.input_proj[3].p == 0.125 and m.input_proj[0].out_features == 256
    assert m.input_proj[1].normalized_shape == (256,)
    for blk, cin, cout, n in ((m.conv_block1, 256, 256, 2), (m.conv_block2, 256, 384, 2), (m.conv_block3, 384, 512, 3)):
        assert [type(c) for c in blk] == [LatentConv1D] + [LatentResBlock1D] * (n - 1)
        assert (blk[0].conv.in_channels, blk[0].conv.out_channels) == (cin, cout) and blk[0].dropout.p == 0.25
        assert all(r.conv1.in_channels == cout and r.dropout.p == 0.25 for r in blk[1:])
    assert [type(c) for c in m.attention] == [nn.Conv1d, nn.Softmax]
    att = m.attention[0]
    assert (att.in_channels, att.out_channels, att.kernel_size) == (512, 1, (1,)) and att.bias is not None
    assert m.attention[1].dim == 2
    assert [type(c) for c in m.classifier] == [nn.Linear, nn.BatchNorm1d, nn.ReLU, nn.Dropout, nn.Linear]
    assert m.classifier[3].p == 0.25 and m.classifier[4].out_features == 7
    m2 = LatentCNNDeep(latent_dim=64, seq_len=5, num_classes=3, dropout=0.0)
    assert m2.input_proj[0].in_features == 64 and m2.classifier[4].out_features == 3 and m2.input_proj[3].p == 0.0


def test_initialisation():
    torch.manual_seed(3)
    m = create_latent_cnn("deep")
    seen_ln = 0
    for mod in m.modules():
        if isinstance(mod, (nn.BatchNorm1d, nn.LayerNorm)):
            assert (mod.weight == 1).all() and (mod.bias == 0).all()
            seen_ln += isinstance(mod, nn.LayerNorm)
        elif isinstance(mod, nn.Linear):
            assert (mod.bias == 0).all() and 0.008 < mod.weight.std().item() < 0.012
        elif isinstance(mod, nn.Conv1d):  # kaiming_normal_(fan_out, relu): std = sqrt(2 / (Cout * k))
            want = (2.0 / (mod.out_channels * mod.kernel_size[0])) ** 0.5
            assert abs(mod.weight.std().item() / want - 1) < 0.1
            assert mod.bias is None or (mod.bias == 0).all()
    assert seen_ln == 1 and (m.attention[0].bias == 0).all()


def test_same_seed_gives_the_same_parameters():
    """The constructor consumes the RNG in a fixed order: two builds from one seed are identical."""
    torch.manual_seed(11)
    a = create_latent_cnn("deep").state_dict()
    torch.manual_seed(11)
    b = create_latent_cnn("deep").state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("shape", [(3, 5, 8), (2, 1, 8), (1, 18, 24)])
def test_attnpool_backward_formulas_against_autograd(shape):
    B, L, C = shape
    g = torch.Generator().manual_seed(B * 100 + L)
    f64 = torch.float64
    x = torch.randn(B * L, C, dtype=f64, generator=g).requires_grad_(True)
    w = torch.randn(C, dtype=f64, generator=g).requires_grad_(True)
    b = torch.randn(1, dtype=f64, generator=g).requires_grad_(True)
    dy = torch.randn(B, C, dtype=f64, generator=g)
    y, a = D.attnpool(x, w, b, B, L)
    (y * dy).sum().backward()
    dx, dw_part, db_part, da, ds = D.attnpool_bwd(dy, x.detach(), w.detach(), a.detach(), B, L)
    assert torch.allclose(dx, x.grad, atol=1e-12) and torch.allclose(dw_part.sum(0), w.grad, atol=1e-12)
    assert torch.allclose(db_part.sum(), b.grad.reshape(()), atol=1e-12) and b.grad.abs().max().item() < 1e-12
    assert torch.allclose(a.sum(1), torch.ones(B, dtype=f64), atol=1e-14)
    if L == 1:  # softmax of one score is 1: ds is exactly 0 and dx is dy
        assert (a == 1).all() and (ds == 0).all() and torch.equal(dx, dy)


def test_attnpool_one_hot():
    """A score far above the others: the pool returns that row and only its row receives dy."""
    B, L, C = 2, 6, 8
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B * L, C, dtype=torch.float64, generator=g)
    w = torch.zeros(C, dtype=torch.float64)
    w[0] = 1.0
    x[:, 0] = 0.0
    x[2, 0] = x[L + 4, 0] = 1000.0
    y, a = D.attnpool(x, w, None, B, L)
    assert torch.equal(a.argmax(1), torch.tensor([2, 4])) and (a.max(1).values == 1).all()
    assert torch.equal(y, x[[2, L + 4]])
    dy = torch.randn(B, C, dtype=torch.float64, generator=g)
    dx, _, db, _, ds = D.attnpool_bwd(dy, x, w, a, B, L)
    assert (ds == 0).all() and (db == 0).all()
    want = torch.zeros_like(x)
    want[2], want[L + 4] = dy[0], dy[1]
    assert torch.equal(dx, want)


def test_forward_deep_float32_reproduces_the_fixture():
    """tests/cnn_deep_ref.py in float32 on the CPU against the reference's recorded step: logits, loss,
    gradient checksums, buffers after the step, the attention weights and the eval logits."""
    fx = R.load_fixture("deep")
    sd, x, labels = D.fixture_inputs(fx)
    assert torch.equal(labels, torch.from_numpy(fx["labels"]))
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items() if v.is_floating_point() and "running_" not in k}
    state = dict(sd)
    state.update(params)
    lg, buf, attn = D.forward_deep(state, x, train=True)
    loss = R.loss_fn(lg, labels)
    loss.backward()
    assert (lg.detach() - torch.from_numpy(fx["logits"])).abs().max().item() < 1e-4
    assert torch.equal(lg.detach().argmax(1), torch.from_numpy(fx["logits"]).argmax(1))
    assert abs(loss.item() - float(fx["loss"])) < 1e-5
    assert (attn.detach() - torch.from_numpy(fx["attn"])).abs().max().item() < 1e-6
    R.check_grads({k: p.grad for k, p in params.items()}, fx, rel=1e-3)
    assert len(buf) == 36
    for k, v in buf.items():
        ref = torch.from_numpy(fx["buf:" + k])
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(ref) == 1
        else:
            assert torch.allclose(v, ref, rtol=1e-5, atol=1e-6), k
    ev = dict(sd)
    ev.update({k: v.detach() for k, v in buf.items()})
    le, buf2, _ = D.forward_deep(ev, x, train=False)
    assert (le - torch.from_numpy(fx["logits_eval"])).abs().max().item() < 1e-4
    assert all(int(v) == 1 for k, v in buf2.items() if k.endswith("num_batches_tracked"))


def test_attention_scores_must_be_a_pointwise_conv():
    from models_fer_vit.latent_cnn import _check_attention

    _check_attention(nn.Conv1d(512, 1, kernel_size=1), 512)
    for bad in (nn.Conv1d(512, 1, kernel_size=3, padding=1), nn.Conv1d(512, 2, kernel_size=1),
                nn.Conv1d(512, 1, kernel_size=1, stride=2), nn.Conv1d(256, 1, kernel_size=1), nn.Linear(512, 1)):
        with pytest.raises(NotImplementedError, match="attention pooling"):
            _check_attention(bad, 512)


def test_2d_is_still_not_implemented():
    with pytest.raises(NotImplementedError, match="2d"):
        create_latent_cnn("2d")
    with pytest.raises(ValueError):
        create_latent_cnn("nope")
