"""CPU checks of the LatentCNN baseline: the constructors' state_dict (keys, shapes, dtypes, parameter
counts) and attributes against the fixtures recorded from the reference, and tests/cnn_ref.py -- the
plain-torch restatement the GPU tests compare the kernels with -- against the same fixtures."""
import pytest
import torch
import torch.nn as nn

import cnn_ref as R
from models_fer_vit.latent_cnn import (LatentCNN, LatentCNNLight, LatentConv1D, LatentResBlock1D,
                                       create_latent_cnn)

KINDS = ("standard", "light")
COUNTS = {"standard": (57, 6_566_919), "light": (25, 987_783)}


@pytest.mark.parametrize("kind", KINDS)
def test_state_dict_matches_the_reference(kind):
    fx = R.load_fixture(kind)
    m = create_latent_cnn(kind)
    sd = m.state_dict()
    assert list(sd.keys()) == fx["sd_keys"].tolist()
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == fx["sd_shapes"].tolist()
    assert [str(v.dtype) for v in sd.values()] == fx["sd_dtypes"].tolist()
    n = sum(p.numel() for p in m.parameters())
    assert (len(sd), n) == COUNTS[kind] and n == int(fx["n_params"])
    nbt = [k for k in sd if k.endswith("num_batches_tracked")]
    assert nbt and all(sd[k].dtype == torch.int64 and sd[k].dim() == 0 for k in nbt)
    assert any(k.endswith("running_mean") for k in sd) and any(k.endswith("running_var") for k in sd)
    # buffers are ordinary torch buffers, not parameters
    assert {k for k, _ in m.named_buffers()} == {k for k in sd if "running_" in k or k.endswith("tracked")}


def test_constructor_attributes():
    m = create_latent_cnn("standard", dropout=0.25)
    assert isinstance(m, LatentCNN) and (m.latent_dim, m.seq_len, m.use_residual, m.use_max_pool) == (512, 18, True, False)
    assert len(m.conv_layers) == 4 and len(m.res_blocks) == 2
    blk = m.conv_layers[0]
    assert isinstance(blk, LatentConv1D) and isinstance(blk.conv, nn.Conv1d) and blk.conv.bias is None
    assert isinstance(blk.bn, nn.BatchNorm1d) and isinstance(blk.relu, nn.ReLU) and blk.dropout.p == 0.25
    rb = m.res_blocks[1]
    assert isinstance(rb, LatentResBlock1D) and rb.conv1.bias is None and rb.conv2.kernel_size == (3,)
    assert rb.dropout.p == 0.25 and isinstance(m.global_avg_pool, nn.AdaptiveAvgPool1d)
    assert [type(c) for c in m.classifier] == [nn.Flatten, nn.Linear, nn.BatchNorm1d, nn.ReLU, nn.Dropout, nn.Linear]
    assert LatentConv1D(8, 8, dropout=0.0).dropout is None and LatentResBlock1D(8, dropout=0.0).dropout is None
    m2 = LatentCNN(latent_dim=64, seq_len=5, num_classes=3, hidden_dims=[32, 16], use_residual=False)
    assert not hasattr(m2, "res_blocks") and m2.classifier[1].in_features == 16 and m2.classifier[5].out_features == 3
    lt = create_latent_cnn("light")
    assert isinstance(lt, LatentCNNLight) and lt.encoder[0].bias is not None and len(lt.encoder) == 11
    assert isinstance(lt.pool, nn.AdaptiveAvgPool1d) and lt.classifier[4].out_features == 7
    with pytest.raises(ValueError):
        create_latent_cnn("nope")


@pytest.mark.parametrize("kind", KINDS)
def test_initialisation(kind):
    torch.manual_seed(3)
    m = create_latent_cnn(kind)
    for mod in m.modules():
        if isinstance(mod, nn.BatchNorm1d):
            assert (mod.weight == 1).all() and (mod.bias == 0).all() and int(mod.num_batches_tracked) == 0
        elif isinstance(mod, nn.Linear):
            assert (mod.bias == 0).all() and 0.008 < mod.weight.std().item() < 0.012
        elif isinstance(mod, nn.Conv1d):  # kaiming_normal_(fan_out, relu): std = sqrt(2 / (Cout * 3))
            want = (2.0 / (mod.out_channels * 3)) ** 0.5
            assert abs(mod.weight.std().item() / want - 1) < 0.05


def test_reference_operators_are_consistent():
    """cnn_ref's hand-written backward formulas against torch autograd of its forwards, in float64."""
    torch.manual_seed(0)
    B, L, C = 3, 5, 8
    x = torch.randn(B * L, C, dtype=torch.float64, requires_grad=True)
    dcols = torch.randn(B * L, 3 * C, dtype=torch.float64)
    (R.conv1d_cols(x, B, L) * dcols).sum().backward()
    assert torch.allclose(x.grad, R.conv1d_cols_bwd(dcols, B, L), atol=1e-12)
    # the second sample's first row must not see the first sample's last row
    cols = R.conv1d_cols(x.detach(), B, L).reshape(B, L, C, 3)
    assert (cols[1, 0, :, 0] == 0).all() and (cols[0, L - 1, :, 2] == 0).all()
    assert torch.equal(cols[1, 1, :, 0], x.detach().reshape(B, L, C)[1, 0])
    for train in (True, False):
        for use_res in (False, True):
            xx = torch.randn(B * L, C, dtype=torch.float64, requires_grad=True)
            g = torch.randn(C, dtype=torch.float64, requires_grad=True)
            b = torch.randn(C, dtype=torch.float64, requires_grad=True)
            res = torch.randn(B * L, C, dtype=torch.float64, requires_grad=True) if use_res else None
            rm, rv = torch.randn(C, dtype=torch.float64), torch.rand(C, dtype=torch.float64) + 0.5
            keep = torch.rand(B * L, C) > 0.3
            dy = torch.randn(B * L, C, dtype=torch.float64)
            y, mean, rstd, _, _ = R.batchnorm(xx, g, b, rm, rv, train, res=res, relu=True, keep=keep, scale=1 / 0.7)
            (y * dy).sum().backward()
            dx, dres, dg, db = R.batchnorm_bwd(dy, xx.detach(), mean.detach(), rstd.detach(), g.detach(), b.detach(),
                                               train, res=None if res is None else res.detach(), relu=True,
                                               keep=keep, scale=1 / 0.7)
            assert torch.allclose(dx, xx.grad, atol=1e-10) and torch.allclose(dg, g.grad, atol=1e-10)
            assert torch.allclose(db, b.grad, atol=1e-10)
            if use_res:
                assert torch.allclose(dres, res.grad, atol=1e-10)


@pytest.mark.parametrize("kind", KINDS)
def test_cnn_ref_float32_reproduces_the_fixture(kind):
    """tests/cnn_ref.py in float32 on the CPU against the reference's recorded step: logits, loss,
    gradient checksums, buffers after the step and the eval logits with those buffers."""
    fx = R.load_fixture(kind)
    sd, x, labels = R.fixture_inputs(kind, fx)
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items() if v.is_floating_point() and "running_" not in k}
    state = dict(sd)
    state.update(params)
    lg, buf = R.forward(kind, state, x, train=True)
    loss = R.loss_fn(lg, labels)
    loss.backward()
    assert (lg.detach() - torch.from_numpy(fx["logits"])).abs().max().item() < 1e-4
    assert torch.equal(lg.detach().argmax(1), torch.from_numpy(fx["logits"]).argmax(1))
    assert abs(loss.item() - float(fx["loss"])) < 1e-5
    R.check_grads({k: p.grad for k, p in params.items()}, fx, rel=1e-3)
    for k, v in buf.items():
        ref = torch.from_numpy(fx["buf:" + k])
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(ref) == 1
        else:
            assert torch.allclose(v, ref, rtol=1e-5, atol=1e-6), k
    ev = dict(sd)
    ev.update({k: v.detach() for k, v in buf.items()})
    le, buf2 = R.forward(kind, ev, x, train=False)
    assert (le - torch.from_numpy(fx["logits_eval"])).abs().max().item() < 1e-4
    assert all(int(v) == 1 for k, v in buf2.items() if k.endswith("num_batches_tracked"))
