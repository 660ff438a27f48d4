"""CPU checks of LatentCNN2D: the constructor's state_dict (keys, shapes, dtypes, parameter count),
attributes and initialisation against the fixture recorded from the reference
(tests/golden/make_cnn_2d_golden.py), and tests/cnn2d_ref.py -- the plain-torch restatement the GPU tests
compare the kernels with -- against the same fixture and against float64 autograd."""
import pytest
import torch
import torch.nn as nn

import cnn2d_ref as D2
import cnn_ref as R
from models_fer_vit.latent_cnn import LatentCNN2D, _check_conv2d, _check_pool2d

COUNTS = (30, 438_663)
F64 = torch.float64


def test_state_dict_matches_the_reference():
    fx = R.load_fixture("2d")
    m = LatentCNN2D()
    sd = m.state_dict()
    assert list(sd.keys()) == fx["sd_keys"].tolist()
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == fx["sd_shapes"].tolist()
    assert [str(v.dtype) for v in sd.values()] == fx["sd_dtypes"].tolist()
    n = sum(p.numel() for p in m.parameters())
    assert (len(sd), n) == COUNTS and n == int(fx["n_params"])
    nbt = [k for k in sd if k.endswith("num_batches_tracked")]
    assert len(nbt) == 4 and all(sd[k].dtype == torch.int64 and sd[k].dim() == 0 for k in nbt)
    assert tuple(sd["features.0.weight"].shape) == (64, 1, 3, 3) and tuple(sd["features.9.weight"].shape) == (256, 128, 3, 3)


def test_fixture_meets_the_recording_rules():
    fx = R.load_fixture("2d")
    assert fx["logits"].shape == (4, 7) and fx["pool_nonfirst"].shape == (2,)
    assert min(fx["margin"].min(), fx["margin_eval"].min()) >= 1e-2
    assert fx["pool_nonfirst"].min() >= 0.5
    # the restatement's pools choose the same share of non-first pixels as torch's did in the reference run
    sd, x, _ = D2.fixture_inputs(fx)
    own = D2.pool_nonfirst(sd, x)
    assert max(abs(a - b) for a, b in zip(own, fx["pool_nonfirst"].tolist())) < 1e-3, own


def test_constructor_attributes():
    m = LatentCNN2D(dropout=0.25)
    assert [n for n, _ in m.named_children()] == ["features", "gap", "classifier"]
    assert [type(c) for c in m.features] == [nn.Conv2d, nn.BatchNorm2d, nn.ReLU, nn.Dropout2d,
                                             nn.Conv2d, nn.BatchNorm2d, nn.ReLU, nn.MaxPool2d, nn.Dropout2d,
                                             nn.Conv2d, nn.BatchNorm2d, nn.ReLU, nn.MaxPool2d, nn.Dropout2d]
    assert [m.features[i].p for i in (3, 8, 13)] == [0.125, 0.125, 0.25]
    for i, cin, cout in ((0, 1, 64), (4, 64, 128), (9, 128, 256)):
        c = m.features[i]
        assert (c.in_channels, c.out_channels, c.kernel_size, c.padding) == (cin, cout, (3, 3), (1, 1))
        assert c.bias is not None and m.features[i + 1].num_features == cout
    assert all(m.features[i].kernel_size == (2, 2) for i in (7, 12))
    assert isinstance(m.gap, nn.AdaptiveAvgPool2d) and m.gap.output_size == 1
    assert [type(c) for c in m.classifier] == [nn.Flatten, nn.Linear, nn.BatchNorm1d, nn.ReLU, nn.Dropout, nn.Linear]
    assert m.classifier[4].p == 0.25 and m.classifier[1].in_features == 256 and m.classifier[5].out_features == 7
    m2 = LatentCNN2D(latent_dim=64, seq_len=5, num_classes=3, dropout=0.0)
    assert m2.classifier[5].out_features == 3 and m2.features[13].p == 0.0


def test_initialisation():
    torch.manual_seed(3)
    m = LatentCNN2D()
    for mod in m.modules():
        if isinstance(mod, (nn.BatchNorm1d, nn.BatchNorm2d)):
            assert (mod.weight == 1).all() and (mod.bias == 0).all()
        elif isinstance(mod, nn.Linear):
            assert (mod.bias == 0).all() and 0.008 < mod.weight.std().item() < 0.012
        elif isinstance(mod, nn.Conv2d):  # kaiming_normal_(fan_out, relu): std = sqrt(2 / (Cout * 9))
            want = (2.0 / (mod.out_channels * 9)) ** 0.5
            assert abs(mod.weight.std().item() / want - 1) < 0.1
            # the reference leaves Conv2d biases at nn.Conv2d's default draw: bounded by 1 / sqrt(fan_in)
            assert mod.bias.abs().max().item() <= 1.0 / (mod.in_channels * 9) ** 0.5


def test_same_seed_gives_the_same_parameters():
    torch.manual_seed(11)
    a = LatentCNN2D().state_dict()
    torch.manual_seed(11)
    b = LatentCNN2D().state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_unsupported_modules_raise():
    _check_conv2d(nn.Conv2d(8, 8, 3, padding=1))
    for bad in (nn.Conv2d(8, 8, 5, padding=2), nn.Conv2d(8, 8, 3, padding=1, stride=2), nn.Conv2d(8, 8, 3),
                nn.Conv2d(8, 8, 3, padding=2, dilation=2), nn.Conv2d(8, 8, 3, padding=1, groups=2),
                nn.Conv2d(8, 8, 3, padding=1, padding_mode="reflect"), nn.Conv1d(8, 8, 3, padding=1)):
        with pytest.raises(NotImplementedError, match="Conv2d"):
            _check_conv2d(bad)
    _check_pool2d(nn.MaxPool2d((2, 2)))
    _check_pool2d(nn.MaxPool2d(2))
    for bad in (nn.MaxPool2d(3), nn.MaxPool2d((2, 2), stride=1), nn.MaxPool2d(2, padding=1),
                nn.MaxPool2d(2, ceil_mode=True), nn.AvgPool2d(2)):
        with pytest.raises(NotImplementedError, match="MaxPool2d"):
            _check_pool2d(bad)


SHAPES = [(1, 1, 1, 8), (2, 1, 5, 8), (3, 2, 3, 4), (2, 3, 4, 8), (1, 9, 16, 4), (2, 5, 7, 4)]


@pytest.mark.parametrize("shape", SHAPES)
def test_cols_backward_against_autograd(shape):
    B, H, W, C = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(B * H * W, C, dtype=F64, generator=g).requires_grad_(True)
    d = torch.randn(B * H * W, 9 * C, dtype=F64, generator=g)
    cols = D2.conv2d_cols(x, B, H, W)
    (cols * d).sum().backward()
    assert torch.allclose(D2.conv2d_cols_bwd(d, B, H, W), x.grad, atol=1e-12)
    # the cols are nn.Conv2d's own: cols @ weight.reshape(Cout, -1).T is conv2d(x) in NHWC
    w = torch.randn(6, C, 3, 3, dtype=F64, generator=g)
    want = torch.nn.functional.conv2d(x.detach().reshape(B, H, W, C).permute(0, 3, 1, 2), w, padding=1)
    assert torch.allclose((cols.detach() @ w.reshape(6, -1).t()).reshape(B, H, W, 6), want.permute(0, 2, 3, 1), atol=1e-12)


def test_cols_hold_zeros_outside_the_image_not_the_neighbours_values():
    B, H, W, C = 2, 3, 4, 2
    x = torch.arange(1, B * H * W * C + 1, dtype=F64).reshape(B * H * W, C)  # no zero anywhere
    cols = D2.conv2d_cols(x, B, H, W).reshape(B, H, W, C, 3, 3)
    assert (cols[:, 0, :, :, 0, :] == 0).all() and (cols[:, H - 1, :, :, 2, :] == 0).all()  # first / last row
    assert (cols[:, :, 0, :, :, 0] == 0).all() and (cols[:, :, W - 1, :, :, 2] == 0).all()  # first / last column
    assert (cols[:, :, :, :, 1, 1].reshape(-1, C) == x).all()
    # the pixel left of a row's first pixel is the previous row's last in memory: it must not appear
    assert cols[0, 1, 0, 0, 1, 0] == 0 and cols[1, 0, 0, 0, 0, 1] == 0
    inside = cols[:, 1:H - 1, 1:W - 1]
    assert (inside != 0).all()


@pytest.mark.parametrize("shape", [(1, 1, 1, 8), (2, 3, 5, 8), (1, 4, 6, 4)])
def test_first_layer_backward_against_autograd(shape):
    B, H, W, Cout = shape
    g = torch.Generator().manual_seed(sum(shape) + 1)
    x = torch.randn(B * H * W, dtype=F64, generator=g).requires_grad_(True)
    w = torch.randn(Cout, 1, 3, 3, dtype=F64, generator=g).requires_grad_(True)
    b = torch.randn(Cout, dtype=F64, generator=g).requires_grad_(True)
    dy = torch.randn(B * H * W, Cout, dtype=F64, generator=g)
    y = D2.conv2d_c1(x, w, b, B, H, W)
    want = torch.nn.functional.conv2d(x.detach().reshape(B, 1, H, W), w.detach(), b.detach(), padding=1)
    assert torch.allclose(y.detach().reshape(B, H, W, Cout), want.permute(0, 2, 3, 1), atol=1e-12)
    (y * dy).sum().backward()
    dw, db, dx = D2.conv2d_c1_bwd(dy, x.detach(), w.detach(), B, H, W)
    assert torch.allclose(dw.reshape(w.shape), w.grad, atol=1e-12) and torch.allclose(db, b.grad, atol=1e-12)
    assert torch.allclose(dx, x.grad, atol=1e-12)


def _pool_input(B, H, W, C, g):
    """ReLU-like rows: about a third exact zeros, values on a coarse grid so windows tie."""
    x = (torch.randn(B * H * W, C, dtype=F64, generator=g) * 2).round() / 2
    return torch.relu(x)


@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("shape", [(1, 2, 2, 4), (3, 3, 5, 4), (2, 9, 16, 8), (2, 4, 4, 4)])
def test_pool_chdrop_backward_against_autograd(shape, pool):
    B, H, W, C = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = _pool_input(B, H, W, C, g).requires_grad_(True)
    keep = torch.rand(B, C, generator=g) > 0.4
    y = D2.pool2_chdrop(x, B, H, W, pool, keep, 1.25)
    dy = torch.randn_like(y)
    (y * dy).sum().backward()
    dx = D2.pool2_chdrop_bwd(dy, x.detach(), B, H, W, pool, keep, 1.25)
    assert torch.equal(dx, x.grad)
    xd = x.detach().reshape(B, H, W, C)
    if pool:
        Ho, Wo = H // 2, W // 2
        assert tuple(y.shape) == (B * Ho * Wo, C)
        # torch's own MaxPool2d: the same values, and its backward puts the gradient on the same pixels
        xt = xd.permute(0, 3, 1, 2).clone().requires_grad_(True)
        yt = torch.nn.functional.max_pool2d(xt, (2, 2))
        nodrop = D2.pool2_chdrop(x.detach(), B, H, W, True)
        assert torch.equal(nodrop.reshape(B, Ho, Wo, C), yt.detach().permute(0, 2, 3, 1))
        (yt * dy.reshape(B, Ho, Wo, C).permute(0, 3, 1, 2)).sum().backward()
        assert torch.equal(D2.pool2_chdrop_bwd(dy, x.detach(), B, H, W, True), xt.grad.permute(0, 2, 3, 1).reshape(-1, C))
        # the rows / columns floor division leaves out receive exactly 0
        d4 = dx.reshape(B, H, W, C)
        assert (d4[:, 2 * Ho:] == 0).all() and (d4[:, :, 2 * Wo:] == 0).all()
        # ties are present and go to the first pixel in scan order
        win = xd[:, :2 * Ho, :2 * Wo].reshape(B, Ho, 2, Wo, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(B, Ho, Wo, C, 4)
        tied = (win == win.max(-1, keepdim=True).values).sum(-1) > 1
        assert tied.any() or H * W < 16
        _, pos = D2.pool_argmax(x.detach(), B, H, W)
        assert torch.equal(pos, (win == win.max(-1, keepdim=True).values).double().argmax(-1))
    dropped = (~keep)[:, None, None, :].expand(B, H, W, C)
    assert (dx.reshape(B, H, W, C)[dropped] == 0).all()


def test_forward_2d_float32_reproduces_the_fixture():
    """tests/cnn2d_ref.py in float32 on the CPU against the reference's recorded step: logits, loss, gradient
    checksums, buffers after the step and the eval logits (the bounds of the 'deep' CPU test)."""
    fx = R.load_fixture("2d")
    sd, x, labels = D2.fixture_inputs(fx)
    assert torch.equal(labels, torch.from_numpy(fx["labels"]))
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items() if v.is_floating_point() and "running_" not in k}
    state = dict(sd)
    state.update(params)
    lg, buf = D2.forward_2d(state, x, train=True)
    loss = R.loss_fn(lg, labels)
    loss.backward()
    assert (lg.detach() - torch.from_numpy(fx["logits"])).abs().max().item() < 1e-4
    assert torch.equal(lg.detach().argmax(1), torch.from_numpy(fx["logits"]).argmax(1))
    assert abs(loss.item() - float(fx["loss"])) < 1e-5
    R.check_grads({k: p.grad for k, p in params.items()}, fx, rel=1e-3)
    assert len(buf) == 12
    for k, v in buf.items():
        ref = torch.from_numpy(fx["buf:" + k])
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(ref) == 1
        else:
            assert torch.allclose(v, ref, rtol=1e-5, atol=1e-6), k
    ev = dict(sd)
    ev.update({k: v.detach() for k, v in buf.items()})
    le, buf2 = D2.forward_2d(ev, x, train=False)
    assert (le - torch.from_numpy(fx["logits_eval"])).abs().max().item() < 1e-4
    assert all(int(v) == 1 for k, v in buf2.items() if k.endswith("num_batches_tracked"))
