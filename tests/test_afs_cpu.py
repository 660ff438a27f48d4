"""CPU checks of the AFS style extractor: the restated arithmetic (tests/afs_ref.py) against float64 autograd
and against the fixture recorded from the reference, and the native modules' constructors (no GPU here:
nothing below launches a kernel)."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import afs_ref as R


def _rand(*shape, seed=0):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape))


@pytest.mark.parametrize("act", ["lrelu", "relu"])
@pytest.mark.parametrize("train", [True, False])
def test_highway_backward_formulas_match_float64_autograd(act, train):
    G, Bn, C = 3, 5, 8
    pn, pl, pg = (_rand(G, Bn, C, seed=s).requires_grad_() for s in (1, 2, 3))
    gamma, beta = (1 + 0.1 * _rand(G, C, seed=4)).requires_grad_(), (0.1 * _rand(G, C, seed=5)).requires_grad_()
    rm, rv = 0.1 * _rand(G, C, seed=6), 0.5 + _rand(G, C, seed=7).abs()
    y, mean, rstd, _, _ = R.highway(pn, pl, pg, gamma, beta, rm, rv, train, act=act)
    dy = _rand(G, Bn, C, seed=8)
    want = torch.autograd.grad(y, (pn, pl, pg, gamma, beta), dy)
    got = R.highway_bwd(dy, pn.detach(), pl.detach(), pg.detach(), mean.detach(), rstd.detach(), gamma.detach(),
                        beta.detach(), train, act=act)
    for a, b in zip(got, want):
        assert (a - b).abs().max().item() <= 1e-12


def test_linear_adjoints_match_float64_autograd():
    G, M, N, K = 3, 5, 16, 32
    x = _rand(G, M, K, seed=1).requires_grad_()
    Ws = [_rand(G, N, K, seed=2 + s).requires_grad_() for s in range(3)]
    bs = [_rand(G, N, seed=5 + s).requires_grad_() for s in range(3)]
    dys = [_rand(G, M, N, seed=8 + s) for s in range(3)]
    ys = [R.linear(x, W, b) for W, b in zip(Ws, bs)]
    want = torch.autograd.grad(ys, [x] + Ws + bs, dys)
    assert (R.linear_dgrad(dys, [W.detach() for W in Ws]) - want[0]).abs().max().item() <= 1e-12
    for s in range(3):
        dW, db = R.linear_wgrad(dys[s], x.detach())
        assert (dW - want[1 + s]).abs().max().item() <= 1e-12 and (db - want[4 + s]).abs().max().item() <= 1e-12


def test_fixture_counts():
    fx = R.load_fixture()
    assert len(fx["sd_keys"]) == 468 and int(fx["n_params"]) == 11856384
    nbt = [fx["buf:" + k] for k in fx["sd_keys"].tolist() if k.endswith("num_batches_tracked")]
    assert len(nbt) == 36 and all(int(v) == 3 for v in nbt)


def test_float32_restatement_reproduces_the_fixture():
    """float32 on the CPU against the reference's float32 on the CPU: the two differ by summation order
    only (einsum against addmm over K <= 512, six chained stages): 1e-4 relative, 1e-5 absolute."""
    fx = R.load_fixture()
    sd, w_src, w_tgt = R.fixture_inputs(fx)
    P = {k: v.clone().requires_grad_() for k, v in sd.items() if v.dtype.is_floating_point and "running" not in k}
    buf = {k: v.clone() for k, v in sd.items() if k not in P}
    state = dict(P)
    s, t, n, loss = R.train_step(lambda w: R.forward(state, w, True, buf=buf), w_src, w_tgt)
    for got, key in ((s, "out_src"), (t, "out_tgt"), (n, "out_new")):
        torch.testing.assert_close(got.detach(), torch.from_numpy(fx[key]), rtol=1e-4, atol=1e-5)
    assert abs(loss.item() - float(fx["loss"])) < 1e-5
    loss.backward()
    R_grads = {k: p.grad for k, p in P.items()}
    from cnn_ref import check_grads

    check_grads(R_grads, fx, rel=1e-4)
    for k, v in buf.items():
        torch.testing.assert_close(v, torch.from_numpy(fx["buf:" + k]), rtol=1e-5, atol=1e-6)
    with torch.no_grad():
        ev = R.forward({k: v.detach() for k, v in P.items()}, w_src, False, buf=buf)
    torch.testing.assert_close(ev, torch.from_numpy(fx["out_eval"]), rtol=1e-4, atol=1e-5)


# ------------------------------------------------------------------ native modules: constructors
def test_state_dict_keys_shapes_and_attributes():
    from afs import StyleExtractor

    fx = R.load_fixture()
    m = StyleExtractor()
    sd = m.state_dict()
    assert list(sd.keys()) == fx["sd_keys"].tolist()
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == fx["sd_shapes"].tolist()
    assert [str(v.dtype) for v in sd.values()] == fx["sd_dtypes"].tolist()
    assert sum(p.numel() for p in m.parameters()) == int(fx["n_params"])
    assert m.n_layers == 18 and len(m.blocks) == 18 and len(m.blocks[0].highways) == 2
    hw = m.blocks[0].highways[0]
    assert isinstance(hw.act, nn.LeakyReLU) and hw.act.negative_slope == 0.2
    assert isinstance(hw.nonlinear[1], nn.BatchNorm1d) and hw.nonlinear[1].momentum == 0.1


def test_same_seed_gives_the_parameters_of_the_plain_torch_construction():
    """The default initialisers consume the RNG in the reference's construction order: Linear, then per
    highway layer Linear, BatchNorm1d, Linear, Linear, then Linear, block after block."""
    from afs import StyleExtractor

    torch.manual_seed(3)
    m = StyleExtractor(n_layers=2, latent_dim=64, mid_dim=32, num_highway=2, act="relu", momentum=0.2)
    torch.manual_seed(3)
    plain = []
    for _ in range(2):
        plain.append(nn.Linear(64, 32))
        for _ in range(2):
            plain += [nn.Linear(32, 32), nn.BatchNorm1d(32, momentum=0.2), nn.Linear(32, 32), nn.Linear(32, 32)]
        plain.append(nn.Linear(32, 64))
    want = [p for mod in plain for p in mod.parameters()]
    got = list(m.parameters())
    assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))
    assert isinstance(m.blocks[1].highways[1].act, nn.ReLU) and m.blocks[0].highways[0].nonlinear[1].momentum == 0.2


def test_unknown_activation_raises_the_reference_error():
    from afs.style_extractor import HighwayLayer, StyleBlock, StyleExtractor

    for make in (lambda: HighwayLayer(8, act="gelu"), lambda: StyleBlock(16, 8, act="gelu"),
                 lambda: StyleExtractor(n_layers=1, latent_dim=16, mid_dim=8, act="gelu")):
        with pytest.raises(ValueError, match="Unknown activation 'gelu': choose 'relu' or 'lrelu'"):
            make()


def test_batchnorm_buffers_are_module_buffers_on_one_backing_store():
    from afs import StyleExtractor

    m = StyleExtractor(n_layers=3, latent_dim=64, mid_dim=32)
    assert m._bound()
    sd = R.det_state([(k, tuple(v.shape)) for k, v in m.state_dict().items()])
    m.load_state_dict(sd)
    assert m._bound()
    bn = m.blocks[2].highways[1].nonlinear[1]
    assert torch.equal(bn.running_var, sd["blocks.2.highways.1.nonlinear.1.running_var"])
    assert torch.equal(m._afs_store[1][1, 2], bn.running_var)
    m.double().float()  # _apply replaces every buffer: the store is rebuilt with the values kept
    assert m._bound() and torch.equal(m.blocks[2].highways[1].nonlinear[1].running_var,
                                      sd["blocks.2.highways.1.nonlinear.1.running_var"])
    assert int(m.blocks[0].highways[0].nonlinear[1].num_batches_tracked) == 0


@pytest.mark.parametrize("name,dep", [("AFSLoss", "ArcFace"), ("GeneratedImageProvider", "StyleGAN2"),
                                      ("DiskImageProvider", "pSp"), ("PairLatentDataset", "pSp")])
def test_unprovided_symbols_name_the_missing_dependency(name, dep):
    import afs

    assert afs.__all__ == ["StyleExtractor"]
    with pytest.raises(ImportError, match=dep):
        getattr(afs, name)
    with pytest.raises(AttributeError):
        afs.no_such_thing
