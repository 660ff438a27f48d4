"""LatentCNN2D on the GPU against the fixture recorded from the reference
(tests/golden/make_cnn_2d_golden.py), plus the model-level behaviour around Dropout2d, BatchNorm's buffers,
the trainer and graph capture; the counterpart of tests/test_gpu_latent_cnn_deep.py.

fp32 path: logits within 1e-3 and identical argmax (the project's bar), loss, every gradient checksum,
the buffers after the step (num_batches_tracked included), the AdamW step and the eval logits.
bf16 path: the gate is not taken from the kernels. tests/cnn2d_ref.py runs on the CPU with the weights
and every stored activation rounded to bf16 where the native path stores bf16; the gate is 4x the error
of that run against the fixture logits (the project's factor for measured bounds). Both values are printed
(`bf16-gate 2d` lines; DESIGN.md section 2.3 has them).
Dropout: a train step at dropout 0.3 in fp32 equals the restatement fed the keep masks rebuilt on the host
from the step's seeds (tests/dropmask.py), within the fp32 test's tolerances."""
import numpy as np
import pytest
import torch

import cnn2d_ref as D2
import cnn_ref as R
from dropmask import keep_mask

pytestmark = pytest.mark.gpu


def build(dropout=0.0, prec="fp32", load=True):
    from models_fer_vit.latent_cnn import LatentCNN2D

    m = LatentCNN2D(dropout=dropout)
    fx = R.load_fixture("2d")
    sd, x, y = D2.fixture_inputs(fx)
    if load:
        m.load_state_dict(sd)
    m = m.cuda()
    m.set_precision(prec)
    return m, fx, sd, x.cuda(), y.cuda()


def buffers(m):
    return {k: v.detach().clone() for k, v in m.named_buffers()}


def test_fp32_path_matches_the_reference_step():
    from fervit.optim import FusedAdamW

    m, fx, sd, x, y = build()
    m.train()
    opt = FusedAdamW(m.parameters(), lr=1e-3, weight_decay=0.05, model=m)
    logits = m(x)
    loss = torch.nn.functional.cross_entropy(logits, y, label_smoothing=0.1)
    loss.backward()
    lg, ref = logits.detach().cpu().numpy(), fx["logits"]
    print(f"fp32 2d: max|logits - ref| = {np.abs(lg - ref).max():.3e}")
    assert logits.dtype == torch.float32 and np.abs(lg - ref).max() < 1e-3
    assert (lg.argmax(1) == ref.argmax(1)).all()
    assert abs(loss.item() - float(fx["loss"])) < 1e-4
    R.check_grads({k: p.grad for k, p in m.named_parameters()}, fx, rel=2e-3)
    own = buffers(m)
    assert len(own) == 12
    for k, v in own.items():
        want = torch.from_numpy(fx["buf:" + k])
        if k.endswith("num_batches_tracked"):
            assert v.dtype == torch.int64 and int(v) == int(want) == 1, k
        else:
            assert torch.allclose(v.cpu(), want, rtol=1e-5, atol=1e-6), k
    opt.step()
    top = float(fx["grad_l2"].max())
    params = dict(m.named_parameters())
    for k, l2, samp, idx in zip(fx["grad_keys"].tolist(), fx["grad_l2"], fx["adamw_samples"], fx["grad_idx"]):
        if l2 < 1e-4 * top:
            continue  # gradient exactly 0 in real arithmetic (bias before BatchNorm): AdamW's g / |g| of noise
        ok = idx >= 0
        got = params[k].detach().reshape(-1).double().cpu().numpy()[idx[ok]]
        # first step: p (1 - lr wd) - lr g / (|g| + eps); a 2e-3 relative gradient error moves it by << 1e-6
        np.testing.assert_allclose(got, samp[ok], atol=2e-6, rtol=0, err_msg=k)
    ev = dict(sd)
    ev.update({k: v.cpu() for k, v in own.items()})
    m.load_state_dict(ev)
    m.eval()
    with torch.no_grad():
        le = m(x).cpu().numpy()
    assert np.abs(le - fx["logits_eval"]).max() < 1e-3
    assert (le.argmax(1) == fx["logits_eval"].argmax(1)).all()
    assert all(int(v) == 1 for k, v in m.named_buffers() if k.endswith("num_batches_tracked"))


def test_bf16_path_within_the_measured_gate():
    m, fx, sd, x, y = build(prec="bf16")
    ref = torch.from_numpy(fx["logits"])
    with torch.no_grad():
        cpu_bf, _ = D2.forward_2d(sd, x.cpu(), train=True, rnd=R.bf16_round)
    measured = (cpu_bf - ref).abs().max().item()
    gate = 4.0 * measured
    m.train()
    with torch.no_grad():
        lg = m(x).float().cpu()
    err = (lg - ref).abs().max().item()
    print(f"bf16-gate 2d: cpu-bf16-rounded error {measured:.4e} gate {gate:.4e} native error {err:.4e} "
          f"max|ref| {ref.abs().max().item():.3f}")
    assert err <= gate
    m.load_state_dict(sd)  # the train-mode forward above moved the running statistics
    m.eval()
    with torch.no_grad():
        cpu_ev, _ = D2.forward_2d(sd, x.cpu(), train=False, rnd=R.bf16_round)
        ref_ev, _ = D2.forward_2d(sd, x.cpu(), train=False)
        le = m(x).float().cpu()
    g_ev = 4.0 * (cpu_ev - ref_ev).abs().max().item()
    e_ev = (le - ref_ev).abs().max().item()
    print(f"bf16-gate 2d eval: gate {g_ev:.4e} native error {e_ev:.4e}")
    assert e_ev <= g_ev


def test_dropout_step_equals_the_restatement_with_the_rebuilt_masks():
    """dropout 0.3, fp32: Dropout2d(0.15), Dropout2d(0.15), Dropout2d(0.3) draw per (sample, channel), the
    classifier's Dropout(0.3) per element; the four seeds are the step's next_seed() values in forward order."""
    from fervit import runtime

    m, fx, sd, x, y = build(dropout=0.3)
    m.train()
    runtime.manual_seed(1234)
    logits = m(x)
    loss = torch.nn.functional.cross_entropy(logits, y, label_smoothing=0.1)
    loss.backward()
    runtime.manual_seed(1234)
    seeds = [runtime.next_seed() for _ in range(4)]
    B = x.shape[0]
    keeps = []
    for seed, C, p in zip(seeds, (64, 128, 256, 256), (0.15, 0.15, 0.3, 0.3)):
        k = keep_mask(seed, (B, C), p)
        assert not k.all() and k.any()
        keeps.append((k, float(np.float32(1.0 / (1.0 - p)))))
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items() if v.is_floating_point() and "running_" not in k}
    state = dict(sd)
    state.update(params)
    lg_ref, buf = D2.forward_2d(state, x.cpu(), train=True, keeps=keeps)
    loss_ref = R.loss_fn(lg_ref, y.cpu())
    loss_ref.backward()
    err = (logits.detach().cpu() - lg_ref.detach()).abs().max().item()
    print(f"dropout 2d: max|logits - restatement| = {err:.3e}")
    assert err < 1e-3 and abs(loss.item() - loss_ref.item()) < 1e-4
    # and the masks matter: without them the restatement is somewhere else
    lg_plain, _ = D2.forward_2d(sd, x.cpu(), train=True)
    assert (lg_plain - lg_ref.detach()).abs().max().item() > 20 * max(err, 1e-5)
    top = max(p.grad.norm().item() for p in params.values())
    for k, p in m.named_parameters():
        ref = params[k].grad.double()
        got = p.grad.detach().cpu().double()
        if ref.norm().item() < 1e-4 * top:
            assert got.norm().item() < 1e-4 * top, k
            continue
        assert (got - ref).norm().item() <= 2e-3 * ref.norm().item(), (k, (got - ref).norm().item(), ref.norm().item())
    for k, v in m.named_buffers():
        if not k.endswith("num_batches_tracked"):
            assert torch.allclose(v.cpu(), buf[k].detach(), rtol=1e-5, atol=1e-6), k


def _batches(n=3, b=8):
    g = torch.Generator().manual_seed(5)
    return [(torch.randn(b, 18, 512, generator=g), torch.randint(0, 7, (b,), generator=g)) for _ in range(n)]


def test_train_epoch_equals_a_hand_written_loop():
    """train.train_latent_cnn.train_epoch = mixup step + a metric forward under model.train(): bit for
    bit the same parameters and buffers as the same calls written out, num_batches_tracked == 6."""
    from fervit.loss import CrossEntropyLoss
    from fervit.optim import FusedAdamW
    from train.train_latent_cnn import train_epoch

    dev = torch.device("cuda")
    crit = CrossEntropyLoss()
    ma, *_ = build(prec="bf16")
    mb, *_ = build(prec="bf16")
    oa = FusedAdamW(ma.parameters(), lr=1e-4, weight_decay=1e-2, model=ma)
    ob = FusedAdamW(mb.parameters(), lr=1e-4, weight_decay=1e-2, model=mb)
    data = _batches()
    np.random.seed(7)
    torch.manual_seed(7)
    loss_a, acc, f1 = train_epoch(ma, data, oa, crit, dev)
    np.random.seed(7)
    torch.manual_seed(7)
    mb.train()
    total = 0.0
    for x, y in data:
        x, y = x.to(dev), y.to(dev)
        lam = np.random.beta(1.0, 1.0)
        index = torch.randperm(x.size(0)).to(dev)
        ob.zero_grad()
        logits = mb(lam * x + (1 - lam) * x[index])
        loss = lam * crit(logits, y) + (1 - lam) * crit(logits, y[index])
        loss.backward()
        ob.step()
        total += loss.item() * x.size(0)
        with torch.no_grad():
            mb(x)
    assert abs(loss_a - total / 24) < 1e-6 and 0.0 <= acc <= 1.0 and 0.0 <= f1 <= 1.0
    for (k, pa), (_, pb) in zip(ma.state_dict().items(), mb.state_dict().items()):
        assert torch.equal(pa, pb), k
    nbt = [int(v) for k, v in ma.named_buffers() if k.endswith("num_batches_tracked")]
    assert len(nbt) == 4 and all(n == 6 for n in nbt)


def test_fp32_model_trains_through_train_epoch():
    from fervit.loss import CrossEntropyLoss
    from fervit.optim import FusedAdamW
    from train.train_latent_cnn import evaluate, train_epoch

    m, *_ = build(dropout=0.3, prec="fp32")
    o = FusedAdamW(m.parameters(), lr=1e-4, weight_decay=1e-2, model=m)
    before = m.features[0].weight.detach().clone()
    loss, acc, f1 = train_epoch(m, _batches(2), o, CrossEntropyLoss(), torch.device("cuda"))
    assert np.isfinite(loss) and 0.0 <= acc <= 1.0
    assert not torch.equal(before, m.features[0].weight.detach())
    assert all(torch.isfinite(p).all() for p in m.parameters())
    out = evaluate(m, _batches(1), CrossEntropyLoss(), torch.device("cuda"))
    assert np.isfinite(out["loss"]) and 0.0 <= out["accuracy"] <= 1.0 and len(out["predictions"]) == 8


def _step_fn(m, o, crit, x, y):
    def step():
        o.zero_grad(set_to_none=True)
        loss = crit(m(x), y)
        loss.backward()
        o.step()
        return loss

    return step


def test_step_graph_replay_equals_eager_steps():
    from fervit.graph import StepGraph
    from fervit.loss import CrossEntropyLoss
    from fervit.optim import FusedAdamW

    crit = CrossEntropyLoss(label_smoothing=0.1)
    x, y = (t.cuda() for t in _batches(1, 16)[0])
    ma, *_ = build(prec="bf16")
    mb, *_ = build(prec="bf16")
    oa = FusedAdamW(ma.parameters(), lr=1e-3, weight_decay=0.05, model=ma)
    ob = FusedAdamW(mb.parameters(), lr=1e-3, weight_decay=0.05, model=mb)
    ea = _step_fn(ma, oa, crit, x, y)
    eager = [ea().item() for _ in range(5)]
    sg = StepGraph(_step_fn(mb, ob, crit, x, y), ob, warmup=2).capture()
    try:
        graphed = [sg.replay().clone().item() for _ in range(3)]
    finally:
        sg.release()
    assert graphed == pytest.approx(eager[2:], rel=0, abs=1e-6)
    for (k, pa), (_, pb) in zip(ma.state_dict().items(), mb.state_dict().items()):
        if k.endswith("num_batches_tracked"):
            assert int(pa) == int(pb) == 5, k
        else:
            assert (pa.float() - pb.float()).abs().max().item() <= 1e-6, k


def test_step_graph_replays_draw_fresh_channel_masks():
    from fervit.graph import StepGraph
    from fervit.loss import CrossEntropyLoss
    from fervit.optim import FusedAdamW

    crit = CrossEntropyLoss(label_smoothing=0.1)
    x, y = (t.cuda() for t in _batches(1, 16)[0])
    m, *_ = build(dropout=0.3, prec="bf16")
    m.classifier[4].p = 0.0  # Dropout2d alone: the losses can differ only through the channel masks
    o = FusedAdamW(m.parameters(), lr=0.0, weight_decay=0.0, model=m)
    sg = StepGraph(_step_fn(m, o, crit, x, y), o, warmup=1).capture()
    try:
        losses = [sg.replay().item() for _ in range(3)]
    finally:
        sg.release()
    assert len(set(losses)) == 3
    assert all(int(v) == 4 for k, v in m.named_buffers() if k.endswith("num_batches_tracked"))


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_one_sample_eval_forward(prec):
    m, fx, sd, x, y = build(prec=prec)
    m.eval()
    with torch.no_grad():
        one, four = m(x[:1]), m(x)
    assert one.shape == (1, 7) and torch.isfinite(one).all()
    assert (one - four[:1]).abs().max().item() < (1e-5 if prec == "fp32" else 5e-2)
    m.train()  # B = 1 still has 9216 values per channel in the features; the classifier's BatchNorm1d has one
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        m(x[:1])
