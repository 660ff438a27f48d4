"""train.common.ReplayedTrainEpoch: a 2-layer LatentViT (18 x 512 input, D 64) at batch 8
over 7 batches -- 2 eager warm-up steps, 4 replays and a tail of 3 samples.

* Replay equals eager: the same step function run eagerly for all 7, with the counter advanced by hand and the
  captured step's host seeds drawn again, gives the same parameters and per-step losses bit for bit.
* Consecutive replays use different lam and perm, each the host mirror's draw (tests/mixup_ref.py) at its counter.
* mixup = 0.0 forces lam = 1: every step's loss is plain cross-entropy of its logits, within the bound of
  fer_cross_entropy's test (tests/test_gpu_rowops.py).
* run_epoch returns run_train_epoch's triple; close() folds the replays into the optimizer's host step counts, and
  an eager run_train_epoch on the same model carries on.
* LatentCNN 'light' through train_latent_cnn.make_replayed_epoch."""
import functools

import numpy as np
import pytest
import torch

import mixup_ref as R
from elemwise import assert_bits_equal, assert_close, measure_c

pytestmark = pytest.mark.gpu

DEV = "cuda"
BS, WARMUP, SEED = 8, 2, 77
SIZES = [8, 8, 8, 8, 8, 8, 3]


@functools.lru_cache(maxsize=None)
def batches():
    g = torch.Generator().manual_seed(5)
    return [(torch.randn(n, 18, 512, generator=g), torch.randint(0, 7, (n,), generator=g)) for n in SIZES]


def make(prec, mixup=1.0, grad_clip=1.0):
    import fervit
    from fervit.loss import CrossEntropyLoss
    from fervit.optim import FusedAdamW
    from models_fer_vit.latent_vit import LatentViT
    from train.common import ReplayedTrainEpoch

    fervit.manual_seed(SEED)
    torch.manual_seed(3)
    m = LatentViT(embed_dim=64, depth=2, heads=2, mlp_dim=128, dropout=0.1).to(DEV)
    m.set_precision(prec)
    opt = FusedAdamW(m.parameters(), lr=1e-3, weight_decay=0.05, model=m)
    crit = CrossEntropyLoss(label_smoothing=0.1)
    runner = ReplayedTrainEpoch(m, opt, crit, DEV, BS, mixup=mixup, grad_clip=grad_clip, metric_forward=True,
                                warmup=WARMUP)
    return m, opt, runner


def record(rec):
    from fervit import runtime

    def on_step(r):
        rec.append(dict(loss=r.loss.clone(), lam=r.mixup.lam.clone(), perm=r.mixup.perm.clone(),
                        logits=r.logits.clone(), y=r.y[:r.mixup.B].clone(), seeds=runtime.SEEDS.counter))
    return on_step


@functools.lru_cache(maxsize=None)
def replayed(prec, mixup=1.0):
    m, opt, runner = make(prec, mixup)
    rec = []
    try:
        triple = runner.run_epoch(batches(), on_step=record(rec))
        assert runner.graph is not None and int(runner.graph.counter.item()) == 5  # 4 replays and the tail
    finally:
        runner.close()
    torch.cuda.synchronize()
    return m, opt, runner, rec, triple


def eager(prec):
    """The runner's own step function, never captured: from the step the runner captures at, the device counter
    is registered, the optimizer frozen on it and advanced by hand, and every full batch draws the host seeds the
    capture drew."""
    from fervit import ops, runtime
    from fervit._lib import check, lib

    m, opt, ref = make(prec)
    m.train()
    losses, counter, c0 = [], None, None
    try:
        for i, (x, y) in enumerate(batches()):
            n = ref.load(x, y)
            if i == WARMUP:
                counter = torch.zeros(1, dtype=torch.int64, device=DEV)
                check(lib().fer_set_step_counter(counter.data_ptr()), "set_step_counter")
                opt.freeze_for_graph(counter)
                c0 = runtime.SEEDS.counter
            if i >= WARMUP:
                if n == BS:
                    runtime.SEEDS.counter = c0
                check(lib().fer_step_advance(counter.data_ptr(), ops.stream()), "step_advance")
            ref.step(n)
            losses.append(ref.loss.clone())
    finally:
        check(lib().fer_set_step_counter(None), "set_step_counter")
        opt.unfreeze()
    torch.cuda.synchronize()
    return m, losses


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_replay_equals_eager(prec):
    ma, _, _, rec, _ = replayed(prec)
    mb, losses = eager(prec)
    assert len(rec) == len(losses) == 7
    for i, (a, b) in enumerate(zip(rec, losses)):
        assert torch.isfinite(b).item()
        assert_bits_equal(f"{prec} loss of step {i}", a["loss"].reshape(1).cpu(), b.reshape(1).cpu())
    for (k, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        assert_bits_equal(f"{prec} {k}", pa.detach().cpu(), pb.detach().cpu())
    assert len({r["loss"].item() for r in rec}) == 7


def test_replays_draw_the_mirrors_lam_and_perm():
    """Steps 0 and 1 (eager, no counter) draw from fresh host seeds; replays 1..4 from the seed the capture drew,
    mixed with counters 1..4; the tail from a fresh seed under counter 5."""
    from fervit.runtime import _Seeds

    _, _, _, rec, _ = replayed("bf16")

    def host_seed(k):  # the k-th seed after fervit.manual_seed(SEED)
        s = _Seeds()
        s.base, s.counter = (SEED * 0x9E3779B97F4A7C15) & (2 ** 64 - 1), k - 1
        return s.next()

    per_step = rec[0]["seeds"]  # host seeds one step takes; the draw's is the first
    assert rec[1]["seeds"] == 2 * per_step and all(r["seeds"] == 3 * per_step for r in rec[2:6])
    c0 = 2 * per_step
    cases = [(0, host_seed(1), None, 8), (1, host_seed(per_step + 1), None, 8)]
    cases += [(1 + r, host_seed(c0 + 1), r, 8) for r in (1, 2, 3, 4)]
    cases += [(6, host_seed(c0 + per_step + 1), 5, 3)]
    for i, seed, counter, n in cases:
        ss = R.stream_seed(seed, 0, counter)
        want, _, margin = R.lam(ss, 1.0)
        assert (rec[i]["perm"].cpu().numpy() == R.perm(ss, n)).all(), (i, counter)
        if margin >= R.MARGIN:
            assert abs(rec[i]["lam"].item() - want) <= R.LAM_TOL, (i, counter, rec[i]["lam"].item(), want)
    for a, b in zip(rec[2:5], rec[3:6]):  # consecutive replays
        assert a["lam"].item() != b["lam"].item() and (a["perm"] != b["perm"]).any().item()


def test_lam_one_is_plain_cross_entropy():
    _, _, _, rec, _ = replayed("bf16", 0.0)
    F = torch.nn.functional
    for i, r in enumerate(rec):
        assert r["lam"].item() == 1.0
        logits, y = r["logits"].float().cpu(), r["y"].cpu()
        ref = F.cross_entropy(logits.double(), y, label_smoothing=0.1)
        f32 = F.cross_entropy(logits, y, label_smoothing=0.1)
        scale = ref.abs().reshape(1)
        c = measure_c("cross_entropy.loss", "fp32", [(f32.reshape(1), ref.reshape(1), scale)])
        assert_close(f"step {i} loss", r["loss"].reshape(1), ref.reshape(1), scale, c, 0.0)


def test_run_epoch_returns_the_triple_of_run_train_epoch():
    from sklearn.metrics import accuracy_score, f1_score

    _, _, runner, rec, triple = replayed("bf16")
    loss, acc, f1 = triple
    assert type(loss) is float and isinstance(acc, float) and isinstance(f1, float)
    last = runner.last
    labels = torch.cat([y for _, y in batches()]).tolist()
    assert last["labels"] == labels and len(last["predictions"]) == len(labels) == sum(SIZES)
    assert acc == accuracy_score(last["labels"], last["predictions"])
    assert f1 == f1_score(last["labels"], last["predictions"], average="macro")
    want = sum(r["loss"].double().item() * n for r, n in zip(rec, SIZES)) / sum(SIZES)
    assert loss == pytest.approx(want, rel=1e-12)


def test_after_close_eager_epochs_carry_on():
    from fervit.loss import CrossEntropyLoss
    from train.common import run_train_epoch

    m, opt, runner = make("bf16")
    try:
        runner.run_epoch(batches())
    finally:
        runner.close()
    assert runner.graph is None
    assert {int(v["step"]) for v in opt.state_dict()["state"].values()} == {7}
    out = run_train_epoch(m, batches()[:2], opt, CrossEntropyLoss(label_smoothing=0.1), DEV, mixup=1.0, grad_clip=1.0,
                          metric_forward=True)
    assert len(out) == 3 and np.isfinite(out[0])
    assert {int(v["step"]) for v in opt.state_dict()["state"].values()} == {9}


def test_needs_a_bound_fused_optimizer():
    from fervit.loss import CrossEntropyLoss
    from fervit.optim import FusedAdamW
    from models_fer_vit.latent_vit import LatentViT
    from train.common import ReplayedTrainEpoch

    m = LatentViT(embed_dim=64, depth=1, heads=2, mlp_dim=128).to(DEV)
    crit = CrossEntropyLoss()
    for opt in (torch.optim.AdamW(m.parameters()), FusedAdamW(m.parameters())):
        with pytest.raises(TypeError, match="FusedAdamW bound to the model"):
            ReplayedTrainEpoch(m, opt, crit, DEV, BS, mixup=1.0)


def test_latent_cnn_light_through_its_trainer():
    import fervit
    from fervit.loss import CrossEntropyLoss
    from fervit.optim import FusedAdamW
    from models_fer_vit.latent_cnn import create_latent_cnn
    from train import train_latent_cnn

    fervit.manual_seed(SEED)
    torch.manual_seed(4)
    m = create_latent_cnn("light").to(DEV)
    m.set_precision("bf16")
    opt = FusedAdamW(m.parameters(), lr=1e-3, weight_decay=0.05, model=m)
    runner = train_latent_cnn.make_replayed_epoch(m, opt, CrossEntropyLoss(label_smoothing=0.1), DEV, BS)
    rec = []
    try:
        loss, acc, f1 = runner.run_epoch(batches()[:3], on_step=record(rec))
        assert runner.graph is not None and runner.metric_forward and runner.mixup.alpha == 1.0
    finally:
        runner.close()
    assert np.isfinite(loss) and 0.0 <= acc <= 1.0 and len(rec) == 3
    assert {int(v["step"]) for v in opt.state_dict()["state"].values()} == {3}
    # two forwards under model.train() per step, as the reference's train_epoch
    assert all(int(v) == 6 for k, v in m.named_buffers() if k.endswith("num_batches_tracked"))
