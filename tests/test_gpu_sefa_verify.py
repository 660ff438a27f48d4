"""fervit.sefa.verify_non_expression_directions end to end: LatentViT(depth=2) (the smallest one
tests/test_gpu_models.py builds) on the fp32 path, 6 samples, 3 directions, the five default steps, against
predictions from the CPU oracle (oracle/vit_oracle.py latent_vit_forward on the same deterministic weights).

A (direction, sample) pair is compared only if the base row and every shifted row of it have a top-2 logit
margin above 2 x 1e-3 in the oracle (1e-3 is the gate test_gpu_models.py holds this model's fp32 logits to:
two logits each off by that much cannot swap places across a wider gap); at most 10% of the pairs may be left
out. SEED was picked on the CPU, from the oracle alone, among 0..7 as the one with the widest smallest margin
(0.050, 25 times the threshold): the oracle leaves out no pair, direction 1 needs one doubling of its scale
before a label changes, and it then changes 3 of the 6 samples.

Direction 0 is the zero vector (rate exactly 0); direction 1 is doubled until the oracle changes a label."""
import pytest
import torch

import vit_oracle as O
from detparams import det_input, det_state_dict
from fervit import sefa

pytestmark = pytest.mark.gpu

SEED = 4
N, K, HEADS, DEPTH = 6, 3, 8, 2
STEPS = [-3.0, -1.5, 0.0, 1.5, 3.0]
NONZERO = [s for s in STEPS if s != 0.0]
MARGIN = 2 * 1e-3


@pytest.fixture(scope="module")
def setup():
    from models_fer_vit.latent_vit import LatentViT

    m = LatentViT(depth=DEPTH, dropout=0.0)
    sd = det_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], SEED)
    m.load_state_dict(sd)
    m = m.cuda()
    m.set_precision("fp32")
    x = det_input("sefa_verify", (N, 18, 512), SEED)
    d = det_input("sefa_verify_dirs", (K, 512), SEED)
    d = d / d.norm(dim=1, keepdim=True)
    d[0] = 0
    base = O.latent_vit_forward(x, sd, HEADS, DEPTH)

    def shifted(dirs):  # rows (direction, step, sample), the reference's w + step * direction
        return O.latent_vit_forward(torch.cat([x + s * dk[None, None] for dk in dirs for s in NONZERO], 0), sd, HEADS,
                                    DEPTH)

    scale = 1.0
    while not (shifted([d[1] * scale]).argmax(1).reshape(len(NONZERO), N) != base.argmax(1)[None]).any():
        scale *= 2.0
        assert scale <= 4096.0
    d[1] *= scale
    lg = shifted(d)
    top = torch.cat([base, lg]).topk(2, 1).values
    margin = top[:, 0] - top[:, 1]
    wide = (margin[N:].reshape(K, len(NONZERO), N) > MARGIN).all(1) & (margin[:N] > MARGIN)[None]   # [K, N]
    preds = lg.argmax(1).reshape(K, len(NONZERO), N)
    return dict(model=m, x=x, dirs=d, base=base.argmax(1), preds=preds, wide=wide,
                changed=(preds != base.argmax(1)[None, None]).any(1))


def test_change_rates_equal_the_oracle(setup):
    s = setup
    wide, want = s["wide"], s["changed"]
    assert (~wide).sum().item() <= 0.1 * K * N, "more than 10% of the pairs are too close to call"
    assert want[1].any() and not want[0].any()
    r = sefa.label_changes_along_directions(s["dirs"].numpy(), s["x"], s["model"], STEPS)
    assert r["steps"] == NONZERO and r["n"] == N
    assert torch.equal(r["base_preds"].cpu()[wide.all(0)], s["base"][wide.all(0)])
    got_changed, got_preds = r["changed"].cpu().bool(), r["preds"].cpu()
    assert torch.equal(got_changed[wide], want[wide])
    sel = wide[:, None, :].expand(K, len(NONZERO), N)
    assert torch.equal(got_preds[sel], s["preds"][sel])
    assert torch.equal(r["counts"].cpu(), got_changed.sum(1))
    assert torch.equal(r["step_counts"].cpu(), (got_preds != r["base_preds"].cpu()[None, None]).sum(2))

    res = sefa.verify_non_expression_directions(s["dirs"].numpy(), s["x"], s["model"], None, STEPS, verbose=False)
    assert [e["direction_idx"] for e in res] == [0, 1, 2]
    assert res[0]["label_change_rate"] == 0.0 and all(v == 0.0 for v in res[0]["step_change_rate"].values())
    assert res[1]["label_change_rate"] > 0.0
    assert list(res[1]["step_change_rate"]) == NONZERO
    if wide.all():
        for k in range(K):
            assert res[k]["label_change_rate"] == int(want[k].sum()) / N
            for j, st in enumerate(NONZERO):
                assert res[k]["step_change_rate"][st] == int((s["preds"][k, j] != s["base"]).sum()) / N
    assert sefa.select_directions(res, 0.0)[0] == 0 and 1 not in sefa.select_directions(res, 0.0)


def test_chunking_gives_the_same_bits(setup):
    """batch_size = 4 * 6: one direction per chunk; 4 * 2: samples in blocks of 2 as well; 1: one direction and one
    sample per forward. preds, changed and both counts are the same bits as from one chunk."""
    s = setup
    one = sefa.label_changes_along_directions(s["dirs"], s["x"], s["model"], STEPS, batch_size=1024)
    for bs in (len(NONZERO) * N, len(NONZERO) * 2, 1):
        r = sefa.label_changes_along_directions(s["dirs"], s["x"], s["model"], STEPS, batch_size=bs)
        for key in ("base_preds", "preds", "changed", "counts", "step_counts"):
            assert torch.equal(r[key], one[key]), (bs, key)


def test_max_samples_takes_the_first_samples(setup):
    s = setup
    r4 = sefa.label_changes_along_directions(s["dirs"], s["x"], s["model"], STEPS, max_samples=4)
    rf = sefa.label_changes_along_directions(s["dirs"], s["x"][:4], s["model"], STEPS, max_samples=None)
    every = sefa.label_changes_along_directions(s["dirs"], s["x"], s["model"], STEPS, max_samples=None)
    assert r4["n"] == 4 and every["n"] == N
    for key in ("preds", "changed", "counts", "step_counts"):
        assert torch.equal(r4[key], rf[key]), key
    assert torch.equal(r4["preds"], every["preds"][:, :, :4]) and torch.equal(r4["changed"], every["changed"][:, :4])
    res = sefa.verify_non_expression_directions(s["dirs"], s["x"], s["model"], max_samples=4, verbose=False)
    assert [e["label_change_rate"] for e in res] == [c / 4 for c in r4["counts"].tolist()]


def test_w_plus_directions_and_zero_steps(setup):
    """[K, L, D] directions that repeat the [K, D] ones over the layers give the same bits; with only zero
    steps nothing is launched and every rate is 0."""
    s = setup
    a = sefa.label_changes_along_directions(s["dirs"], s["x"], s["model"], STEPS)
    b = sefa.label_changes_along_directions(s["dirs"][:, None, :].expand(K, 18, 512), s["x"], s["model"], STEPS)
    for key in ("preds", "changed", "counts", "step_counts"):
        assert torch.equal(a[key], b[key]), key
    res = sefa.verify_non_expression_directions(s["dirs"], s["x"], s["model"], step_sizes=[0.0], verbose=False)
    assert [e["label_change_rate"] for e in res] == [0.0, 0.0, 0.0]
