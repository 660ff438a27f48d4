"""A replayed training step with dropout against the float64 reference.

fervit.graph.StepGraph captures one step of a two-layer ImageViT (layer_ref.IMAGE_VIT_CASES[0]: B = 5, 10 tokens,
D 96, p = 0.1, nine dropout sites) and replays it three times, with FlatParams, the weight-gradient stream, the
deferred reductions and FusedAdamW.freeze_for_graph all real. lr = 0 and weight_decay = 0 keep the weights, and
so the reference, the same in every replay.

The masks of a replay exist only on the device: every captured launch keeps its host seed (the warm-up step draws
seeds 1 to 9, the capture 10 to 18) and mixes the device counter into it, and fer_step_advance is the first node
of the graph (fervit/graph.py: it is enqueued on the capture stream ahead of step_fn), so replay r runs with the
counter at r. The reference of replay r is layer_ref.run_case with the masks of dropmask.step_seed(seed_{10+i}, r).

Gate: layer_ref.compare on the logits and every parameter gradient, read after each replay from the parameters'
.grad, which the captured step leaves as the views into the flat gradient buffer (the capture does not re-home
them: step_fn's zero_grad(set_to_none) drops them and the captured backward attaches FlatParams.grad_views, whose
memory the replays write). c: layer_ref.replay_c_table, measured on the CPU (tests/test_step_seed_cpu.py).

The test can fail: the reference built from the unmixed seeds 10 to 18 falls outside the gate for replay 1, and
the reference of replay 1 fails against replay 2. After release() an eager step matches the reference of the
plain seeds 1 to 9 again: the counter is unregistered in every code object."""
import pytest
import torch

import fervit
import layer_ref as L
from fervit import runtime
from fervit.graph import StepGraph
from fervit.optim import FusedAdamW
from test_gpu_layers_elementwise import build

pytestmark = pytest.mark.gpu

DEV = "cuda"
CASE = L.IMAGE_VIT_CASES[0]
DRAWN, REPLAYS = 9, 3  # warmup=1 draws nine host seeds before the capture


@pytest.fixture(scope="module")
def refs():
    def run(masks_of):
        return L.run_case(CASE, L.REF, device=DEV, masks_of=masks_of, accumulate=False)

    r = {k: run(lambda case, pas, device, k=k: L.replay_masks(case, DRAWN, k, device)) for k in range(1, REPLAYS + 1)}
    r["unmixed"] = run(lambda case, pas, device: L.case_masks(case, 1, device))  # host seeds 10 to 18 as they are
    r["plain"] = run(L.case_masks)  # host seeds 1 to 9
    return r


def grads_and(out, named):
    got = {k: v.grad.clone() for k, v in named.items()}
    got["out"] = out.detach().clone()
    return got


@pytest.mark.parametrize("dtype", CASE.dtypes)
def test_replayed_step_with_dropout(dtype, refs):
    c, own = L.replay_c_table(CASE, DRAWN, REPLAYS)[dtype]
    x0, dout0, _ = L.case_data(CASE)
    x, dout = x0.to(DEV), dout0.to(DEV)
    m = build(CASE, dtype)
    named = dict(m.named_parameters())
    opt = FusedAdamW(m.parameters(), lr=0.0, weight_decay=0.0, model=m)

    def step_fn():
        opt.zero_grad(set_to_none=True)
        out = m(x)
        out.backward(dout)
        opt.step()
        return out

    fervit.manual_seed(CASE.seed)
    sg = StepGraph(step_fn, opt, warmup=1)
    try:
        sg.capture()
        assert runtime.SEEDS.counter == 2 * DRAWN
        flat = m.fer_flat()
        for k, v in named.items():
            assert v.grad is not None and v.grad.data_ptr() == flat.grad_views[id(v)].data_ptr(), \
                f"{k}: .grad is not its view into the flat gradient buffer after the capture"
        got = {}
        for r in range(1, REPLAYS + 1):
            out = sg.replay()
            torch.cuda.synchronize()
            assert int(sg.counter.item()) == r, f"replay {r} leaves the device counter at {int(sg.counter.item())}"
            got[r] = grads_and(out, named)
    finally:
        sg.release()
        torch.cuda.synchronize()
    worst = {}
    for r in range(1, REPLAYS + 1):
        L.compare(f"replay {r} {dtype}", got[r], refs[r], c, dtype, worst=worst)
    k = max(worst, key=worst.get)
    print(f"worst err/bound replayed {CASE.id} {dtype}: {worst[k]:.3f} ({k}), c = {c:.1f} (own measurement {own:.1f})")
    for name in sorted(worst):
        print(f"  err/bound {dtype} {name}: {worst[name]:.3f}")
    with pytest.raises(AssertionError):  # the unmixed host seeds of the captured pass are not what a replay uses
        L.compare(f"replay 1 {dtype} against seeds 10 to 18 unmixed", got[1], refs["unmixed"], c, dtype)
    with pytest.raises(AssertionError):  # nor does replay 2 repeat replay 1
        L.compare(f"replay 2 {dtype} against the reference of replay 1", got[2], refs[1], c, dtype)

    # released: an eager step draws seeds 1 to 9 again and no kernel mixes a counter into them
    fervit.manual_seed(CASE.seed)
    opt.zero_grad(set_to_none=True)
    out = m(x)
    out.backward(dout)
    torch.cuda.synchronize()
    assert runtime.SEEDS.counter == DRAWN
    w = L.compare(f"eager step after release {dtype}", grads_and(out, named), refs["plain"],
                  L.c_table(CASE.kind, CASE.act)[dtype], dtype)
    k = max(w, key=w.get)
    print(f"worst err/bound after release {CASE.id} {dtype}: {w[k]:.3f} ({k})")
