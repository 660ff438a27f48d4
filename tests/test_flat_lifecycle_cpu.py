"""Host logic of the flat parameter store, on CPU tensors (no GPU, no built library).

FlatParams constructs on CPU tensors; the one kernel its shadow needs (`ops.cast_bf16`) is replaced by
`out.copy_(x)`, which rounds fp32 to bf16 the same way (round to nearest even). Checked here:
  * the bf16 shadow after every kind of parameter edit (the scenarios of tests/test_gpu_flat_lifecycle.py,
    at the FlatParams level: begin_pass, bf16, half_view);
  * the gradient side channel (grad_target, attach, settle_grads) against torch's semantics;
  * what FerModule and FusedAdamW do with a store across no-op / real conversions, deep copies and rebuilds.
"""
import copy

import pytest
import torch
import torch.nn as nn

from fervit import ops
from fervit.module import FerModule
from fervit.optim import FusedAdamW
from fervit.runtime import ALIGN, FlatParams


class Net(FerModule):
    def __init__(self):
        super().__init__()
        self.a = nn.Linear(5, 3)       # 15 + 3 elements: neither a multiple of the 64-element alignment
        self.b = nn.Linear(3, 70)      # 210 elements: more than one aligned slot
        self.scale = nn.Parameter(torch.ones(1))


def slots_of(m):
    return [(s._parameters, n, p) for s in m.modules() for n, p in s._parameters.items() if p is not None]


@pytest.fixture
def casts(monkeypatch):
    calls = []

    def cast(x, out=None):
        calls.append(1)
        return out.copy_(x)

    monkeypatch.setattr(ops, "cast_bf16", cast)
    return calls


def build(seed=0):
    torch.manual_seed(seed)
    m = Net()
    flat = FlatParams(list(m.parameters()), slots_of(m))
    object.__setattr__(m, "_fer_flat", flat)
    return m, flat


def assert_shadow_fresh(flat):
    for p in flat.params:
        assert p.data_ptr() == flat.view(p).data_ptr()
        h = flat.half_view(p)
        assert h.dtype == torch.bfloat16
        assert torch.equal(h.view(torch.int16), p.detach().to(torch.bfloat16).view(torch.int16))


def test_constructs_on_cpu_and_aliases_parameters(casts):
    m, flat = build()
    want = sum((p.numel() + ALIGN - 1) // ALIGN * ALIGN for p in m.parameters())
    assert flat.numel == want and flat.data.device.type == "cpu"
    lo, hi = flat.data.data_ptr(), flat.data.data_ptr() + 4 * flat.numel
    for p in m.parameters():
        assert lo <= p.data_ptr() < hi and flat.offsets[id(p)] % ALIGN == 0
    assert flat.begin_pass()
    assert_shadow_fresh(flat)


def _sgd(m, ps):
    for p in ps:
        p.grad = torch.full_like(p, 0.25)
    torch.optim.SGD(ps, lr=0.5).step()


def _edited_state(m, names):
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    for n in names:
        sd[n] = sd[n] * 1.5 + 0.125
    return sd


# kind -> (edit(m, flat, [weight, bias]), the host can see it without being told)
EDITS = {
    "no_grad_mul_": (lambda m, ps: [p.mul_(1.5) for p in ps], True),
    "nn_init_normal_": (lambda m, ps: [nn.init.normal_(p) for p in ps], True),
    "sgd_step": (_sgd, True),
    "load_state_dict": (lambda m, ps: m.load_state_dict(_edited_state(m, ["b.weight", "b.bias"])), True),
    "load_state_dict_assign": (lambda m, ps: m.load_state_dict(_edited_state(m, ["b.weight", "b.bias"]), assign=True),
                               True),
    "data_mul_": (lambda m, ps: [p.data.mul_(1.5) for p in ps], False),
    "data_copy_": (lambda m, ps: [p.data.copy_(torch.randn(p.shape)) for p in ps], False),
    "data_assign": (lambda m, ps: [setattr(p, "data", torch.randn(p.shape)) for p in ps], True),
}


@pytest.mark.parametrize("kind", list(EDITS))
def test_shadow_follows_every_kind_of_edit(casts, kind):
    m, flat = build()
    flat.begin_pass()
    assert_shadow_fresh(flat)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    n0 = len(casts)
    flat.begin_pass()
    flat.bf16()
    assert len(casts) == n0, "an unchanged model must not cast again"

    edit, visible = EDITS[kind]
    with torch.no_grad():
        edit(m, [m.b.weight, m.b.bias])
    assert not torch.equal(m.b.weight.detach(), before["b.weight"]) and not torch.equal(m.b.bias.detach(),
                                                                                         before["b.bias"])
    assert torch.equal(m.a.weight.detach(), before["a.weight"])
    if not visible:
        m.fer_params_changed()  # in-place writes through .data leave no trace: the documented call
    ok = flat.begin_pass()
    if kind == "load_state_dict_assign":
        assert not ok, "replaced Parameter objects must make the owner rebuild the store"
        flat = FlatParams(list(m.parameters()), slots_of(m))
        assert flat.begin_pass()
    else:
        assert ok
    assert_shadow_fresh(flat)
    assert len(casts) > n0
    for n, p in m.named_parameters():  # the edit itself survived re-pointing / rebuilding
        if n not in ("b.weight", "b.bias"):
            assert torch.equal(p.detach(), before[n]), n


def test_data_assign_of_another_dtype_or_shape_is_not_adopted(casts):
    for t in (torch.randn(70, 3, dtype=torch.float64), torch.randn(3, 70)):
        m, flat = build()
        m.b.weight.data = t
        assert not flat.begin_pass()


# ---------------------------------------------------------------- gradient side channel
def test_grad_none_overwrites(casts):
    m, flat = build()
    p = m.b.weight
    gv, acc = flat.grad_target(p)
    assert acc is False and gv.data_ptr() == flat.grad_views[id(p)].data_ptr() and gv.shape == p.shape
    gv.fill_(2.0)
    flat.attach(p)
    assert p.grad.data_ptr() == gv.data_ptr() and torch.equal(p.grad, torch.full_like(p, 2.0))


def test_grad_that_is_our_view_accumulates(casts):
    m, flat = build()
    p = m.b.weight
    flat.grad_target(p)[0].fill_(2.0)
    flat.attach(p)
    held = p.grad
    gv, acc = flat.grad_target(p)
    assert acc is True and torch.equal(gv, torch.full_like(p, 2.0))
    flat.attach(p)
    assert p.grad is held  # attach leaves our own view in place


def test_foreign_grad_is_copied_in_then_accumulated(casts):
    m, flat = build()
    p = m.b.weight
    flat.grad_target(p)[0].fill_(7.0)  # stale content of the slot must not survive
    foreign = torch.randn(p.shape)
    p.grad = foreign.clone()
    gv, acc = flat.grad_target(p)
    assert acc is True and torch.equal(gv, foreign)
    gv.add_(1.0)  # what an accumulating kernel does
    flat.attach(p)
    assert p.grad.data_ptr() == gv.data_ptr() and torch.equal(p.grad, foreign + 1.0)


def test_zero_grad_in_place_keeps_the_view_and_accumulates_onto_zero(casts):
    m, flat = build()
    for p in m.parameters():
        flat.grad_target(p)[0].fill_(3.0)
        flat.attach(p)
    torch.optim.SGD(m.parameters(), lr=0.1).zero_grad(set_to_none=False)
    assert not flat.grad.any()
    for p in m.parameters():
        gv, acc = flat.grad_target(p)
        assert acc is True and p.grad.data_ptr() == gv.data_ptr() and not gv.any()


def test_settle_grads_follows_torch(casts):
    m, flat = build()
    w, b, s = m.b.weight, m.b.bias, m.scale
    for p in (w, b, s):
        flat.grad_target(p)[0].fill_(3.0)
        flat.attach(p)
    w.grad = None                      # dropped by zero_grad(set_to_none=True): contributes nothing
    foreign = torch.randn(b.shape)
    b.grad = foreign.clone()           # assigned by user code: its values count
    flat.settle_grads()
    assert not flat.grad_views[id(w)].any()
    assert torch.equal(flat.grad_views[id(b)], foreign)
    assert torch.equal(flat.grad_views[id(s)], torch.full_like(s, 3.0))
    assert not flat.grad_views[id(m.a.weight)].any()  # never written


# ---------------------------------------------------------------- module and optimizer around the store
def test_noop_conversions_keep_the_store_and_real_ones_drop_it(casts):
    m, flat = build()
    assert m.float() is m and m._fer_flat is flat
    assert m.to("cpu") is m and m._fer_flat is flat
    assert m.to(torch.float32) is m and m._fer_flat is flat
    m.double()
    assert m._fer_flat is None
    m.float()
    assert m._fer_flat is None  # nothing to keep: the next forward rebuilds
    m, flat = build()
    m.b.weight.data = torch.randn(70, 3)  # re-pointed and not yet adopted: not the flat view any more
    m.float()
    assert m._fer_flat is None


def test_deepcopy_owns_its_storage_and_no_store(casts):
    m, flat = build()
    flat.begin_pass()
    flat.bf16()
    c = copy.deepcopy(m)
    assert type(c) is Net and c._fer_flat is None and c._fer_owner is None
    lo, hi = flat.data.data_ptr(), flat.data.data_ptr() + 4 * flat.numel
    for (n, p), (nc, pc) in zip(m.named_parameters(), c.named_parameters()):
        assert n == nc and pc is not p and torch.equal(pc.detach(), p.detach())
        assert not lo <= pc.data_ptr() < hi
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(1.5)
    assert not torch.equal(c.b.weight.detach(), m.b.weight.detach())


def test_fused_adamw_keeps_moments_when_the_store_is_rebuilt(casts):
    m, flat = build()
    opt = FusedAdamW(m.parameters(), lr=1e-3, model=m)
    assert opt._bind() is flat
    opt._m.copy_(torch.arange(flat.numel, dtype=torch.float32))
    opt._v.copy_(torch.arange(flat.numel, dtype=torch.float32) * 0.5)
    want = {id(p): (flat.view(p, opt._m).clone(), flat.view(p, opt._v).clone()) for p in flat.params}
    assert opt._bind() is flat and opt._m[5] == 5.0  # same store: untouched

    # rebuilt over the same Parameter objects in another order (other offsets): carried per parameter
    new = FlatParams(list(m.parameters())[::-1], slots_of(m))
    object.__setattr__(m, "_fer_flat", new)
    assert opt._bind() is new
    for p in m.parameters():
        assert torch.equal(new.view(p, opt._m), want[id(p)][0])
        assert torch.equal(new.view(p, opt._v), want[id(p)][1])

    # a replaced Parameter object starts from zero moments, the others keep theirs
    m.scale = nn.Parameter(torch.ones(1))
    assert not new.begin_pass()
    newer = FlatParams(list(m.parameters()), slots_of(m))
    object.__setattr__(m, "_fer_flat", newer)
    assert opt._bind() is newer
    assert not newer.view(m.scale, opt._m).any()
    assert torch.equal(newer.view(m.b.weight, opt._m), want[id(m.b.weight)][0])
