"""FusedAdamW's advance-or-rebuild decision for a resident segment table (optim.SegTable.advances), on CPU
tensors: pure host logic, no device and no built library. The signatures and steps come from the optimizer's
own walk over (param group, parameter) pairs, so a changed hyper-parameter or subset is seen the way step()
and the backward hook see it.
"""
import pytest
import torch
import torch.nn as nn

from fervit.module import FerModule
from fervit.optim import FusedAdamW, SegTable
from fervit.runtime import FlatParams


class Net(FerModule):
    def __init__(self):
        super().__init__()
        self.a = nn.Linear(5, 3)
        self.b = nn.Linear(3, 70)
        self.scale = nn.Parameter(torch.ones(1))


@pytest.fixture
def setup():
    torch.manual_seed(0)
    m = Net()
    flat = FlatParams(list(m.parameters()))
    object.__setattr__(m, "_fer_flat", flat)
    for p in m.parameters():
        p.grad = flat.grad_views[id(p)]
    opt = FusedAdamW([{"params": [m.a.weight, m.a.bias, m.scale]}, {"params": [m.b.weight, m.b.bias], "lr": 3e-4}],
                     lr=1e-3, weight_decay=0.05, model=m)
    pairs = opt._pairs()
    maxn, sig, steps = opt._scan(flat, pairs, bump=True)  # the launch that left the table resident
    return m, flat, opt, pairs, SegTable(None, len(sig), maxn, pairs, sig, steps)


def test_walk_describes_every_pair(setup):
    m, flat, opt, pairs, t = setup
    assert [gi for gi, _ in pairs] == [0, 0, 0, 1, 1]
    assert t.maxn == 210 and t.nseg == 5 and t.steps == (1,) * 5
    assert t.sig[3] == (flat.offsets[id(m.b.weight)], 210, 3e-4, 0.05, 0.9, 0.999, 1e-8)
    assert [opt.state[p]["step"] for _, p in pairs] == [1] * 5
    assert opt._scan(flat, pairs, bump=False) == (t.maxn, t.sig, t.steps)  # bump=False counts nothing


def test_every_step_plus_one_advances(setup):
    _, flat, opt, pairs, t = setup
    for _ in range(3):
        _, sig, steps = opt._scan(flat, pairs, bump=True)
        assert t.advances(sig, steps)
        t.steps = steps


@pytest.mark.parametrize("off", [-1, 1])
@pytest.mark.parametrize("which", [0, 4])
def test_one_step_off_by_zero_or_two_rebuilds(setup, which, off):
    """One parameter's host step did not move (off by 0) or moved twice (off by 2) since the table's last
    launch -- another update path touched it, or skipped it."""
    _, flat, opt, pairs, t = setup
    opt.state[pairs[which][1]]["step"] += off
    _, sig, steps = opt._scan(flat, pairs, bump=True)
    assert sig == t.sig and steps[which] == t.steps[which] + 1 + off
    assert not t.advances(sig, steps)


@pytest.mark.parametrize("group", [0, 1])
@pytest.mark.parametrize("key,value", [("lr", 5e-4), ("weight_decay", 0.0), ("betas", (0.8, 0.999)),
                                       ("betas", (0.9, 0.99)), ("eps", 1e-6)])
def test_any_hyper_parameter_differing_rebuilds(setup, group, key, value):
    _, flat, opt, pairs, t = setup
    opt.param_groups[group][key] = value
    _, sig, steps = opt._scan(flat, pairs, bump=True)
    assert all(s == u + 1 for s, u in zip(steps, t.steps))
    assert not t.advances(sig, steps)


def test_a_different_subset_rebuilds(setup):
    """The steps of the subset's parameters all moved by one: only the segments tell it from the table's."""
    _, flat, opt, pairs, t = setup
    for sub in (pairs[:-1], pairs[1:], pairs[:2] + pairs[3:]):
        _, sig, steps = opt._scan(flat, sub, bump=True)
        assert all(s == 2 for s in steps)
        assert not t.advances(sig, steps)
        for _, p in sub:
            opt.state[p]["step"] = 1
