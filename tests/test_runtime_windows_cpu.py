"""Host logic of the two per-backward windows' shared helper (runtime.OncePerBackward) and of the
weight-gradient stream's CU-masked stream cache, without a device: the helper runs inside CPU autograd
backward passes, the stream constructors are replaced by sentinels.
"""
import pytest
import torch

from fervit import runtime


class _Hooked(torch.autograd.Function):
    """Identity whose backward calls `ctx.fn()` (the place a layer backward arms its windows)."""

    @staticmethod
    def forward(ctx, x, fn):
        ctx.fn = fn
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        ctx.fn()
        return g, None


def _backward(*fns):
    x = torch.ones(2, requires_grad=True)
    y = x
    for fn in fns:
        y = _Hooked.apply(y, fn)
    y.sum().backward()


def test_once_per_backward_queues_one_callback_per_pass():
    ran, seen = [], []
    once = runtime.OncePerBackward(lambda: ran.append(1))
    assert once.arm() is False and not once.queued  # not inside a backward pass

    def use():
        assert once.arm() is True and once.queued
        seen.append(len(ran))  # (the callback runs when the backward ends, not here)

    _backward(use, use, use)
    assert seen == [0, 0, 0] and ran == [1] and not once.queued
    _backward(use)
    assert seen == [0, 0, 0, 1] and ran == [1, 1] and not once.queued


def test_once_per_backward_heals_after_a_backward_that_raised():
    """Torch drops the queued callback when the backward raises: the next use -- in another backward or
    outside one -- runs it first, and the new backward gets its own."""
    ran = []
    once = runtime.OncePerBackward(lambda: ran.append("end"))

    def boom():
        raise RuntimeError("injected backward failure")

    for heal in ("backward", "outside"):
        del ran[:]
        with pytest.raises(RuntimeError, match="injected"):
            _backward(boom, once.arm)  # (backward runs the last function first)
        assert once.queued and ran == []
        if heal == "outside":
            assert once.current() is False and ran == ["end"]
            assert once.arm() is False and ran == ["end"]
        else:
            _backward(lambda: (once.arm(), ran.append("armed")))
            assert ran == ["end", "armed", "end"]
        assert not once.queued


def test_masked_side_streams_are_cached_per_device_and_mask(monkeypatch):
    made, plain = [], []
    w = runtime._WgradStream()

    def create(dev, words):
        made.append((dev, words))
        return ("masked", len(made))

    monkeypatch.setattr(w, "_create_masked", create)
    monkeypatch.setattr(torch.cuda, "Stream", lambda device=None: plain.append(device) or ("plain", len(plain)))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda: None)
    d0, d1 = torch.device("cuda", 0), torch.device("cuda", 1)

    w.cu_mask = [0xFFFF, 0x1_0000_00FF]  # (words are taken modulo 2^32)
    s = w._side(d0)
    assert w._side(d0) is s and made == [(d0, (0xFFFF, 0xFF))]
    for _ in range(2):  # two reset()s with the same mask: one creation, the same stream back
        w.reset()
        assert w.stream(d0) is None
        assert w._side(d0) is s
    assert len(made) == 1
    w.reset()
    w.cu_mask = [0xFF]  # a second mask: a second creation
    s2 = w._side(d0)
    assert s2 is not s and made[1:] == [(d0, (0xFF,))]
    assert w._side(d1) is not s2 and made[2:] == [(d1, (0xFF,))]  # per device
    w.reset()
    w.cu_mask = None  # no mask: an ordinary stream, not cached
    assert w._side(d0) == ("plain", 1) and plain == [d0] and len(made) == 3
    w.reset()
    w.cu_mask = [0xFFFF, 0xFF]
    assert w._side(d0) is s and len(made) == 3
