"""CPU checks of the attention-map feature: the two C entry points are declared, exported and
bound; the host wrapper refuses CPU tensors; rollout_reference (the definition the device
rollout is tested against) on hand-computable cases; capture_attention's tap bookkeeping."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "fervit.h")
LIB = os.path.join(ROOT, "fer-vit_amd", "fervit", "libfervit.so")
NEW = ("fer_attention_probs", "fer_attention_rollout_cls")


def test_header_declares_the_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    names = set(re.findall(r"\b(fer_[a-z0-9_]+)\s*\(", src))
    for n in NEW:
        assert n in names, n


@pytest.mark.skipif(not os.path.exists(LIB), reason="libfervit.so not built (run __graft_entry__.build())")
def test_library_exports_and_binds_the_entry_points():
    from fervit._lib import SIGNATURES

    lib = ctypes.CDLL(LIB)
    for n in NEW:
        assert hasattr(lib, n), n
        assert n in SIGNATURES, n
    assert len(SIGNATURES["fer_attention_probs"][1]) == 14
    assert len(SIGNATURES["fer_attention_rollout_cls"][1]) == 7


def test_attention_probs_refuses_cpu_tensors():
    from fervit import ops

    qkv = torch.zeros(2 * 5, 3 * 2 * 8)
    with pytest.raises(RuntimeError, match="needs tensors on a ROCm device"):
        ops.attention_probs(qkv, 2, 5, 2, 8)
    with pytest.raises(RuntimeError, match="needs tensors on a ROCm device"):
        ops.attention_rollout_cls(torch.zeros(1, 2, 5, 5))


def _stochastic(L, B, N, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.softmax(3 * torch.randn(L, B, N, N, generator=g), dim=-1)


def test_rollout_reference_single_layer():
    from fervit.explain import rollout_reference

    A = _stochastic(1, 3, 7, 0)
    for res in (0.0, 0.5, 0.25):
        want = (1 - res) * A[0, :, 0, :].double()
        want[:, 0] += res
        assert torch.allclose(rollout_reference(A, res), want, atol=1e-15, rtol=0)


def test_rollout_reference_identity_maps_give_e0():
    from fervit.explain import rollout_reference

    A = torch.eye(6).expand(4, 2, 6, 6)
    r = rollout_reference(A, 0.5)
    e0 = torch.zeros(2, 6, dtype=torch.float64)
    e0[:, 0] = 1
    assert r.dtype == torch.float64 and torch.equal(r, e0)


def test_rollout_reference_uniform_maps_closed_form():
    """A = J/N is idempotent, so (aI + (1-a)J/N)^L = a^L I + (1 - a^L) J/N."""
    from fervit.explain import rollout_reference

    L, B, N, a = 5, 2, 9, 0.5
    r = rollout_reference(torch.full((L, B, N, N), 1.0 / N, dtype=torch.float64), a)
    want = torch.full((B, N), (1 - a ** L) / N, dtype=torch.float64)
    want[:, 0] += a ** L
    assert torch.allclose(r, want, atol=1e-14, rtol=0)


def test_rollout_reference_is_the_cls_row_of_the_ordered_product():
    """Two layers by hand: row 0 of A'_2 A'_1 (the LAST layer is the leftmost factor)."""
    from fervit.explain import rollout_reference

    A = _stochastic(2, 1, 4, 1).double()
    eye = torch.eye(4, dtype=torch.float64)
    P = (0.5 * eye + 0.5 * A[1, 0]) @ (0.5 * eye + 0.5 * A[0, 0])
    assert torch.allclose(rollout_reference(A, 0.5)[0], P[0], atol=1e-15, rtol=0)
    with pytest.raises(ValueError):
        rollout_reference(A, 1.0)


def test_capture_attention_restores_the_previous_tap():
    from fervit import explain, layers

    assert layers.ATTN_TAP is None
    with pytest.raises(KeyError):
        with explain.capture_attention() as maps:
            assert callable(layers.ATTN_TAP) and maps == []
            raise KeyError("inside the block")
    assert layers.ATTN_TAP is None

    def outer(qkv, cfg):
        pass

    layers.ATTN_TAP = outer
    try:
        with explain.capture_attention(queries="cls"):
            assert layers.ATTN_TAP is not outer
        assert layers.ATTN_TAP is outer
    finally:
        layers.ATTN_TAP = None
    with pytest.raises(ValueError):
        with explain.capture_attention(queries="first"):
            pass
    assert layers.ATTN_TAP is None
