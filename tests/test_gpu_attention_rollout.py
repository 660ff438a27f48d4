"""fer_attention_rollout_cls (csrc/attn_probs.hip) on the GPU against fervit.explain.rollout_reference
(fp64, full matrix product, row 0) on the same random row-stochastic maps.

Element gate = 4x the maximum measured on an MI355X over the shapes and residuals below (each run
prints `rollout-measure L B N residual <max|d|> <max|sum - 1|>`), never looser than 1e-5.
  measured: max |d| 2.5e-8
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = [(1, 2, 19), (4, 3, 37), (12, 2, 197), (3, 2, 1)]
GATE = 4 * 2.5e-8
CAP = 1e-5


def make_maps(L, B, N):
    g = torch.Generator().manual_seed(L * 1000 + N)
    return torch.softmax(3 * torch.randn(L, B, N, N, generator=g), dim=-1)


@pytest.mark.parametrize("L,B,N", SHAPES)
@pytest.mark.parametrize("residual", [0.0, 0.5])
def test_rollout_matches_reference(L, B, N, residual):
    from fervit import ops
    from fervit.explain import rollout_reference

    maps = make_maps(L, B, N)
    ref = rollout_reference(maps, residual)
    md = maps.to(DEV)
    r = ops.attention_rollout_cls(md, residual)
    again = ops.attention_rollout_cls(md, residual, out=torch.full((B, N), float("nan"), device=DEV))
    assert r.shape == (B, N) and r.dtype == torch.float32
    assert torch.equal(r, again)
    r = r.cpu()
    err = (r.double() - ref).abs().max().item()
    serr = (r.double().sum(-1) - 1.0).abs().max().item()
    print(f"rollout-measure {L} {B} {N} {residual} {err:.3e} {serr:.3e}")
    assert GATE <= CAP
    # a convex combination of probability rows
    assert not torch.isnan(r).any() and r.min().item() >= 0.0 and r.max().item() <= 1.0
    assert serr <= 4 * L * N * 2.0 ** -23
    assert err <= GATE, err


def test_rollout_refuses_bad_arguments():
    from fervit import ops
    from fervit._lib import lib

    maps = make_maps(2, 2, 19).to(DEV)
    out = torch.full((2, 19), -7.5, device=DEV)
    L = lib()
    for res in (1.0, -0.1, float("nan")):
        rc = L.fer_attention_rollout_cls(maps.data_ptr(), 2, 2, 19, res, out.data_ptr(), ops.stream())
        assert rc < 0 and "residual" in L.fer_last_error().decode(), res
    assert L.fer_attention_rollout_cls(maps.data_ptr(), 0, 2, 19, 0.5, out.data_ptr(), ops.stream()) < 0
    torch.cuda.synchronize()
    assert (out == -7.5).all()
    with pytest.raises(ValueError):
        ops.attention_rollout_cls(maps, 1.0)
    with pytest.raises(ValueError):
        ops.attention_rollout_cls(maps[:, :, :, :18])
