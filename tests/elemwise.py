"""The per-element comparison the kernel tests share (tests/test_gpu_rowops.py,
tests/test_gpu_gemm_elementwise.py): |got - ref| <= out_round * |ref| + c * 2^-23 * scale_i, with c
measured from float32 torch on the CPU against the same float64 reference."""
import torch

U = 2.0 ** -23
BF_ROUND = 2.0 ** -8


def measure_c(op, dtype, pairs):
    """c for one op: pairs = [(fp32-torch result, float64 ref, scale)]; worst error of the fp32 torch
    computation in units of 2^-23 * scale, times 4, floor 16. A fourth element of a pair is the absolute
    term of the caller's error model (assert_close's `extra`), taken off the error first."""
    worst = 0.0
    for f32, ref, scale, *extra in pairs:
        f32, ref, scale = torch.as_tensor(f32).double(), torch.as_tensor(ref).double(), torch.as_tensor(scale).double()
        err = (f32 - ref).abs()
        if extra:
            err = (err - torch.as_tensor(extra[0]).double()).clamp_min(0)
        live = scale > 0
        if live.any():
            worst = max(worst, (err[live] / (U * scale[live])).max().item())
        assert (err[~live] == 0).all(), f"{op}: fp32 torch differs from the reference where the scale is 0"
    print(f"c-measure {op} {dtype} {worst:.3f}")
    return max(16.0, 4.0 * worst)


def assert_close(name, got, ref, scale, c, out_round, extra=None):
    """|got - ref| <= out_round * |ref| + c * 2^-23 * scale (+ extra, an absolute term of the caller's error
    model); computed where `ref` lives. Returns the worst err / bound (0 / 0 counts as 0)."""
    ref = torch.as_tensor(ref).double()
    got = torch.as_tensor(got).detach().to(ref.device).double().reshape(-1)
    scale = torch.as_tensor(scale).to(ref.device).double().broadcast_to(ref.shape).reshape(-1)
    if extra is not None:
        extra = torch.as_tensor(extra).to(ref.device).double().broadcast_to(ref.shape).reshape(-1)
    ref = ref.reshape(-1)
    assert got.shape == ref.shape == scale.shape, (name, got.shape, ref.shape, scale.shape)
    bound = out_round * ref.abs() + c * U * scale
    if extra is not None:
        bound = bound + extra
    err = (got - ref).abs()
    bad = ~(err <= bound)  # also true for NaN
    if bad.any():
        ratio = torch.where(bad, err / bound.clamp_min(1e-300), torch.zeros_like(err))
        ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
        i = int(ratio.argmax())
        raise AssertionError(
            f"{name}: {int(bad.sum())} of {bad.numel()} elements out of bound; worst at flat index {i}: "
            f"got {got[i].item():.9g} ref {ref[i].item():.9g} |err| {err[i].item():.3g} bound {bound[i].item():.3g} "
            f"(c = {c:.1f}, out_round = {out_round:g})")
    return (err / bound.clamp_min(1e-300)).max().item() if err.numel() else 0.0


def assert_bits_equal(name, a, b):
    ia = a.contiguous().view(torch.int16 if a.element_size() == 2 else torch.int32)
    ib = b.contiguous().view(torch.int16 if b.element_size() == 2 else torch.int32)
    ne = (ia != ib).reshape(-1)
    if ne.any():
        i = int(ne.nonzero()[0])
        raise AssertionError(f"{name}: {int(ne.sum())} elements differ bit-wise, first at flat index {i}: "
                             f"{a.reshape(-1)[i].item()!r} vs {b.reshape(-1)[i].item()!r}")
