"""The harness the element-wise kernel tests share (tests/test_gpu_convbn.py, test_gpu_attnpool.py,
test_gpu_rowops.py, test_gpu_gemm_elementwise.py, test_gpu_grouped_gemm.py, test_gpu_highway.py,
test_gpu_attention_elementwise.py, test_gpu_edge_kernels.py, test_gpu_optim_kernels.py,
test_gpu_reduce_window.py): access to the C ABI, and operands as views into NaN-filled parents whose guard
rows and padding columns must keep their bits. The bound arithmetic is tests/elemwise.py.

The tests call the raw library (`lib()`) with the strides of these views, not the fervit.ops wrappers, so
that padded strides reach the kernel and a slip in a wrapper cannot hide one in the ABI."""
import numpy as np
import torch

from elemwise import BF_ROUND, assert_bits_equal

DEV = "cuda"
NAN = float("nan")


def ops():
    from fervit import ops as o

    return o


def lib():
    from fervit._lib import lib as l_

    return l_()


def last_error():
    return lib().fer_last_error().decode()


def tdt(dtype):
    return torch.bfloat16 if dtype == "bf16" else torch.float32


def f32v(v):
    """The fp32 value a `float` argument of the C ABI carries."""
    return float(np.float32(v))


def ptr(t):
    return None if t is None else t.data_ptr()


def exact(v):
    """The float64 values a device tensor holds."""
    return v.float().cpu().double()


def out_round(dt):
    """2^-8 for a bf16 output, 0 for an fp32 one; dt: torch dtype or "bf16" / "fp32"."""
    return BF_ROUND if dt in (torch.bfloat16, "bf16") else 0.0


def _same_but(name, parent, inside):
    """Everything of `parent` outside the index `inside` still holds the NaN bits it was filled with."""
    a = parent.clone()
    a[inside] = 0
    b = torch.full_like(parent, NAN)
    b[inside] = 0
    assert_bits_equal(name, a, b)


# ---------------------------------------------------------------------- [rows][cols] operands
def nanview(rows, cols, pad, dt, src=None, guard=2, align=16):
    """[rows][cols] view inside a NaN-filled parent with `guard` rows above and below and `pad` extra
    columns; returns (view, parent). `align`: the byte alignment the view's first element must have (a row
    stride that is no multiple of 4 elements is only for kernels that move single elements)."""
    parent = torch.full((rows + 2 * guard, cols + pad), NAN, dtype=dt, device=DEV)
    v = parent[guard:guard + rows, :cols]
    if src is not None:
        v.copy_(src.to(dt))
    assert v.data_ptr() % align == 0
    return v, parent


def untouched(name, parent, rows, cols, guard=2):
    """Everything outside the view still holds the parent's NaN bits."""
    _same_but(name + " padding", parent, (slice(guard, guard + rows), slice(0, cols)))


def all_nan(name, parent):
    assert_bits_equal(name + " untouched", parent, torch.full_like(parent, NAN))


def nanvec(n):
    """[n] fp32 view inside a NaN-filled parent with 4 guard elements on each side (16-byte aligned);
    returns (view, parent)."""
    parent = torch.full((n + 8,), NAN, dtype=torch.float32, device=DEV)
    return parent[4:4 + n], parent


def untouched_vec(name, parent, n):
    _same_but(name + " guards", parent, slice(4, 4 + n))


def nanflat(n, dt, src=None, guard=8, shift=0):
    """[n] contiguous view of either dtype inside a NaN-filled parent, `guard` elements in front (16-byte
    aligned for guard = 8; `shift` more elements move it off that alignment) and at least as many behind;
    returns (view, parent)."""
    parent = torch.full((n + 2 * guard + shift,), NAN, dtype=dt, device=DEV)
    v = parent[guard + shift:guard + shift + n]
    if src is not None:
        v.copy_(src.reshape(-1).to(dt))
    return v, parent


def untouched_flat(name, parent, n, guard=8, shift=0):
    _same_but(name + " guards", parent, slice(guard + shift, guard + shift + n))


# ---------------------------------------------------------------------- grouped [G][rows][cols] operands
def parent(G, rows, cols, dtype, data=None):
    """[G][rows][cols] view inside a NaN-filled parent with a guard row on each side of every group and 8
    padding columns; returns (parent, view)."""
    p = torch.full((G, rows + 2, cols + 8), NAN, dtype=dtype, device=DEV)
    v = p[:, 1:-1, :cols]
    if data is not None:
        v.copy_(data)
    return p, v


def untouched_parent(name, p, cols):
    _same_but(name + ": wrote outside its operand", p, (slice(None), slice(1, -1), slice(0, cols)))


def vec_parent(G, n, data=None):
    """[G, n] fp32 vectors at a padded group stride inside a NaN parent; returns (parent, view)."""
    p = torch.full((G, n + 8), NAN, dtype=torch.float32, device=DEV)
    v = p[:, :n]
    if data is not None:
        v.copy_(data)
    return p, v


def untouched_vec_parent(name, p, n):
    _same_but(name + ": wrote outside its vectors", p, (slice(None), slice(0, n)))
