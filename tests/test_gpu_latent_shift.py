"""fer_latent_shift (csrc/latent_dirs.hip) bit for bit against torch on the CPU: out = x + step * direction with
the product and the sum rounded separately (`data/augment_latents.py:56`, `sefa/verify_directions.py:58`).

Shapes: (1, 1, 1); (3, 2, 5) D % 4 != 0, the element path; (2, 3, 4) and (5, 18, 512) the 16-byte path;
(228, 18, 512): 525,312 pieces of 16 bytes, more than the 2048 x 256 threads of the largest grid, so the
grid-stride loop runs a second round. Each with a [K, D] and a [K, L, D] direction set and K x S in
{1 x 1, 3 x 4}. The raw C ABI is called where strides and pointers matter."""
import numpy as np
import pytest
import torch

import latent_dirs_ref as R
from abi_harness import DEV, NAN, last_error, lib
from elemwise import assert_bits_equal
from fervit import ops

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (3, 2, 5), (2, 3, 4), (5, 18, 512), (228, 18, 512)]
KS = [(1, 1), (3, 4)]
INT32_MIN = -2 ** 31


def operands(n, L, D, K, S, per_layer, salt=0):
    g = torch.Generator().manual_seed(1000 * n + 10 * L + D + salt)
    x = torch.randn(n, L, D, generator=g)
    dirs = torch.randn(*((K, L, D) if per_layer else (K, D)), generator=g)
    steps = torch.tensor([-2.0, 0.3, 1.0, -0.7][:S]) if S <= 4 else torch.randn(S, generator=g)
    return x, dirs, steps


@pytest.mark.parametrize("K,S", KS)
@pytest.mark.parametrize("per_layer", [False, True])
@pytest.mark.parametrize("n,L,D", SHAPES)
def test_grid_mode_and_choice_mode(n, L, D, per_layer, K, S):
    """Grid mode equals the CPU, and choice mode fed the same (src, c) pairs equals grid mode."""
    if (n, L, D) == (228, 18, 512):
        assert n * L * D // 4 > 2048 * 256
    x, dirs, steps = operands(n, L, D, K, S, per_layer)
    ref = R.shift_grid(x, dirs, steps)
    xd, dd, sd = x.to(DEV), dirs.to(DEV), steps.to(DEV)
    got = ops.latent_shift(xd, dd, sd)
    assert got.shape == (K * S * n, L, D)
    assert_bits_equal("grid mode", got.cpu(), ref)
    c = torch.arange(K * S, dtype=torch.int32).repeat_interleave(n)
    by_choice = ops.latent_shift(xd.repeat(K * S, 1, 1), dd, sd, choice=c.to(DEV))
    assert_bits_equal("choice mode against grid mode", by_choice, got)


@pytest.mark.parametrize("per_layer", [False, True])
@pytest.mark.parametrize("n,L,D", [(7, 2, 5), (9, 18, 512)])
def test_choice_outside_the_range_copies_the_row(n, L, D, per_layer):
    """-1, K*S and INT32_MIN leave a row's bits alone (NaN payloads, -0.0 and denormals included: x + 0 * d
    would not); the other rows are shifted."""
    K, S = 3, 4
    x, dirs, steps = operands(n, L, D, K, S, per_layer)
    odd = torch.tensor([NAN, -0.0, 1e-40, float("inf")])
    x.view(-1)[:4] = odd[: min(4, x.numel())]
    x.view(torch.int32).view(-1)[4] = 0x7FC12345  # a NaN with a payload
    c = [-1, 0, K * S, 5, INT32_MIN, K * S - 1, 2 ** 31 - 1, 7, 3][:n]
    ref = R.shift_rows(x, dirs, steps, range(n), c)
    got = ops.latent_shift(x.to(DEV), dirs.to(DEV), steps.to(DEV), choice=torch.tensor(c, dtype=torch.int32, device=DEV))
    for r, cc in enumerate(c):
        assert_bits_equal(f"row {r} (choice {cc})", got[r].cpu(), x[r] if not 0 <= cc < K * S else ref[r])


@pytest.mark.parametrize("n,L,D", [(6, 2, 5), (6, 18, 512)])
def test_in_place(n, L, D):
    """out == x in choice mode. The choices differ from row to row and a copied row sits between shifted ones:
    a kernel that read row r after another row's write had landed on it, or that took its source from a row
    other than r, would show."""
    K, S = 2, 3
    x, dirs, steps = operands(n, L, D, K, S, False)
    c = [5, -1, 0, 3, 3, 1]
    ref = R.shift_rows(x, dirs, steps, range(n), c)
    xd = x.to(DEV)
    out = ops.latent_shift(xd, dirs.to(DEV), steps.to(DEV), choice=torch.tensor(c, dtype=torch.int32, device=DEV), out=xd)
    assert out.data_ptr() == xd.data_ptr()
    assert_bits_equal("in place", xd.cpu(), ref)


def raw_shift(x, ldx, dirs, dir_layers, steps, choice, out, ldo, n, K, S, L, D):
    return lib().fer_latent_shift(x.data_ptr(), ldx, dirs.data_ptr(), dir_layers, steps.data_ptr(),
                                  None if choice is None else choice.data_ptr(), out.data_ptr(), ldo, n, K, S, L, D,
                                  ops.stream())


@pytest.mark.parametrize("grid", [True, False])
@pytest.mark.parametrize("n,L,D,pad_x,pad_o", [(3, 2, 5, 3, 1), (5, 18, 512, 8, 4), (4, 3, 4, 4, 6)])
def test_padded_sample_strides(n, L, D, pad_x, pad_o, grid):
    """Sample strides above L * D on both sides; the NaN sentinels in out's padding and in its guard rows keep
    their bits. (4, 3, 4) with pad_o = 6: an output stride that is no multiple of 4 takes the element path."""
    K, S = 2, 2
    x, dirs, steps = operands(n, L, D, K, S, True)
    rows = K * S * n if grid else n
    xp = torch.full((n, L * D + pad_x), NAN, device=DEV)
    xp[:, :L * D] = x.reshape(n, -1).to(DEV)
    op = torch.full((rows + 2, L * D + pad_o), NAN, device=DEV)
    c = None if grid else torch.tensor([1, -1, 3, 0, 2][:n], dtype=torch.int32, device=DEV)
    rc = raw_shift(xp, L * D + pad_x, dirs.to(DEV), L, steps.to(DEV), c, op[1], L * D + pad_o, n, K, S, L, D)
    assert rc == 0, last_error()
    ref = R.shift_grid(x, dirs, steps) if grid else R.shift_rows(x, dirs, steps, range(n), c.tolist())
    got = op.cpu()
    assert_bits_equal("values", got[1:-1, :L * D], ref.reshape(rows, -1))
    sentinel = torch.full_like(got, NAN)
    got[1:-1, :L * D] = 0
    sentinel[1:-1, :L * D] = 0
    assert_bits_equal("padding and guard rows", got, sentinel)
    assert_bits_equal("x untouched", xp[:, :L * D].cpu(), x.reshape(n, -1))


@pytest.mark.parametrize("which", ["x", "out", "dirs"])
def test_unaligned_base_pointer_gives_the_same_bits(which):
    """One operand 4 bytes off a 16-byte boundary: the element path, the same bits as the aligned call."""
    n, L, D, K, S = 5, 18, 512, 3, 4
    x, dirs, steps = operands(n, L, D, K, S, False)
    ref = R.shift_grid(x, dirs, steps)

    def place(t, off):
        buf = torch.full((t.numel() + 8,), NAN, device=DEV)
        v = buf[4 + off:4 + off + t.numel()]
        v.copy_(t.reshape(-1))
        assert v.data_ptr() % 16 == (4 * off) % 16
        return buf, v

    _, xv = place(x, 1 if which == "x" else 0)
    _, dv = place(dirs, 1 if which == "dirs" else 0)
    off = 1 if which == "out" else 0
    obuf = torch.full((ref.numel() + 8,), NAN, device=DEV)
    ov = obuf[4 + off:4 + off + ref.numel()]
    rc = raw_shift(xv, L * D, dv, 1, steps.to(DEV), None, ov, L * D, n, K, S, L, D)
    assert rc == 0, last_error()
    assert_bits_equal("unaligned " + which, ov.cpu(), ref.reshape(-1))
    assert torch.isnan(obuf[:4 + off]).all() and torch.isnan(obuf[4 + off + ref.numel():]).all()


def test_argument_errors():
    """Each bad argument: a non-zero code and a message that names the entry; nothing is launched."""
    n, L, D, K, S = 2, 3, 4, 2, 2
    x, dirs, steps = (t.to(DEV) for t in operands(n, L, D, K, S, True))
    out = torch.full((K * S * n, L, D), NAN, device=DEV)
    good = dict(x=x, ldx=L * D, dirs=dirs, dir_layers=L, steps=steps, choice=None, out=out, ldo=L * D, n=n, K=K, S=S,
                L=L, D=D)
    bad = [dict(K=0), dict(K=-1), dict(S=0), dict(dir_layers=2), dict(dir_layers=0), dict(ldx=L * D - 1),
           dict(ldo=L * D - 1), dict(L=0), dict(D=0, dir_layers=L),
           dict(n=(2 ** 31 - 1) // (L * D) + 1, choice=torch.zeros(1, dtype=torch.int32, device=DEV)),  # too many elements
           dict(n=(2 ** 31 - 1) // (L * D * K * S) + 1)]
    for over in bad:
        rc = raw_shift(**{**good, **over})
        assert rc != 0 and last_error().startswith("latent_shift:"), (over, rc, last_error())
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    for empty in (0, -3):
        assert raw_shift(**{**good, "n": empty}) == 0
    assert torch.isnan(out).all()
    assert raw_shift(**good) == 0, last_error()
    assert_bits_equal("after the errors", out.cpu(), R.shift_grid(x.cpu(), dirs.cpu(), steps.cpu()))


def test_wrapper_rejects_what_the_kernel_cannot_take():
    x, dirs, steps = (t.to(DEV) for t in operands(2, 3, 4, 2, 2, False))
    with pytest.raises(ValueError):
        ops.latent_shift(x, dirs[:, :3], steps)
    with pytest.raises(ValueError):
        ops.latent_shift(x, dirs, steps, out=torch.empty(3, 3, 4, device=DEV))
    with pytest.raises(ValueError):
        ops.latent_shift(x, dirs, steps, out=torch.empty(8, 4, 3, device=DEV).transpose(1, 2))
    with pytest.raises(ValueError):  # grid mode in place
        ops.latent_shift(x, dirs[:1], steps[:1], out=x)
    with pytest.raises(ValueError):
        ops.latent_shift(x, dirs, steps, choice=torch.zeros(3, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        ops.latent_shift(x, dirs, steps.double())
