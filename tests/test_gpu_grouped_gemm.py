"""Grouped linear kernels (csrc/grouped.hip) element-wise against float64 on the CPU, with the bound of
DESIGN.md section 2.1 (tests/elemwise.py): |got - ref| <= out_round |ref| + c 2^-23 scale_i, scale_i the sum of
the absolute products behind element i, c measured per case from float32 torch on the CPU.

Every operand is a view into a NaN-filled parent with a guard row on each side and 8 padding columns: a
read outside the operand poisons the result, a write outside it is found afterwards. Each launch is
repeated into a fresh parent and must give the same bits."""
import functools

import numpy as np
import pytest
import torch

from abi_harness import NAN, all_nan, out_round, parent, untouched_parent, untouched_vec_parent, vec_parent
from elemwise import assert_bits_equal, assert_close, measure_c

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = {"bf16": torch.bfloat16, "fp32": torch.float32}
NK = [(256, 512), (512, 256), (256, 256), (16, 32)]  # (16, 32): the smallest shape the kernels accept
GS = [1, 3, 18]
MS = [1, 2, 8, 16, 17, 40]  # below one MFMA tile, exactly one, one row over, several
MMAX = max(MS)


@functools.lru_cache(maxsize=4)
def data(dtype, G, N, K):
    """Inputs rounded to `dtype` (as float64), shared by the tests of one shape, never modified."""
    g = np.random.default_rng(1000 * G + N + K)
    dt = DT[dtype]

    def r(*shape):
        return torch.from_numpy(g.standard_normal(shape)).to(dt).double()

    def rw():
        return (torch.from_numpy(g.standard_normal((G, N, K))) / K ** 0.5).to(dt).double()

    return dict(x=r(G, MMAX, K), w=[rw() for _ in range(3)],
                b=[torch.from_numpy(g.standard_normal((G, N))).float().double() for _ in range(3)],
                dy=[r(G, MMAX, N) for _ in range(3)])


def fwd_ref(d, s, bias):
    y = torch.einsum("gmk,gnk->gmn", d["x"], d["w"][s])
    sc = torch.einsum("gmk,gnk->gmn", d["x"].abs(), d["w"][s].abs())
    f32 = torch.einsum("gmk,gnk->gmn", d["x"].float(), d["w"][s].float())
    if bias:
        y, sc, f32 = y + d["b"][s][:, None], sc + d["b"][s].abs()[:, None], f32 + d["b"][s].float()[:, None]
    return y, sc, f32


@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("N,K", NK)
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_forward(dtype, N, K, G):
    from fervit import ops

    dt, d = DT[dtype], data(dtype, G, N, K)
    refs = {(s, bias): fwd_ref(d, s, bias) for s in range(3) for bias in (True, False)}
    c = measure_c(f"grouped fwd N{N} K{K} G{G}", dtype, [(f, y, sc) for y, sc, f in refs.values()])
    _, w = zip(*[parent(G, N, K, dt, d["w"][s]) for s in range(3)])
    _, b = zip(*[vec_parent(G, N, d["b"][s]) for s in range(3)])
    for M in MS:
        _, x = parent(G, M, K, dt, d["x"][:, :M])
        for ns in (1, 2, 3):
            for bias in (True, False):
                runs = []
                for _ in range(2):
                    ps, ys = zip(*[parent(G, M, N, dt) for _ in range(ns)])
                    ops.grouped_linear_fwd(x, list(w[:ns]), list(b[:ns]) if bias else None, outs=list(ys))
                    runs.append((ps, ys))
                for s in range(ns):
                    name = f"fwd {dtype} G{G} M{M} N{N} K{K} sets{ns} bias{bias} set{s}"
                    y, sc, _ = refs[(s, bias)]
                    assert_close(name, runs[0][1][s], y[:, :M], sc[:, :M], c, out_round(dt))
                    untouched_parent(name, runs[0][0][s], N)
                    assert_bits_equal(name, runs[0][0][s].nan_to_num(), runs[1][0][s].nan_to_num())


@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("N,K", NK)
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_dgrad(dtype, N, K, G):
    from fervit import ops

    dt, d = DT[dtype], data(dtype, G, N, K)
    refs, pairs = {}, []
    for ns in (1, 2, 3):
        ref = sum(torch.einsum("gmn,gnk->gmk", d["dy"][s], d["w"][s]) for s in range(ns))
        sc = sum(torch.einsum("gmn,gnk->gmk", d["dy"][s].abs(), d["w"][s].abs()) for s in range(ns))
        f32 = sum(torch.einsum("gmn,gnk->gmk", d["dy"][s].float(), d["w"][s].float()) for s in range(ns))
        refs[ns] = (ref, sc)
        pairs.append((f32, ref, sc))
    c = measure_c(f"grouped dgrad N{N} K{K} G{G}", dtype, pairs)
    _, w = zip(*[parent(G, N, K, dt, d["w"][s]) for s in range(3)])
    for M in MS:
        _, dy = zip(*[parent(G, M, N, dt, d["dy"][s][:, :M]) for s in range(3)])
        for ns in (1, 2, 3):
            name = f"dgrad {dtype} G{G} M{M} N{N} K{K} sets{ns}"
            runs = []
            for _ in range(2):
                p, dx = parent(G, M, K, dt)
                ops.grouped_linear_dgrad(list(dy[:ns]), list(w[:ns]), out=dx)
                runs.append((p, dx))
            assert_close(name, runs[0][1], refs[ns][0][:, :M], refs[ns][1][:, :M], c, out_round(dt))
            untouched_parent(name, runs[0][0], K)
            assert_bits_equal(name, runs[0][0].nan_to_num(), runs[1][0].nan_to_num())


@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("N,K", NK)
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_wgrad(dtype, N, K, G):
    """dW and db from one launch, 1-3 sets, with and without db, overwrite and accumulate (onto a random
    previous value, which joins the reference and the scale)."""
    from fervit import ops

    dt, d = DT[dtype], data(dtype, G, N, K)
    g = np.random.default_rng(7)
    prev_w = torch.from_numpy(g.standard_normal((G, N, K))).float()
    prev_b = torch.from_numpy(g.standard_normal((G, N))).float()
    for M in MS:
        x64 = d["x"][:, :M]
        refs, pairs = [], []
        for s in range(3):
            dy64 = d["dy"][s][:, :M]
            rw, rb = torch.einsum("gmn,gmk->gnk", dy64, x64), dy64.sum(1)
            sw, sb = torch.einsum("gmn,gmk->gnk", dy64.abs(), x64.abs()), dy64.abs().sum(1)
            fw, fb = torch.einsum("gmn,gmk->gnk", dy64.float(), x64.float()), dy64.float().sum(1)
            refs.append((rw, rb, sw, sb))
            pairs += [(fw, rw, sw), (fb, rb, sb), (fw + prev_w, rw + prev_w.double(), sw + prev_w.abs().double())]
        c = measure_c(f"grouped wgrad N{N} K{K} G{G} M{M}", dtype, pairs)
        _, x = parent(G, M, K, dt, x64)
        _, dy = zip(*[parent(G, M, N, dt, d["dy"][s][:, :M]) for s in range(3)])
        # every set count, db on / off and accumulate on / off, without the full cross product
        for ns, with_db, acc in ((1, True, False), (2, False, True), (3, True, True), (3, False, False)):
            runs = []
            for _ in range(2):
                pw, dw = zip(*[parent(G, N, K, torch.float32, prev_w if acc else None) for _ in range(ns)])
                pb, db = zip(*[vec_parent(G, N, prev_b if acc else None) for _ in range(ns)])
                ops.grouped_linear_wgrad(list(dy[:ns]), x, list(dw), list(db) if with_db else None,
                                         accumulate=acc)
                runs.append((pw, dw, pb, db))
            for s in range(ns):
                name = f"wgrad {dtype} G{G} M{M} N{N} K{K} sets{ns} db{with_db} acc{acc} set{s}"
                rw, rb, sw, sb = refs[s]
                if acc:
                    rw, sw = rw + prev_w.double(), sw + prev_w.abs().double()
                    rb, sb = rb + prev_b.double(), sb + prev_b.abs().double()
                assert_close(name + " dw", runs[0][1][s], rw, sw, c, 0.0)
                untouched_parent(name, runs[0][0][s], K)
                assert_bits_equal(name, runs[0][0][s].nan_to_num(), runs[1][0][s].nan_to_num())
                if with_db:
                    assert_close(name + " db", runs[0][3][s], rb, sb, c, 0.0)
                    untouched_vec_parent(name + " db", runs[0][2][s], N)
                elif not acc:
                    all_nan(name + " db (not asked for)", runs[0][2][s])


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_in_place_bgk_addressing_and_skip_mask(dtype):
    """x read as the [B, G, K] tensor it is (row stride G*K, group stride K), y and dx written into
    [B, G, N] / [B, G, K] tensors in place; a skipped group's gradients stay untouched."""
    from fervit import ops

    dt = DT[dtype]
    G, M, N, K = 3, 8, 32, 64
    d = data(dtype, G, N, K)
    x64, w64, dy64 = d["x"][:, :M], d["w"][0], d["dy"][0][:, :M]
    xb = x64.transpose(0, 1).contiguous().to(dt).to(DEV)  # [M, G, K]
    _, w = parent(G, N, K, dt, w64)
    _, b = vec_parent(G, N, d["b"][0])
    y, sc, f32 = fwd_ref(d, 0, True)
    c = measure_c("grouped in-place fwd", dtype, [(f32, y, sc)])
    yb = torch.full((M, G, N), NAN, dtype=dt, device=DEV)
    ops.grouped_linear_fwd(xb.transpose(0, 1), [w], [b], outs=[yb.transpose(0, 1)])
    assert_close("in-place fwd", yb.transpose(0, 1), y[:, :M], sc[:, :M], c, out_round(dt))
    dyb = dy64.transpose(0, 1).contiguous().to(dt).to(DEV)
    ref = torch.einsum("gmn,gnk->gmk", dy64, w64)
    scd = torch.einsum("gmn,gnk->gmk", dy64.abs(), w64.abs())
    cd = measure_c("grouped in-place dgrad", dtype,
                   [(torch.einsum("gmn,gnk->gmk", dy64.float(), w64.float()), ref, scd)])
    dxb = torch.full((M, G, K), NAN, dtype=dt, device=DEV)
    ops.grouped_linear_dgrad([dyb.transpose(0, 1)], [w], out=dxb.transpose(0, 1))
    assert_close("in-place dgrad", dxb.transpose(0, 1), ref, scd, cd, out_round(dt))
    rw, sw = torch.einsum("gmn,gmk->gnk", dy64, x64), torch.einsum("gmn,gmk->gnk", dy64.abs(), x64.abs())
    cw = measure_c("grouped in-place wgrad", dtype,
                   [(torch.einsum("gmn,gmk->gnk", dy64.float(), x64.float()), rw, sw)])
    pw, dw = parent(G, N, K, torch.float32)
    pb, db = vec_parent(G, N)
    ops.grouped_linear_wgrad([dyb.transpose(0, 1)], xb.transpose(0, 1), [dw], [db], skip_mask=0b010)
    assert bool(dw[1].isnan().all()) and bool(db[1].isnan().all())
    for g in (0, 2):
        assert_close(f"in-place wgrad group {g}", dw[g], rw[g], sw[g], cw, 0.0)
    untouched_parent("in-place wgrad", pw, K)


def test_rejected_shapes_return_an_error_with_a_message():
    """One case per rejection rule; nothing is launched."""
    from fervit import ops
    from fervit._lib import FerError, lib

    bf = torch.bfloat16

    def t(*shape, dtype=bf):
        return torch.zeros(*shape, dtype=dtype, device=DEV)

    with pytest.raises(FerError, match="K must be a multiple of 32"):
        ops.grouped_linear_fwd(t(1, 2, 48), [t(1, 16, 48)])
    with pytest.raises(FerError, match="N must be a multiple of 16"):
        ops.grouped_linear_fwd(t(1, 2, 32), [t(1, 24, 32)])
    with pytest.raises(FerError, match="N must be a multiple of 16"):
        ops.grouped_linear_dgrad([t(1, 2, 24)], [t(1, 24, 32)])
    with pytest.raises(FerError, match="K must be a multiple of 32"):
        ops.grouped_linear_wgrad([t(1, 2, 16)], t(1, 2, 48), [t(1, 16, 48, dtype=torch.float32)])
    with pytest.raises(FerError, match="16-byte aligned rows"):  # a row stride that is no multiple of 8
        ops.grouped_linear_fwd(t(1, 2, 36)[:, :, :32], [t(1, 16, 32)])
    with pytest.raises(FerError, match="16-byte aligned rows"):  # a base 8 bytes off
        ops.grouped_linear_fwd(t(1, 2, 40)[:, :, 4:36], [t(1, 16, 32)])
    with pytest.raises(FerError, match="16-byte aligned rows"):  # a group stride that is no multiple of 8
        ops.grouped_linear_fwd(torch.as_strided(t(400), (2, 2, 32), (68, 32, 1)), [t(2, 16, 32)])
    with pytest.raises(FerError, match="no output requested"):
        ops.grouped_linear_wgrad([t(1, 2, 16)], t(1, 2, 32))
    x, w, y = t(1, 2, 32), t(1, 16, 32), t(1, 2, 16)
    L = lib()
    # a gap in the weight sets (set 2 without set 1), and more groups than the launch grid takes
    assert L.fer_grouped_linear_fwd(0, x.data_ptr(), 32, 0, w.data_ptr(), None, w.data_ptr(), 32, 0, None, None, None,
                                    0, y.data_ptr(), None, y.data_ptr(), 16, 0, 1, 2, 16, 32, None) != 0
    assert b"from set 0 upwards" in L.fer_last_error()
    assert L.fer_grouped_linear_fwd(0, x.data_ptr(), 32, 0, w.data_ptr(), None, None, 32, 0, None, None, None, 0,
                                    y.data_ptr(), None, None, 16, 0, 65536, 2, 16, 32, None) != 0
    assert b"launch grid" in L.fer_last_error()


def test_rejections_of_the_gradient_entry_points():
    """The remaining rules, through the C ABI with everything else valid; nothing is launched."""
    import ctypes

    from fervit._lib import SIGNATURES, lib

    L = lib()
    t = torch.zeros(4096, dtype=torch.float32, device=DEV)
    p = t.data_ptr()

    def raw(name, **over):
        args = [None if a is ctypes.c_void_p else (0.0 if a is ctypes.c_float else 0) for a in SIGNATURES[name][1]]
        for pos, val in over.items():
            args[int(pos[1:])] = val
        rc = getattr(L, name)(*args)
        return rc, L.fer_last_error().decode()

    # fer_grouped_linear_wgrad: dy 1-3, lddy 4, x 6, ldx 7, dw 9-11, lddw 12, db 14-16, skip 19, G M N K 20-23
    ok = dict(a1=p, a4=16, a6=p, a7=32, a9=p, a12=32, a20=1, a21=2, a22=16, a23=32)
    for over, text in ((dict(a10=p), "an output without its gradient set"),
                       (dict(a12=34), "dw needs 16-byte aligned fp32 rows"),
                       (dict(a9=p + 4), "dw needs 16-byte aligned fp32 rows"),
                       (dict(a19=1, a20=65), "skip_mask covers at most 64 groups"),
                       (dict(a21=65535 * 4 + 1), "launch grid"),
                       (dict(a22=1 << 30, a23=1 << 20, a4=1 << 30, a7=1 << 20, a12=1 << 20), "too large for one launch")):
        rc, msg = raw("fer_grouped_linear_wgrad", **dict(ok, **over))
        assert rc != 0 and text in msg, (over, rc, msg)
    # fer_grouped_linear_dgrad: dy 1-3, lddy 4, w 6-8, ldw 9, dx 11, lddx 12, G M N K 14-17
    okd = dict(a1=p, a4=16, a6=p, a9=32, a11=p, a12=32, a14=1, a15=2, a16=16, a17=32)
    for over, text in ((dict(a7=p), "from set 0 upwards"), (dict(a12=36), "dx needs 16-byte aligned rows"),
                       (dict(a14=65536), "launch grid")):
        rc, msg = raw("fer_grouped_linear_dgrad", **dict(okd, **over))
        assert rc != 0 and text in msg, (over, rc, msg)
