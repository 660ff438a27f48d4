"""Element-wise checks of the fused AdamW (fer_adamw, csrc/optim.hip adamw_kernel) and of the transposed bf16
weight shadow (fer_transpose_bf16_segments, transpose_segs_kernel) through the raw C ABI, with hand-built
segment tables over one flat buffer.

Conventions of tests/test_gpu_rowops.py (DESIGN.md sections 2.1 and 2.6): the flat buffers are NaN-filled
(sentinel-filled for the shadow) outside the segments and must keep those bits; AdamW is compared per element
with a float64 AdamW (decoupled decay, bias-corrected) evaluated with the fp32 hyper-parameter values the
segment struct holds, |got - ref| <= c * 2^-23 * scale_i, c measured by running the same formula function in
float32 torch on the CPU (times 4, floor 16, printed as `c-measure`); the shadow is compared as uint16
patterns."""
import ctypes
import math

import pytest
import torch

from abi_harness import f32v, last_error, ops
from abi_harness import lib as L
from elemwise import assert_bits_equal, assert_close, measure_c

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
F64, F32 = torch.float64, torch.float32
STEPS = [1, 2, 1000, 100000]


def stream():
    return ops().stream()


def to_device_bytes(arr):
    host = torch.frombuffer(bytearray(ctypes.string_at(ctypes.addressof(arr), ctypes.sizeof(arr))), dtype=torch.uint8)
    return host.to(DEV)


# ====================================================================== AdamW
def make_segments(layout, rot):
    """layout: [(offset, numel)]; per-segment hyper-parameters all different, step cycling through STEPS from
    `rot`. Returns the ctypes array (whose float fields hold the fp32 values the kernel reads)."""
    from fervit._lib import AdamWSegment

    segs = []
    for i, (off, numel) in enumerate(layout):
        segs.append(AdamWSegment(off, numel, 1e-3 * (1 + i), 0.05 * i, 0.9 - 0.01 * i, 0.999 - 0.002 * i,
                                 1e-8 * (1 + 10 * i), STEPS[(i + rot) % 4]))
    return (AdamWSegment * len(segs))(*segs)


def adamw_formula(p, g, m, v, s, gscale, clip, add, dt, hyper=None):
    """One AdamW step of a segment in dt arithmetic. s: the segment struct (fp32 values); hyper: (lr, wd, b1,
    b2, eps) to use instead (the double-precision values of torch.optim.AdamW).
    m' = b1 m + (1 - b1) g, v' = b2 v + (1 - b2) g^2, m^ = m' / (1 - b1^t), v^ = v' / (1 - b2^t),
    p' = p (1 - lr wd) - lr m^ / (sqrt(v^) + eps), g the gradient times grad_scale times the clip factor.
    Scales: m: b1 |m| + (1 - b1) |g|; v: v'; p: |p| + lr |m^| / (sqrt(v^) + eps)."""
    lr, wd, b1, b2, eps = hyper if hyper is not None else (s.lr, s.weight_decay, s.beta1, s.beta2, s.eps)
    T = lambda x: torch.tensor(x, dtype=dt)
    lr, wd, b1, b2, eps = T(lr), T(wd), T(b1), T(b2), T(eps)
    t = T(float(s.step + add))
    p, g, m, v = (x.to(dt) for x in (p, g, m, v))
    gr = g * (T(gscale) * T(clip))
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    m2 = b1 * m + (1 - b1) * gr
    v2 = b2 * v + (1 - b2) * gr * gr
    upd = lr * (m2 / bc1) / ((v2 / bc2).sqrt() + eps)
    return dict(p=p * (1 - lr * wd) - upd, m=m2, v=v2, upd=upd, s_p=p.abs() + upd.abs(),
                s_m=b1 * m.abs() + (1 - b1) * gr.abs(), s_v=v2)


def adamw_state(total, layout, seed):
    """NaN everywhere, the segments filled: p randn, m 0.1 randn, v >= 0 (some exact zeros), gradients randn
    with exact zeros and a few values of magnitude 1e-8 and 1e4."""
    gen = torch.Generator().manual_seed(seed)
    bufs = {k: torch.full((total,), NAN) for k in "pgmv"}
    inside = torch.zeros(total, dtype=torch.bool)
    for off, n in layout:
        inside[off:off + n] = True
        bufs["p"][off:off + n] = torch.randn(n, generator=gen)
        bufs["m"][off:off + n] = 0.1 * torch.randn(n, generator=gen)
        v = 0.01 * torch.rand(n, generator=gen)
        v[torch.rand(n, generator=gen) < 0.05] = 0.0
        bufs["v"][off:off + n] = v
        g = torch.randn(n, generator=gen)
        sel = torch.rand(n, generator=gen)
        g[sel < 0.10] = 0.0
        g[(sel >= 0.10) & (sel < 0.15)] *= 1e-8
        g[(sel >= 0.15) & (sel < 0.20)] *= 1e4
        bufs["g"][off:off + n] = g
    return bufs, inside


def run_adamw(layout, rot, add, clip, gscale, with_bf16, tag):
    segs = make_segments(layout, rot)
    total = max(off + n for off, n in layout) + 64
    host, inside = adamw_state(total, layout, 17 * len(layout) + rot)
    d = {k: t.to(DEV) for k, t in host.items()}
    pb = torch.full((total,), NAN, dtype=torch.bfloat16, device=DEV) if with_bf16 else None
    segs_dev = to_device_bytes(segs)
    add_dev = None if add is None else torch.tensor([add], dtype=torch.int64, device=DEV)
    clip_dev = None if clip is None else torch.tensor([clip], dtype=F32, device=DEV)
    gscale = f32v(gscale)
    rc = L().fer_adamw(d["p"].data_ptr(), d["g"].data_ptr(), d["m"].data_ptr(), d["v"].data_ptr(),
                       None if pb is None else pb.data_ptr(), segs_dev.data_ptr(), len(layout),
                       max(n for _, n in layout), gscale, None if clip_dev is None else clip_dev.data_ptr(),
                       None if add_dev is None else add_dev.data_ptr(), stream())
    assert rc == 0, last_error()
    got = {k: t.cpu() for k, t in d.items()}
    pairs = {k: [] for k in "pmv"}
    refs = []
    for s, (off, n) in zip(segs, layout):
        sl = slice(off, off + n)
        args = (host["p"][sl], host["g"][sl], host["m"][sl], host["v"][sl], s, gscale, 1.0 if clip is None else clip,
                0 if add is None else add)
        r64, r32 = adamw_formula(*args, F64), adamw_formula(*args, F32)
        refs.append(r64)
        for k in "pmv":
            pairs[k].append((r32[k], r64[k], r64["s_" + k]))
    c = {k: measure_c(f"adamw.{k}", "fp32", pairs[k]) for k in "pmv"}
    for i, (r64, (off, n)) in enumerate(zip(refs, layout)):
        for k in "pmv":
            assert_close(f"{tag} segment {i} (offset {off}, numel {n}, step {segs[i].step}) {k}", got[k][off:off + n],
                         r64[k], r64["s_" + k], c[k], 0.0)
    # everything outside the segments keeps its bits, in all five buffers (the gradient included)
    for k in "pgmv":
        assert_bits_equal(f"{tag} {k} outside the segments", got[k][~inside], host[k][~inside])
    assert_bits_equal(f"{tag} gradient unchanged", got["g"], host["g"])
    if pb is not None:
        pbh = pb.cpu()
        assert_bits_equal(f"{tag} param_bf16 is the RNE cast of the fp32 p written", pbh[inside],
                          got["p"][inside].to(torch.bfloat16))
        assert_bits_equal(f"{tag} param_bf16 outside the segments", pbh[~inside],
                          torch.full((int((~inside).sum()),), NAN, dtype=torch.bfloat16))
    return got, host, segs


LAYOUTS = {
    1: [(64, 1025)],
    2: [(66, 5), (128, 1023)],
    7: [(0, 1), (64, 3), (128, 4), (194, 5), (256, 1023), (1344, 1025), (2432, 700)],
}
ADAMW_OPTS = [dict(add=None, clip=None, gscale=1.0, with_bf16=True), dict(add=0, clip=0.25, gscale=0.125, with_bf16=False),
              dict(add=3, clip=None, gscale=0.125, with_bf16=True), dict(add=3, clip=0.25, gscale=1.0, with_bf16=False)]


@pytest.mark.parametrize("opt", range(len(ADAMW_OPTS)))
@pytest.mark.parametrize("nseg", sorted(LAYOUTS))
def test_adamw_segment_tables(nseg, opt):
    """fer_adamw over tables of 1, 2 and 7 segments of one flat buffer, per-segment lr / weight decay / betas /
    eps / step all different (steps 1, 2, 1000, 100000, rotated by the option index so every segment size
    meets every step). adamw_kernel's 4-wide path needs offset % 4 == 0: offsets are multiples of 64 but for
    the numel = 5 segment at offset 66 / 194 (offset % 4 == 2: the per-element loop over the whole segment).
    numel = 1, 3: no 4-wide head at all; 4: no tail; 5, 1023, 1025: a tail of 1 or 3 after the 4-wide head.
    Options: step_add null / -> 0 / -> 3, clip null / -> 0.25, grad_scale 1 / 1/8, param_bf16 null / not. m, v
    and p within the measured bound, param_bf16 the RNE cast of p bit for bit, the gaps between segments and
    the tail of all five buffers untouched."""
    run_adamw(LAYOUTS[nseg], opt, tag=f"adamw[{nseg} segments]", **ADAMW_OPTS[opt])


def test_adamw_grid_stride():
    """A segment of 8192 * 1024 + 5 elements: the launch has at most 256 blocks per segment, so the 4-wide loop
    strides (33 trips) and the 1-element tail follows; a 1000-element segment in the same launch leaves all
    but its first block with nothing to do."""
    run_adamw([(0, 1000), (1024, 8192 * 1024 + 5)], 2, add=3, clip=0.25, gscale=0.125, with_bf16=True,
              tag="adamw[grid stride]")


def test_adamw_against_double_precision_hyperparameters():
    """torch.optim.AdamW holds lr / betas / eps as doubles, the segment struct as floats: 1 - 0.999f differs from
    0.001 by 1.3e-5 relative. At step 1 (on a non-zero state, so that the betas do not cancel) the update of the
    kernel is compared with the float64 formula on the DOUBLE hyper-parameters; allowed is the usual bound
    plus 4 x the difference the float64 formula itself shows between fp32 and double hyper-parameters. The
    measured discrepancy is printed."""
    layout = [(64, 4096)]
    hyper = (1e-3, 0.05, 0.9, 0.999, 1e-8)
    from fervit._lib import AdamWSegment

    seg = AdamWSegment(64, 4096, *hyper, 1)
    segs = (AdamWSegment * 1)(seg)
    host, inside = adamw_state(64 + 4096 + 64, layout, 5)
    d = {k: t.to(DEV) for k, t in host.items()}
    segs_dev = to_device_bytes(segs)
    rc = L().fer_adamw(d["p"].data_ptr(), d["g"].data_ptr(), d["m"].data_ptr(), d["v"].data_ptr(), None,
                       segs_dev.data_ptr(), 1, 4096, 1.0, None, None, stream())
    assert rc == 0, last_error()
    sl = slice(64, 64 + 4096)
    args = (host["p"][sl], host["g"][sl], host["m"][sl], host["v"][sl], segs[0], 1.0, 1.0, 0)
    r_f, r_d, r32 = adamw_formula(*args, F64), adamw_formula(*args, F64, hyper=hyper), adamw_formula(*args, F32)
    c = measure_c("adamw.p", "fp32", [(r32["p"], r_f["p"], r_f["s_p"])])
    gap = (r_f["p"] - r_d["p"]).abs()
    live = r_d["upd"].abs() > 0
    print(f"adamw-hyper-discrepancy fp32-vs-double update max-rel {(gap[live] / r_d['upd'].abs()[live]).max().item():.3e} "
          f"1-beta2 rel {abs((1 - segs[0].beta2) - 0.001) / 0.001:.3e}")
    assert_close("adamw p against double hyper-parameters", d["p"].cpu()[sl], r_d["p"], r_d["s_p"], c, 0.0, extra=4 * gap)


# ====================================================================== transposed shadow
def build_table(shapes, gaps, first_off):
    """[(rows, cols)] -> int64 [nseg][4] {off, rows, cols, first_tile}, total elements, total tiles; segment i
    starts gaps[i] elements after the end of segment i - 1."""
    rows_, off, tile = [], first_off, 0
    for (r, c), gap in zip(shapes, gaps):
        off += gap
        rows_.append([off, r, c, tile])
        tile += math.ceil(r / 64) * math.ceil(c / 64)
        off += r * c
    return torch.tensor(rows_, dtype=torch.int64), off + 32, tile


def run_shadow(shapes, gaps, first_off=0, seed=3):
    table, total, tiles = build_table(shapes, gaps, first_off)
    gen = torch.Generator().manual_seed(seed)
    src = torch.randint(-32768, 32768, (total,), generator=gen, dtype=torch.int32).to(torch.int16)
    # NaN, Inf and -0 patterns at the start of every segment (the kernel moves bits and must not touch them)
    special = torch.tensor([0x7FC1, 0xFFC0, 0x7F80, 0xFF80, 0x8000, 0x0001, 0x7FFF], dtype=torch.int32).to(torch.int16)
    want = torch.full((total,), 0x5A5A, dtype=torch.int16)
    for off, r, c, _ in table.tolist():
        k = min(r * c, special.numel())
        src[off:off + k] = special[:k]
        want[off:off + r * c] = src[off:off + r * c].view(r, c).t().reshape(-1)
    srcd = src.to(DEV)
    dst = torch.full((total,), 0x5A5A, dtype=torch.int16, device=DEV)
    tabled = table.to(DEV)
    rc = L().fer_transpose_bf16_segments(srcd.data_ptr(), dst.data_ptr(), tabled.data_ptr(), len(shapes), tiles, stream())
    assert rc == 0, last_error()
    assert_bits_equal(f"shadow {shapes} at {table[:, 0].tolist()} (segments and the sentinel between them)", dst,
                      want.to(DEV))
    assert_bits_equal("shadow source unchanged", srcd, src.to(DEV))


SHADOW_SINGLE = [(64, 64), (128, 192), (136, 72), (8, 8), (70, 130), (1, 5), (129, 1), (65, 64)]


@pytest.mark.parametrize("shape", SHADOW_SINGLE, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shadow_one_segment(shape):
    """fer_transpose_bf16_segments, one segment at offset 8, uint16 patterns exact (NaN, Inf, -0 included).
    (64, 64), (128, 192): every tile takes the 16-byte fast path; (136, 72): rows and cols multiples of 8 with
    full tiles (fast) and edge tiles (the pair path) in one segment; (8, 8): multiples of 8 but no full tile;
    (70, 130), (1, 5), (129, 1), (65, 64): ragged, the pair path with its single-element edge stores (odd row
    counts put every second output row on an odd element)."""
    run_shadow([shape], [0], first_off=8)


def test_shadow_fast_shape_at_unaligned_offset():
    """(64, 64) at off % 8 == 4: the shape qualifies for 16-byte accesses, the offset does not (8-byte aligned), so
    the kernel's condition sends the tile to the pair path. This checks the result at that offset, not the branch
    taken: a 16-byte access at an 8-byte aligned address gives the same bits where the hardware allows it. Also
    an odd offset, where every second 4-byte store of the pair path would be misaligned and is split."""
    run_shadow([(64, 64)], [0], first_off=12)
    run_shadow([(64, 64)], [0], first_off=7)


@pytest.mark.parametrize("nseg", [2, 7])
def test_shadow_segment_tables(nseg):
    """2 and 7 segments in one launch with gaps between them (the block -> segment binary search on first_tile,
    fast and slow tiles of different segments side by side): the gaps and the tail keep the sentinel."""
    if nseg == 2:
        run_shadow([(64, 64), (136, 72)], [0, 16], first_off=0)
    else:
        run_shadow([(70, 130), (1, 5), (129, 1), (65, 64), (64, 64), (128, 192), (8, 8)], [0, 3, 8, 5, 10, 12, 24],
                   first_off=8)


def test_shadow_in_place_is_an_error():
    """src == dst is rejected with the entry point's message; the buffer keeps its bits."""
    table, total, tiles = build_table([(64, 64)], [0], 0)
    buf = torch.arange(total, dtype=torch.int16, device=DEV)
    tabled = table.to(DEV)
    rc = L().fer_transpose_bf16_segments(buf.data_ptr(), buf.data_ptr(), tabled.data_ptr(), 1, tiles, stream())
    assert rc != 0 and "in-place is not supported" in last_error()
    torch.cuda.synchronize()
    assert_bits_equal("shadow buffer of a rejected call", buf, torch.arange(total, dtype=torch.int16, device=DEV))
