"""The attention size queries against their formulas, on the CPU (the library loads without a GPU and
neither query makes a HIP call). fer_attention_saved_floats is the contract between the forward, which
writes the dropout keep bits behind lse, and the backward, which reads them: the formulas below are
written out independently of the library's dispatch plan (attn_plan() in csrc/attention.hip), with shapes
on both sides of every boundary of that plan."""
import itertools
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "fer-vit_amd", "fervit", "libfervit.so")
BF16, F32 = 0, 1

NS = (1, 32, 33, 96, 97, 224, 225, 256, 257)
DHS = (8, 64, 72, 128)
THRS = (0, 6554)
UNITS = ((1, 1), (2, 3))  # (B, H): B*H = 1 and 6


def saved_floats(dtype, B, N, H, dh, thr):
    lse = -(-B * H * N // 64) * 64
    nb = -(-N // 32)
    keep_bits = dtype == BF16 and thr != 0 and N <= 224 and dh <= 64
    return lse + (B * H * nb * nb * 32 if keep_bits else 0)


@pytest.mark.skipif(not os.path.exists(LIB), reason="libfervit.so not built")
@pytest.mark.parametrize("dtype", [BF16, F32])
def test_attention_saved_floats_and_ws_follow_their_formulas(dtype):
    from fervit._lib import lib

    L = lib()
    try:
        for fwd_kernel in (0, 1, 2):  # the forward kernel choice moves no size
            assert L.fer_attention_set_fwd_kernel(fwd_kernel) == 0
            for (B, H), N, dh, thr in itertools.product(UNITS, NS, DHS, THRS):
                got = L.fer_attention_saved_floats(dtype, B, N, H, dh, thr)
                assert got == saved_floats(dtype, B, N, H, dh, thr), (dtype, B, N, H, dh, thr, fwd_kernel, got)
    finally:
        L.fer_attention_set_fwd_kernel(0)
    for (B, H), N in itertools.product(UNITS, NS):
        # fp32: the P and dS slabs; then the larger of the stand-alone column-sum pass's partials over
        # [B*N][3*H*128] and the fused bias-gradient partials [B][7][3*H*64] fp32
        slabs = 2 * B * H * N * N * 4 if dtype == F32 else 0
        colsum = max(L.fer_colsum_ws(B * N, 3 * H * 128), B * 7 * 3 * H * 64 * 4)
        assert L.fer_attention_ws(dtype, B, N, H) == slabs + colsum, (dtype, B, N, H)
