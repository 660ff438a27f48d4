"""fer_label_change (csrc/metrics.hip) on synthetic logits: every output an integer, compared exactly with the
numpy / torch-CPU replica (latent_dirs_ref.label_change). C = 65 and 130: lanes take more than one element of a
row; n = 5 and 7 with K = 3 and 2: K * n is no multiple of the 4 waves of a block."""
import numpy as np
import pytest
import torch

import latent_dirs_ref as R
from abi_harness import DEV, NAN, last_error, lib
from fervit import ops

pytestmark = pytest.mark.gpu

CASES = [(1, 1, 1, 1), (3, 4, 5, 7), (2, 2, 7, 65), (1, 1, 3, 130), (2, 3, 9, 7)]


def logits(K, S, n, C, salt=0):
    """Base and shifted logits in which about half of the shifted rows keep the base row's argmax."""
    g = torch.Generator().manual_seed(100 * K + 10 * S + n + C + salt)
    base = torch.randn(n, C, generator=g)
    shifted = torch.randn(K * S * n, C, generator=g)
    same = torch.rand(K * S * n, generator=g) < 0.5
    shifted[same] = base.repeat(K * S, 1)[same] * 1.5
    return base, shifted


def run_raw(base, ldb, shifted, lds, K, S, n, C, preds, changed, counts, step_counts):
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    rc = lib().fer_label_change(base.data_ptr(), ldb, shifted.data_ptr(), lds, K, S, n, C, p(preds), p(changed),
                                p(counts), p(step_counts), ops.stream())
    assert rc == 0, last_error()


def check_all(base, shifted, K, S, got):
    preds, changed, counts, step_counts = R.label_change(base.numpy(), shifted.numpy(), K, S)
    assert np.array_equal(got[0].cpu().numpy(), preds)
    assert np.array_equal(got[1].cpu().numpy(), changed)
    assert np.array_equal(got[2].cpu().numpy(), counts)
    assert np.array_equal(got[3].cpu().numpy(), step_counts)


@pytest.mark.parametrize("K,S,n,C", CASES)
def test_counts_against_numpy(K, S, n, C):
    base, shifted = logits(K, S, n, C)
    got = ops.label_change(base.to(DEV), shifted.to(DEV), K, S)
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.uint8 and got[2].dtype == torch.int64
    check_all(base, shifted, K, S, got)
    if n >= 5:
        assert 0 < int(got[2].sum()) and int(got[3].sum()) < K * S * n  # both outcomes occur


def test_ties_go_to_the_lowest_index_and_nan_rows_follow_torch():
    K, S, n, C = 2, 2, 4, 70
    base = torch.zeros(n, C)
    base[0, 3] = base[0, 66] = 5.0            # tie across two lane rounds: 3
    base[1, 10] = NAN; base[1, 4] = 9.0       # noqa: E702  a NaN is the maximum: 10
    base[2, 69] = NAN; base[2, 65] = NAN      # noqa: E702  the first NaN wins: 65
    base[3] = -1.0                            # all equal: 0
    assert base.argmax(1).tolist() == [3, 10, 65, 0]
    shifted = base.repeat(K * S, 1).clone()
    shifted[1, 10] = 0.0                      # (k 0, s 0, i 1): the NaN gone -> 4, a change
    shifted[2 * n + 0, 2] = 5.0               # (k 1, s 0, i 0): an earlier tie -> 2, a change
    shifted[3 * n + 3, 69] = -1.0             # (k 1, s 1, i 3): still all equal -> 0, no change
    shifted[3 * n + 2, 64] = float("inf")     # (k 1, s 1, i 2): inf below the NaN -> still 65
    got = ops.label_change(base.to(DEV), shifted.to(DEV), K, S)
    check_all(base, shifted, K, S, got)
    assert got[2].tolist() == [1, 1] and got[3].tolist() == [[1, 0], [1, 0]]
    assert got[0][0, 0].tolist() == [3, 4, 65, 0] and got[0][1, 0, 0].item() == 2


def test_padded_row_strides():
    K, S, n, C = 3, 4, 5, 7
    base, shifted = logits(K, S, n, C, salt=1)
    bp = torch.full((n, C + 3), float("inf"), device=DEV)   # padding that would win any argmax
    sp = torch.full((K * S * n, C + 9), float("inf"), device=DEV)
    bp[:, :C] = base.to(DEV)
    sp[:, :C] = shifted.to(DEV)
    got = ops.label_change(bp[:, :C], sp[:, :C], K, S)
    check_all(base, shifted, K, S, got)


def test_two_calls_accumulate():
    K, S, n, C = 3, 4, 5, 7
    b1, s1 = logits(K, S, n, C, salt=2)
    b2, s2 = logits(K, S, n, C, salt=3)
    _, _, counts, step_counts = ops.label_change(b1.to(DEV), s1.to(DEV), K, S)
    _, _, c2, sc2 = ops.label_change(b2.to(DEV), s2.to(DEV), K, S, counts=counts, step_counts=step_counts)
    assert c2.data_ptr() == counts.data_ptr() and sc2.data_ptr() == step_counts.data_ptr()
    r1, r2 = R.label_change(b1.numpy(), s1.numpy(), K, S), R.label_change(b2.numpy(), s2.numpy(), K, S)
    assert np.array_equal(counts.cpu().numpy(), r1[2] + r2[2])
    assert np.array_equal(step_counts.cpu().numpy(), r1[3] + r2[3])
    # a chunk of the directions through offset pointers: rows of direction 1 alone, added onto counts[1:2]
    before = counts.clone()
    ops.label_change(b1.to(DEV), s1.to(DEV)[S * n:2 * S * n], 1, S, counts=counts[1:2], step_counts=step_counts[1:2])
    assert counts.tolist() == [before[0].item(), before[1].item() + int(r1[2][1]), before[2].item()]


@pytest.mark.parametrize("which", ["preds", "changed", "step_counts", "none"])
def test_each_optional_output_alone(which):
    K, S, n, C = 2, 2, 7, 65
    base, shifted = logits(K, S, n, C, salt=4)
    bd, sd = base.to(DEV), shifted.to(DEV)
    full = ops.label_change(bd, sd, K, S)
    preds = torch.empty(K, S, n, dtype=torch.int64, device=DEV) if which == "preds" else None
    changed = torch.empty(K, n, dtype=torch.uint8, device=DEV) if which == "changed" else None
    step_counts = torch.zeros(K, S, dtype=torch.int64, device=DEV) if which == "step_counts" else None
    counts = torch.zeros(K, dtype=torch.int64, device=DEV)
    run_raw(bd, C, sd, C, K, S, n, C, preds, changed, counts, step_counts)
    assert torch.equal(counts, full[2])
    for got, want in ((preds, full[0]), (changed, full[1]), (step_counts, full[3])):
        assert got is None or torch.equal(got, want)


def test_argument_errors():
    K, S, n, C = 2, 2, 3, 7
    base, shifted = (t.to(DEV) for t in logits(K, S, n, C))
    counts = torch.zeros(K, dtype=torch.int64, device=DEV)
    L = lib()
    args = dict(base=base.data_ptr(), ldb=C, shifted=shifted.data_ptr(), lds=C, K=K, S=S, n=n, C=C, preds=None,
                changed=None, counts=counts.data_ptr(), step_counts=None)
    for over in (dict(K=0), dict(S=0), dict(C=0), dict(ldb=C - 1), dict(lds=C - 1), dict(base=None),
                 dict(shifted=None), dict(counts=None)):
        rc = L.fer_label_change(*{**args, **over}.values(), ops.stream())
        assert rc != 0 and last_error().startswith("label_change:"), (over, last_error())
    assert L.fer_label_change(*{**args, "n": 0}.values(), ops.stream()) == 0
    torch.cuda.synchronize()
    assert counts.tolist() == [0, 0]
