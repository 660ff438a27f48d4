"""The host mirror of fer_mixup_draw (tests/mixup_ref.py) on its own, without a GPU: its permutation is one, its
lam follows Beta(alpha, alpha) by a Kolmogorov-Smirnov gate that can fail, its permutations fill every
(i, perm[i]) cell evenly, no draw runs out of attempts, and few enough draws sit on an accept / reject boundary
for the GPU test to leave them out. The GPU tests (tests/test_gpu_mixup_kernels.py) hold the kernel to this
mirror and apply the same gates to the device's own draws. DESIGN.md section 2.14."""
import functools
import math
import os
import re

import numpy as np
import pytest

import mixup_ref as R

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fer-vit_amd", "csrc")


@functools.lru_cache(maxsize=None)
def draws(alpha):
    return R.lam_draws(alpha)


@pytest.mark.parametrize("B", [1, 2, 5, 64, 257, 2048])
def test_mirror_perm_is_a_permutation(B):
    for s in range(3):
        p = R.perm(R.stream_seed(R.SEED, s), B)
        assert p.dtype == np.int32 and sorted(p.tolist()) == list(range(B))
    if B <= 257:  # the sort against the kernel's own rule, pair by pair
        ss = R.stream_seed(R.SEED, 7)
        assert (R.perm(ss, B) == R.perm_by_definition(ss, B)).all()


def test_mirror_perm_breaks_ties_on_the_index(monkeypatch):
    """All keys equal: the rank is the index."""
    monkeypatch.setattr(R, "fer_hash", lambda seed, pair: np.full(len(pair), 5, dtype=np.uint64))
    assert R.perm(1, 9).tolist() == list(range(9)) == R.perm_by_definition(1, 9).tolist()


def test_constants_are_the_kernels():
    src = open(os.path.join(CSRC, "mixup.hip")).read()
    assert f"MIXUP_ATTEMPTS = {R.ATTEMPTS};" in src and f"MIXUP_MAX_B = {R.MAX_B};" in src
    for c in (R.PERM_XOR, *R.GAMMA_XOR):
        assert f"0x{c:016X}ull" in src
    hdr = open(os.path.join(CSRC, "step_seed.h")).read()
    assert re.search(r"step_stream_seed\(uint64_t seed, uint64_t s\)\s*\{\s*uint64_t z = step_seed\(seed\) \^ "
                     r"\(s \* 0x9E3779B97F4A7C15ull\);", hdr)


def test_ks_limit():
    assert R.KS_LIMIT == pytest.approx(0.0421, abs=5e-5)


@pytest.mark.parametrize("alpha", [0.5, 1.0, 2.0])
def test_mirror_lam_is_beta(alpha):
    lam, capped, _ = draws(alpha)
    assert ((lam >= 0) & (lam <= 1)).all()
    D = R.ks_statistic(lam, R.CDF[alpha])
    print(f"KS alpha={alpha}: D = {D:.4f} (limit {R.KS_LIMIT:.4f})")
    assert D < R.KS_LIMIT
    assert not capped.any()


def test_ks_gate_can_fail():
    D = R.ks_statistic(draws(0.5)[0], R.CDF[1.0])
    print(f"KS alpha=0.5 draws against the alpha=1 CDF: D = {D:.4f}")
    assert D > R.KS_LIMIT


def test_mirror_lam_is_one_without_mixup():
    for alpha in (0.0, -1.0, float("nan")):
        assert R.lam(R.stream_seed(R.SEED, 0), alpha)[0] == 1.0


def test_mirror_perm_cells_are_even():
    perms = np.stack([R.perm(R.stream_seed(R.SEED, s), 5) for s in range(R.N_DRAWS)])
    R.cell_gate(perms)
    skew = perms.copy()
    skew[:600, 0] = 0  # 600 more hits in one cell: outside 6 sigma (153.6)
    with pytest.raises(AssertionError):
        R.cell_gate(skew)


@pytest.mark.parametrize("alpha", [0.5, 1.0, 2.0])
def test_few_draws_sit_on_a_boundary(alpha):
    """The GPU test leaves out draws whose margin is below MARGIN; at most 1 % may be."""
    _, _, margin = draws(alpha)
    share = float((margin < R.MARGIN).mean())
    print(f"alpha={alpha}: {share:.4%} of the draws within {R.MARGIN:g} of an accept / reject boundary")
    assert share <= 0.01


def test_step_counter_and_set_change_the_draw():
    a = R.draw(R.SEED, 1.0, 64)
    assert R.draw(R.SEED, 1.0, 64)[0] == a[0] and (R.draw(R.SEED, 1.0, 64)[1] == a[1]).all()
    for other in (R.draw(R.SEED, 1.0, 64, s=1), R.draw(R.SEED, 1.0, 64, counter=0), R.draw(R.SEED, 1.0, 64, counter=1)):
        assert other[0] != a[0] and (other[1] != a[1]).any()
    assert math.isfinite(R.lam(R.stream_seed(R.SEED, 3), 1e-3)[0])  # the log form: no 0 / 0 at a tiny alpha
