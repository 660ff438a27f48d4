"""Host parts of the SeFa pipeline (fervit.sefa): the factorisation against numpy, the draw replica's
distribution, the selection rule, and the header's three new entry points. No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import latent_dirs_ref as R
from fervit.sefa import factorize_weight, select_directions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def seeded_weight():
    """24 x 16 with a spectrum that is distinct by construction: orthogonal factors around singular values
    16, 15, ..., 1 (eigenvalues of A^T A: their squares, gaps of at least 3)."""
    rng = np.random.default_rng(20240611)
    U, _ = np.linalg.qr(rng.standard_normal((24, 16)))
    V, _ = np.linalg.qr(rng.standard_normal((16, 16)))
    return (U * np.arange(16, 0, -1.0)) @ V.T


def check_against_eigh(A, got, K):
    A64 = A.astype(np.float64)
    ATA = A64.T @ A64
    w, v = np.linalg.eigh(ATA)
    w, v = w[::-1], v[:, ::-1]
    assert np.all(np.diff(w) < -1e-3 * w[0]), "the test needs a distinct spectrum"
    ev, dirs = got["eigenvalues"], got["directions"]
    assert ev.dtype == np.float32 and dirs.dtype == np.float32
    assert ev.shape == (K,) and dirs.shape == (K, A.shape[1])
    assert np.all(np.diff(ev) < 0), "eigenvalues descending"
    # the float32 cast of the float64 eigenvalue: half an fp32 ulp of it, plus eigh's own backward error
    # (a few fp64 ulps of lambda_max, far below)
    assert np.all(np.abs(ev.astype(np.float64) - w[:K]) <= 2.0 ** -24 * np.abs(w[:K]) + 1e-12 * w[0])
    for k in range(K):
        d = dirs[k].astype(np.float64)
        sign = 1.0 if d @ v[:, k] > 0 else -1.0
        # each component rounded to fp32 (|component| <= 1: 2^-24 absolute) on top of the eigensolver's error,
        # which the spectral gap (>= 3 against lambda_max = 256) keeps at a few hundred fp64 ulps
        assert np.abs(sign * d - v[:, k]).max() <= 2.0 ** -24 + 1e-12
        assert np.abs(ATA @ d - w[k] * d).max() <= 2.0 ** -22 * w[0]


def test_factorize_weight_matches_numpy_eigh():
    A = seeded_weight()
    check_against_eigh(A, factorize_weight(A, num_semantics=5), 5)
    check_against_eigh(A, factorize_weight(torch.from_numpy(A), num_semantics=16), 16)


def test_factorize_weight_layer_idx_slices_rows():
    A = seeded_weight()
    rows = [0, 3, 4, 7, 8, 9, 11, 12, 13, 15, 16, 17, 19, 20, 21, 22, 23, 2]  # 18 rows: A[rows]^T A[rows] full rank
    got = factorize_weight(A, layer_idx=rows, num_semantics=4)
    ref = factorize_weight(A[rows], num_semantics=4)
    assert np.array_equal(got["eigenvalues"], ref["eigenvalues"]) and np.array_equal(got["directions"], ref["directions"])
    full = factorize_weight(A, num_semantics=4)
    assert not np.array_equal(got["eigenvalues"], full["eigenvalues"])
    w = np.linalg.eigvalsh(A[rows].T @ A[rows])[::-1]
    assert np.all(np.abs(got["eigenvalues"].astype(np.float64) - w[:4]) <= 2.0 ** -24 * w[:4] + 1e-12 * w[0])


def test_factorize_weight_rejects_bad_counts():
    A = seeded_weight()
    for k in (17, 0, -1):
        with pytest.raises(ValueError):
            factorize_weight(A, num_semantics=k)
    with pytest.raises(ValueError):
        factorize_weight(np.zeros(16), num_semantics=1)


def test_draw_replica_distribution():
    """2^16 indices, p_keep = 1/17, 16 choices: the -1 share within 5 binomial standard deviations of p_keep,
    and each choice's share of the rest within 5 binomial standard deviations of 1/16."""
    n, p, nc = 1 << 16, 1.0 / 17.0, 16
    c = R.dir_draw(0x5EED0123456789, n, nc, p)
    assert c.dtype == np.int32 and c.min() >= -1 and c.max() < nc
    kept = int((c == -1).sum())
    assert abs(kept - n * p) <= 5.0 * np.sqrt(n * p * (1 - p)), kept
    rest = n - kept
    counts = np.bincount(c[c >= 0], minlength=nc)
    q = 1.0 / nc
    assert np.all(np.abs(counts - rest * q) <= 5.0 * np.sqrt(rest * q * (1 - q))), counts
    # the ends of the keep probability, and a different seed draws differently
    assert np.all(R.dir_draw(7, 1000, nc, 1.0) == -1) and np.all(R.dir_draw(7, 1000, nc, 0.0) >= 0)
    assert not np.array_equal(R.dir_draw(7, 1000, nc, p), R.dir_draw(8, 1000, nc, p))
    assert np.all(R.dir_draw(7, 1000, 1, 0.0) == 0)


def test_select_directions():
    res = [{"direction_idx": 0, "label_change_rate": 0.0}, {"direction_idx": 1, "label_change_rate": 0.3},
           {"direction_idx": 2, "label_change_rate": 0.05}, {"direction_idx": 5, "label_change_rate": 0.051}]
    assert select_directions(res, 0.05) == [0, 2]
    assert select_directions(res, 1.0) == [0, 1, 2, 5]
    assert select_directions(res, -1.0) == [] and select_directions([], 0.5) == []


def test_header_names_the_new_entry_points():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fervit.h")).read(), flags=re.S)
    from fervit._lib import SIGNATURES

    for name in ("fer_latent_shift", "fer_latent_dir_draw", "fer_label_change"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in SIGNATURES


def test_drop_in_modules_export_the_reference_names():
    import sefa
    import sefa.factorize
    import sefa.verify_directions
    from fervit import sefa as S

    assert sefa.factorize.factorize_stylegan_weights is S.factorize_stylegan_weights
    assert sefa.verify_directions.verify_non_expression_directions is S.verify_non_expression_directions
    assert sefa.factorize_weight is S.factorize_weight
