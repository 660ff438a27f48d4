"""The linear-SVM restatement of tests/svm_ref.py checked without a GPU: its optimum is sklearn's LinearSVC
optimum, slipped problems fail the optimality gate of tests/test_gpu_svm_fit.py, the directions file round-trips
through LatentDecomposer.from_file, and the entry points are declared."""
import os
import re

import numpy as np
import pytest
import torch

import svm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 7


@pytest.mark.parametrize("method", ["binary", "multiclass"])
@pytest.mark.parametrize("N,F", [(192, 300), (600, 96)])
def test_restatement_optimum_is_linearsvc_optimum(N, F, method):
    """LinearSVC(C=0.1, class_weight='balanced', tol=1e-10) against the dense-Newton optimum of the restatement:
    1e-6 absolute on coef_ and intercept_ (measured 2.5e-12 to 8e-8)."""
    svm = pytest.importorskip("sklearn.svm")
    import warnings

    X, y = R.gaussian_classes(N, F, K, seed=N + F)
    s, c, reg = R.problem(y, K, method)
    W, b = R.newton(X, s, c, reg)
    assert R.relative_gradient(X, W, b, s, c, reg).max() <= 1e-10
    Xd = X.astype(np.float64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if method == "multiclass":
            m = svm.LinearSVC(max_iter=200000, C=0.1, class_weight="balanced", tol=1e-10).fit(Xd, y)
            coef, icpt = m.coef_, m.intercept_
        else:
            fits = [svm.LinearSVC(max_iter=200000, C=0.1, class_weight="balanced", tol=1e-10).fit(Xd, (y == k).astype(int))
                    for k in range(K)]
            coef, icpt = np.stack([f.coef_[0] for f in fits]), np.array([f.intercept_[0] for f in fits])
    err = max(np.abs(coef - W).max(), np.abs(icpt - b).max())
    print(f"svm-ref ({N},{F}) {method}: max |sklearn - restatement| = {err:.2e}")
    assert err <= 1e-6


def slipped(y, method, slip):
    """(s, c, reg_bias) of the method's problem with one slip built in."""
    s, c, reg = R.problem(y, K, method)
    if slip == "negatives weighted like binary":
        assert method == "multiclass"
        _, cn = R.weights(y, K, "binary")
        c = np.where(s > 0, c, cn[None, :])
    elif slip == "unregularised bias":
        reg = False
    elif slip == "wrong sign for one class":
        s = s.copy()
        s[:, 3] = -s[:, 3]
    elif slip == "C not multiplied in":
        c = c / 0.1
    return s, c, reg


@pytest.mark.parametrize("method,slip", [("multiclass", "negatives weighted like binary"), ("binary", "unregularised bias"),
                                         ("multiclass", "unregularised bias"), ("binary", "wrong sign for one class"),
                                         ("multiclass", "wrong sign for one class"), ("binary", "C not multiplied in"),
                                         ("multiclass", "C not multiplied in")])
def test_slipped_problems_fail_the_gate(method, slip):
    """The optimum of a slipped problem, held against the true problem's gradient, lies above the gate's cap in
    at least one class (every class but for the one-class slip): the gate of the GPU test discriminates."""
    X, y = R.gaussian_classes(600, 96, K, seed=600 + 96)
    s, c, reg = R.problem(y, K, method)
    Ws, bs = R.newton(X, *slipped(y, method, slip))
    rel = R.relative_gradient(X, Ws, bs, s, c, reg)
    print(f"svm-slip {method} / {slip}: relative gradient {['%.2e' % v for v in rel]}")
    assert R.GATE <= R.GATE_CAP
    if slip == "wrong sign for one class":
        assert rel[3] > R.GATE_CAP
    else:
        assert (rel > R.GATE_CAP).all(), rel
    # and the true optimum passes it by orders of magnitude
    W, b = R.newton(X, s, c, reg)
    assert R.relative_gradient(X, W, b, s, c, reg).max() <= 1e-10


def test_weights_are_the_balanced_class_weights():
    from fervit.directions import class_weights

    y = np.array([0, 0, 0, 1, 2, 2])
    cp, cn = R.weights(y, 3, "binary", 0.1)
    assert np.allclose(cp, [0.1, 0.3, 0.15]) and np.allclose(cn, [0.1, 0.06, 0.075])
    cp, cn = R.weights(y, 3, "multiclass", 0.1)
    assert np.allclose(cp, [0.1 * 6 / 9, 0.1 * 6 / 3, 0.1 * 6 / 6]) and np.allclose(cn, 0.1)
    for method in ("binary", "multiclass"):
        a, b = class_weights(np.bincount(y), method, 0.1)
        assert np.array_equal(a.numpy(), R.weights(y, 3, method)[0]) and np.array_equal(b.numpy(), R.weights(y, 3, method)[1])


def test_save_directions_round_trips_through_the_decomposer(tmp_path):
    """Keys and shapes of the reference's file; loads with weights_only=True (LatentDecomposer.from_file)."""
    from fervit.directions import EMOTION_NAMES, save_directions
    from models_fer_vit.latent_decomposer import LatentDecomposer

    g = torch.Generator().manual_seed(0)
    dirs = {k: torch.nn.functional.normalize(torch.randn(18 * 512, generator=g), dim=0) for k in range(K)}
    path = save_directions(dirs, str(tmp_path / "directions"), "multiclass")
    assert path == str(tmp_path / "directions" / "multiclass_directions.pt")
    data = torch.load(path, map_location="cpu", weights_only=True)
    assert set(data) == {"directions", "emotion_names", "seq_len", "latent_dim", "method"}
    assert data["seq_len"] == 18 and data["latent_dim"] == 512 and data["method"] == "multiclass"
    assert data["emotion_names"] == EMOTION_NAMES and sorted(data["directions"]) == list(range(K))
    for k in range(K):
        d = data["directions"][k]
        assert d.shape == (18, 512) and d.dtype == torch.float32 and torch.equal(d.reshape(-1), dirs[k])
    dec = LatentDecomposer.from_file(path)
    assert dec.directions.shape == (K, 18, 512)
    assert (dec.directions.reshape(K, -1) - torch.stack([dirs[k] for k in range(K)])).abs().max() <= 1e-6
    # numpy directions (the reference's type) are taken as well
    p2 = save_directions({k: v.numpy() for k, v in dirs.items()}, str(tmp_path), "binary", 18, 512)
    assert torch.equal(torch.load(p2, weights_only=True)["directions"][3], dirs[3].view(18, 512))


def test_fit_raises_on_cpu_tensors():
    from fervit import ops
    from fervit.directions import fit_linear_svm

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fit_linear_svm(torch.zeros(8, 4), torch.zeros(8, dtype=torch.int64), 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.svm_xtr(torch.zeros(8, 4), torch.zeros(8, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.svm_hinge(torch.zeros(8, 4), torch.zeros(2, 4), torch.zeros(2), torch.zeros(8, dtype=torch.int64),
                      torch.arange(2), torch.ones(2), torch.ones(2))


def test_header_declares_the_entry_points():
    src = open(os.path.join(ROOT, "include", "fervit.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("fer_svm_forward", "fer_svm_xtr", "fer_svm_slab", "fer_svm_max_groups"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
    assert re.search(r"\bint64_t\s+fer_svm_ws\s*\(", code)
    assert not re.search(r"fer_svm_\w+\s*\(\s*int\s+dtype\b", code)  # neither entry point takes a dtype
    assert "compute_expression_direction.py:58-116" in src
    from fervit._lib import SIGNATURES

    assert {"fer_svm_forward", "fer_svm_xtr", "fer_svm_ws", "fer_svm_slab", "fer_svm_max_groups"} <= set(SIGNATURES)
