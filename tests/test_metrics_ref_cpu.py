"""CPU checks of the evaluation metrics: the float64 restatements the GPU tests compare the kernels with
(tests/metrics_ref.py) against sklearn and float64 torch on the cases include/fervit.h names, the wrappers'
refusal of CPU tensors, and the header's declarations."""
import os
import re
import warnings

import numpy as np
import pytest
import torch

import metrics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sk_report(labels, preds):
    from sklearn.metrics import accuracy_score, f1_score, precision_recall_fscore_support

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        acc = accuracy_score(labels, preds)
        mac = f1_score(labels, preds, average="macro")
        wei = f1_score(labels, preds, average="weighted")
        present = np.unique(np.concatenate([labels, preds]))
        p, r, f, s = precision_recall_fscore_support(labels, preds, labels=present, zero_division=0)
    return acc, mac, wei, present, p, r, f, s


def confusion_of(labels, preds, C):
    cm = np.zeros((C, C), np.int64)
    np.add.at(cm, (labels, preds), 1)
    return cm


def report_cases():
    g = np.random.default_rng(0)
    cases = {}
    for C, n in ((2, 50), (7, 400), (33, 1000)):
        cases[f"random C={C}"] = (g.integers(0, C, n), g.integers(0, C, n), C)
    cases["issue example"] = (np.array([0, 0, 1, 3]), np.array([0, 1, 1, 1]), 4)  # class 2 absent from both
    lab = g.integers(0, 7, 300)
    pred = g.integers(0, 7, 300)
    lab[lab == 4], pred[pred == 4] = 5, 3
    cases["class absent from labels and predictions"] = (lab, pred, 7)
    pred2 = g.integers(0, 7, 300)
    pred2[pred2 == 2] = 6
    cases["class never predicted"] = (g.integers(0, 7, 300), pred2, 7)
    cases["single class"] = (np.zeros(20, np.int64), np.zeros(20, np.int64), 1)
    cases["single class of several"] = (np.full(20, 3), np.full(20, 3), 7)
    return cases


@pytest.mark.parametrize("name", list(report_cases()))
def test_report_restatement_equals_sklearn(name):
    labels, preds, C = report_cases()[name]
    out = R.report_ref(confusion_of(labels, preds, C))
    acc, mac, wei, present, p, r, f, s = sk_report(labels, preds)
    assert abs(out[0] - acc) <= 1e-12 and abs(out[1] - mac) <= 1e-12 and abs(out[2] - wei) <= 1e-12
    assert out[3] == len(labels)
    per = out[4:].reshape(C, 4)
    for got, want in zip(per[present].T, (p, r, f, s)):
        assert np.abs(got - want).max() <= 1e-12
    absent = np.setdiff1d(np.arange(C), present)
    assert (per[absent] == 0).all()


def test_report_issue_example_figures_and_empty_matrix():
    out = R.report_ref(confusion_of(np.array([0, 0, 1, 3]), np.array([0, 1, 1, 1]), 4))
    assert abs(out[1] - 0.38889) < 1e-5 and abs(out[2] - 0.45833) < 1e-5
    z = R.report_ref(np.zeros((5, 5), np.int64))
    assert (z == 0).all() and not np.isnan(z).any()


def test_argmax_restatement_equals_torch():
    nan = float("nan")
    rows = [[1, 5, 5, 2], [1, nan, 5, nan], [nan, nan, 0, 0], [-np.inf, -np.inf, -np.inf, -np.inf], [0, 0, 0, 0],
            [3, 1, 2, 3]]
    z = np.array(rows, np.float32)
    assert R.argmax_ref(z).tolist() == [1, 1, 0, 0, 0, 0]
    assert R.argmax_ref(z).tolist() == torch.from_numpy(z).double().argmax(1).tolist()
    g = torch.Generator().manual_seed(1)
    w = torch.randn(64, 33, generator=g).round()  # many exact ties
    assert R.argmax_ref(w.numpy()).tolist() == w.double().argmax(1).tolist()


def test_softmax_restatement_equals_torch():
    g = torch.Generator().manual_seed(2)
    z = torch.randn(17, 7, generator=g) * 30
    p, scale = R.softmax_ref(z.numpy())
    assert np.abs(p - torch.softmax(z.double(), 1).numpy()).max() <= 1e-15
    assert (scale >= p).all()
    z[3, 2] = float("nan")
    p, _ = R.softmax_ref(z.numpy())
    assert np.isnan(p[3]).all() and not np.isnan(np.delete(p, 3, 0)).any()


def test_cls_stats_restatement_skips_labels_outside_the_classes():
    z = np.array([[0, 1, 0], [2, 0, 0], [0, 0, 3], [0, 4, 0], [5, 0, 0]], np.float32)
    r = R.cls_stats_ref(z, [1, -100, 3, -1, 2])
    assert r["preds"].tolist() == [1, 0, 2, 1, 0] and r["counters"].tolist() == [2, 3]
    assert r["confusion"].tolist() == [[0, 0, 0], [0, 1, 0], [1, 0, 0]]
    assert np.array_equal(r["conf"], r["probs"][np.arange(5), r["preds"]])


def test_cosine_restatement_equals_torch():
    """torch.cosine_similarity in float64, including its per-vector clamp: (3e-9, 0) . (1, 0) = 0.3 at eps 1e-8."""
    x = torch.tensor([[[3e-9, 0.0], [1.0, 0.0], [0.0, 0.0], [0.0, 2.0]]], dtype=torch.float64)
    cls, tok, cs, ts = R.cosine_ref(x.numpy(), 1e-8)
    assert abs(cls[0, 0] - 0.3) <= 1e-15 and cls[0, 1] == 0 and cls[0, 2] == 0
    assert (tok[0, 1] == 0).all() and (tok[0, :, 1] == 0).all()  # the zero row: 0, not NaN
    g = torch.Generator().manual_seed(3)
    y = torch.randn(2, 10, 64, generator=g, dtype=torch.float64)
    y[0, 4] = 0
    y[1, 2] *= 1e-10
    y[1, 7] = y[1, 3]
    for t in (x, y):
        cls, tok, cs, ts = R.cosine_ref(t.numpy(), 1e-8)
        want_cls = torch.cosine_similarity(t[:, :1], t[:, 1:], dim=2, eps=1e-8)
        want_tok = torch.cosine_similarity(t[:, 1:].unsqueeze(2), t[:, 1:].unsqueeze(1), dim=3, eps=1e-8)
        assert np.abs(cls - want_cls.numpy()).max() <= 1e-14
        assert np.abs(tok - want_tok.numpy()).max() <= 1e-14
        assert (cs >= np.abs(cls) - 1e-15).all() and (ts >= np.abs(tok) - 1e-15).all()
    assert abs(R.cosine_ref(y.numpy())[1][1, 6, 2] - 1.0) <= 1e-15  # two identical rows


def test_wrappers_and_meter_raise_on_cpu_tensors():
    from fervit import layers, ops
    from fervit.metrics import ClassificationMeter

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cls_stats(torch.zeros(4, 7), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cls_report(torch.zeros(7, 7, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.token_cosine(torch.zeros(1, 4, 32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ClassificationMeter(7, "cpu")
    assert layers.TOKEN_TAP is None and layers.ATTN_TAP is None


def test_header_declares_the_entry_points_and_cites_the_reference():
    src = open(os.path.join(ROOT, "include", "fervit.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("fer_cls_stats", "fer_cls_report", "fer_token_cosine"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
    assert "eval/evaluate_model.py:135-159" in src and "eval/evaluate_model.py:231-296" in src
    from fervit._lib import SIGNATURES

    assert {"fer_cls_stats", "fer_cls_report", "fer_token_cosine"} <= set(SIGNATURES)


def test_classification_summary_equals_sklearn_report():
    """eval.evaluate_model.classification_summary on a meter's report (here the restatement's figures in the
    meter's layout): sklearn's classification_report(output_dict=True), key by key."""
    from sklearn.metrics import classification_report

    from eval.evaluate_model import classification_summary

    labels, preds, C = report_cases()["class absent from labels and predictions"]
    cm = confusion_of(labels, preds, C)
    out = R.report_ref(cm)
    per = out[4:].reshape(C, 4)

    class Meter:
        num_classes = C

        def compute(self):
            return {"accuracy": out[0], "f1_macro": out[1], "f1_weighted": out[2], "n": int(out[3]),
                    "per_class": {"precision": per[:, 0].tolist(), "recall": per[:, 1].tolist(),
                                  "f1": per[:, 2].tolist(), "support": [int(v) for v in per[:, 3]]},
                    "confusion": cm, "skipped": 0}

    names = [f"c{i}" for i in range(C)]
    got = classification_summary(Meter(), names)
    present = np.unique(np.concatenate([labels, preds]))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = classification_report(labels, preds, labels=present, target_names=[names[i] for i in present],
                                     output_dict=True, zero_division=0)
    assert got["test_dataset_size"] == len(labels) and abs(got["accuracy"] - want["accuracy"]) <= 1e-12
    rep = got["classification_report"]
    assert set(rep) == set(want)
    for k, v in want.items():
        if k == "accuracy":
            assert abs(rep[k] - v) <= 1e-12
            continue
        for kk, vv in v.items():
            assert abs(rep[k][kk] - vv) <= 1e-12, (k, kk)
