"""float64 numpy restatements of the three evaluation ops (include/fervit.h fer_cls_stats, fer_cls_report,
fer_token_cosine), shared by tests/test_metrics_ref_cpu.py (against sklearn and float64 torch) and the GPU
tests (against the kernels)."""
import numpy as np


# ---------------------------------------------------------------------- fer_cls_stats
def argmax_ref(z):
    """Lowest index of the row maximum of z [B, C]; a NaN counts as the maximum, the first NaN wins
    (torch.argmax on the CPU)."""
    z = np.asarray(z)
    out = np.zeros(z.shape[0], np.int64)
    for b, row in enumerate(z):
        nan = np.flatnonzero(np.isnan(row))
        out[b] = nan[0] if nan.size else int(np.flatnonzero(row == row.max())[0])
    return out


def softmax_ref(z):
    """(probs [B, C], scale [B, C]) in float64 from the values z holds: probs_i = exp(z_i - m) / sum_j exp(z_j - m),
    scale_i = probs_i (1 + |z_i - m|), the size of an fp32 evaluation's error per unit 2^-23. A row with a
    NaN is all NaN."""
    z = np.asarray(z, np.float64)
    with np.errstate(invalid="ignore"):
        m = np.where(np.isnan(z).any(1), np.nan, np.nanmax(np.where(np.isnan(z), -np.inf, z), axis=1))[:, None]
        e = np.exp(z - m)
        p = e / e.sum(1, keepdims=True)
        return p, p * (1.0 + np.abs(z - m))


def cls_stats_ref(z, labels):
    """preds, conf, probs, scale, confusion [C, C] (row = label, column = prediction), counters (counted,
    skipped) of one batch."""
    z = np.asarray(z)
    labels = np.asarray(labels, np.int64)
    C = z.shape[1]
    preds = argmax_ref(z)
    probs, scale = softmax_ref(z)
    rows = np.arange(z.shape[0])
    ok = (labels >= 0) & (labels < C)
    cm = np.zeros((C, C), np.int64)
    np.add.at(cm, (labels[ok], preds[ok]), 1)
    return {"preds": preds, "conf": probs[rows, preds], "conf_scale": scale[rows, preds], "probs": probs,
            "scale": scale, "confusion": cm, "counters": np.array([ok.sum(), (~ok).sum()], np.int64)}


# ---------------------------------------------------------------------- fer_cls_report
def report_ref(cm):
    """float64 [4 + 4 C]: accuracy, f1_macro, f1_weighted, n, then precision, recall, f1, support per class.
    A zero denominator gives 0; f1_macro averages over the classes with row sum + column sum > 0."""
    cm = np.asarray(cm, np.int64)
    C = cm.shape[0]
    rs, cs, tp = cm.sum(1), cm.sum(0), np.diag(cm)
    n = int(rs.sum())

    def div(a, b):
        return np.where(b > 0, a.astype(np.float64) / np.maximum(b, 1).astype(np.float64), 0.0)

    prec, rec, f1 = div(tp, cs), div(tp, rs), div(2 * tp, rs + cs)
    present = int(((rs + cs) > 0).sum())
    out = np.zeros(4 + 4 * C, np.float64)
    out[0] = tp.sum() / n if n else 0.0
    out[1] = f1.sum() / present if present else 0.0
    out[2] = (f1 * rs).sum() / n if n else 0.0
    out[3] = n
    out[4:] = np.stack([prec, rec, f1, rs.astype(np.float64)], 1).reshape(-1)
    return out


# ---------------------------------------------------------------------- fer_token_cosine
def cosine_ref(x, eps=1e-8):
    """x [B, N, D] (the values the tokens hold) -> (cls_sim [B, N-1], tok_sim [B, N-1, N-1], their scales):
    cos(x, y) = x.y / (max(|x|, eps) max(|y|, eps)), scale = sum_k |x_k y_k| over the same denominator."""
    x = np.asarray(x, np.float64)
    nrm = np.maximum(np.sqrt((x * x).sum(-1)), eps)
    den = nrm[:, :, None] * nrm[:, None, :]
    cos = np.einsum("bik,bjk->bij", x, x) / den
    scale = np.einsum("bik,bjk->bij", np.abs(x), np.abs(x)) / den
    return cos[:, 0, 1:], cos[:, 1:, 1:], scale[:, 0, 1:], scale[:, 1:, 1:]
