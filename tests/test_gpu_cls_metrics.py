"""fer_cls_stats and fer_cls_report against the float64 restatements of tests/metrics_ref.py, through the raw
C ABI with padded strides (tests/abi_harness.py), and ClassificationMeter under graph capture.

One kernel serves every B and C of fer_cls_stats (a wave per row, lanes striding the row), so there is no
dispatch threshold; the sizes still straddle what the code counts in: 4 rows per workgroup (B = 63, 64, 65)
and 64 lanes per row (C = 33, 64, 65, 1000).

Bounds. preds, confusion and counters are exact. probs and conf: c 2^-23 scale_i + 2^-149 with
scale_i = p_i (1 + |z_i - m|) (an exponential's argument error scales with |z_i - m|), c from float32 torch's
CPU softmax against the same float64 restatement (x 4, floor 16); 2^-149 is one
fp32 denormal step. fer_cls_report: (C + 8) 2^-52 relative (a sum of C non-negative fp64 terms in another
order, plus a handful of roundings)."""
import numpy as np
import pytest
import torch

import metrics_ref as R
from abi_harness import DEV, NAN, all_nan, last_error, lib, nanvec, nanview, ops, ptr, untouched, untouched_vec
from elemwise import assert_bits_equal, assert_close, measure_c

pytestmark = pytest.mark.gpu

SENT = -7777  # what the int64 parents are filled with (they cannot hold a NaN)
TINY = 2.0 ** -149
KINDS = ("randn", "x1e4", "ties", "nan")


def intview(n, zero=False, guard=4):
    """[n] int64 view inside a SENT-filled parent with `guard` elements on each side; returns (view, parent)."""
    parent = torch.full((n + 2 * guard,), SENT, dtype=torch.int64, device=DEV)
    v = parent[guard:guard + n]
    if zero:
        v.zero_()
    return v, parent


def int_untouched(name, parent, n, guard=4):
    p = parent.cpu()
    assert (p[:guard] == SENT).all() and (p[guard + n:] == SENT).all(), f"{name}: guard elements were written"


def logits_of(kind, B, C, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, C, generator=g)
    if kind == "x1e4":
        z = z * 1e4
    elif kind == "ties":
        z = (z * 2).round()  # a few integer levels: exact ties in most rows, also at the maximum
        z[0, :] = 3.0  # a whole row tied: index 0
        if C > 2:
            z[B // 2, C - 1] = z[B // 2, 1] = 50.0  # the maximum twice: the lower index
    elif kind == "nan":
        z[B // 2, C // 2] = NAN
        z[B // 2, C - 1] = NAN  # two NaNs: the first one
        if B > 2:
            z[B - 1, 0] = float("inf")
    return z


def labels_of(B, C, seed, skip):
    """int64 [B] in [0, C), with -100, -1 and C mixed in (`skip` = "some") or nothing else (`skip` = "all")."""
    g = torch.Generator().manual_seed(seed + 1)
    y = torch.randint(0, C, (B,), generator=g)
    if skip == "all":
        return torch.tensor([-100, -1, C], dtype=torch.int64)[torch.arange(B) % 3]
    for k, bad in enumerate((-100, -1, C)):
        if B > 2 * k + 1:
            y[2 * k + 1] = bad
    return y


_C = {}


def softmax_c():
    """c of the softmax bound, measured once: float32 torch on the CPU against the float64 restatement, on the
    input kinds and row lengths the tests use."""
    if "c" not in _C:
        pairs = []
        for kind in ("randn", "x1e4", "ties"):
            for C in (2, 7, 33, 1000):
                z = logits_of(kind, 65, C, 100 + C)
                ref, scale = R.softmax_ref(z.numpy())
                pairs.append((torch.softmax(z, 1), ref, scale, TINY))
        _C["c"] = measure_c("cls_stats softmax", "fp32", pairs)
    return _C["c"]


def call(z, B, C, pad, labels, zero_state=True, want=("preds", "conf", "probs", "confusion", "counters"), state=None):
    """One fer_cls_stats call on views with guards; returns (rc, outputs, parents)."""
    zv, zp = nanview(B, C, pad, torch.float32, src=z, align=4)
    y = labels.to(DEV)
    o, p = {}, {}
    o["preds"], p["preds"] = intview(B)
    o["conf"], p["conf"] = nanvec(B)
    o["probs"], p["probs"] = nanview(B, C, pad + 1, torch.float32, align=4)
    if state is None:
        o["confusion"], p["confusion"] = intview(C * C, zero=zero_state)
        o["counters"], p["counters"] = intview(2, zero=zero_state)
    else:
        (o["confusion"], p["confusion"]), (o["counters"], p["counters"]) = state
    a = {k: (ptr(o[k]) if k in want else None) for k in o}
    rc = lib().fer_cls_stats(ptr(zv), zv.stride(0), ptr(y), B, C, a["preds"], a["conf"], a["probs"], o["probs"].stride(0),
                             a["confusion"], a["counters"], ops().stream())
    torch.cuda.synchronize()
    assert_bits_equal("logits", zp, zp)  # still readable
    return rc, o, p


def check_outputs(name, z, labels, B, C, o, p, times=1, base=None):
    ref = R.cls_stats_ref(z.numpy(), labels.numpy())
    assert o["preds"].cpu().tolist() == ref["preds"].tolist(), f"{name}: preds"
    cm = ref["confusion"] * times + (0 if base is None else base)
    assert np.array_equal(o["confusion"].cpu().numpy().reshape(C, C), cm), f"{name}: confusion"
    assert o["counters"].cpu().tolist() == (ref["counters"] * times).tolist(), f"{name}: counters"
    c = softmax_c()
    for k, r, s in (("probs", ref["probs"], ref["scale"]), ("conf", ref["conf"], ref["conf_scale"])):
        got = o[k].cpu().double().numpy()
        nan = np.isnan(r)
        assert np.array_equal(np.isnan(got), nan), f"{name}: {k} NaN pattern"
        assert_close(f"{name} {k}", torch.from_numpy(np.where(nan, 0, got)), torch.from_numpy(np.where(nan, 0, r)),
                     torch.from_numpy(np.where(nan, 0, s)), c, 0.0, extra=TINY)
    # conf is probs[pred], the same bits (rows without a NaN: a NaN's payload is not part of the contract)
    live = torch.from_numpy(~np.isnan(ref["conf"])).to(DEV)
    assert_bits_equal(f"{name} conf = probs[pred]", o["conf"][live].contiguous(),
                      o["probs"][torch.arange(B, device=DEV), o["preds"]][live].contiguous())
    int_untouched(f"{name} preds", p["preds"], B)
    int_untouched(f"{name} confusion", p["confusion"], C * C)
    int_untouched(f"{name} counters", p["counters"], 2)
    untouched_vec(f"{name} conf", p["conf"], B)
    untouched(f"{name} probs", p["probs"], B, C)


SHAPES = [(B, C) for B in (1, 2, 63, 64, 65, 257) for C in (1, 2, 7, 33, 1000)] + [(5, 64), (5, 65), (9, 129)]


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("B,C", SHAPES)
def test_cls_stats_every_shape_and_input_kind(B, C, pad):
    for n, kind in enumerate(KINDS):
        z = logits_of(kind, B, C, 7 * B + C + n)
        y = labels_of(B, C, B + C + n, "some")
        name = f"B={B} C={C} pad={pad} {kind}"
        rc, o, p = call(z, B, C, pad, y)
        assert rc == 0, last_error()
        check_outputs(name, z, y, B, C, o, p)
        # a second call accumulates the counts and rewrites the same per-row outputs
        first = {k: v.clone() for k, v in o.items()}
        rc, o2, p2 = call(z, B, C, pad, y, state=((o["confusion"], p["confusion"]), (o["counters"], p["counters"])))
        assert rc == 0, last_error()
        check_outputs(name + " twice", z, y, B, C, o2, p2, times=2)
        # a repeat from zero: bit-identical
        rc, o3, p3 = call(z, B, C, pad, y)
        for k in ("conf", "probs"):
            assert_bits_equal(f"{name} repeat {k}", o3[k].contiguous(), first[k].contiguous())
        for k in ("preds", "confusion", "counters"):
            assert torch.equal(o3[k], first[k]), f"{name} repeat {k}"


@pytest.mark.parametrize("B,C", [(1, 1), (2, 7), (65, 33), (257, 1000)])
def test_cls_stats_every_label_skipped(B, C):
    z = logits_of("randn", B, C, 5)
    y = labels_of(B, C, 5, "all")
    rc, o, p = call(z, B, C, 3, y)
    assert rc == 0, last_error()
    check_outputs(f"B={B} C={C} all skipped", z, y, B, C, o, p)
    assert o["counters"].cpu().tolist() == [0, B] and int(o["confusion"].abs().sum()) == 0


def test_cls_stats_counts_near_2_40_survive():
    B, C = 257, 7
    z, y = logits_of("randn", B, C, 9), labels_of(B, C, 9, "some")
    base = (2 ** 40 - 3) + torch.arange(C * C, dtype=torch.int64)
    cm, cmp_ = intview(C * C)
    cm.copy_(base)
    cnt, cntp = intview(2)
    cnt.copy_(torch.tensor([2 ** 40 - 1, 2 ** 40 + 5]))
    rc, o, p = call(z, B, C, 0, y, state=((cm, cmp_), (cnt, cntp)))
    assert rc == 0, last_error()
    ref = R.cls_stats_ref(z.numpy(), y.numpy())
    assert np.array_equal(o["confusion"].cpu().numpy(), base.numpy() + ref["confusion"].reshape(-1))
    assert o["counters"].cpu().tolist() == [2 ** 40 - 1 + int(ref["counters"][0]), 2 ** 40 + 5 + int(ref["counters"][1])]
    int_untouched("confusion", p["confusion"], C * C)


def test_cls_stats_each_output_is_optional():
    B, C = 65, 33
    z, y = logits_of("ties", B, C, 4), labels_of(B, C, 4, "some")
    rc, full, _ = call(z, B, C, 3, y)
    assert rc == 0
    for only in ("preds", "conf", "probs", "confusion", "counters"):
        rc, o, p = call(z, B, C, 3, y, want=(only,))
        assert rc == 0, last_error()
        if only in ("conf", "probs"):
            assert_bits_equal(only, o[only].contiguous(), full[only].contiguous())
        else:
            assert torch.equal(o[only], full[only]), only
        for k in set(o) - {only}:
            if k in ("conf", "probs"):
                all_nan(k, p[k])
            else:
                q = p[k].clone()
                if k in ("confusion", "counters"):  # the zeroed view inside the SENT parent
                    assert int(o[k].abs().sum()) == 0, k
                else:
                    assert (q == SENT).all(), k


def test_cls_stats_rejections_leave_the_outputs_untouched():
    B, C = 5, 7
    z, y = logits_of("randn", B, C, 1), labels_of(B, C, 1, "some").to(DEV)
    zv, _ = nanview(B, C, 3, torch.float32, src=z, align=4)
    L, st = lib(), ops().stream()

    def outs():
        return intview(B), nanvec(B), nanview(B, C, 1, torch.float32, align=4), intview(C * C), intview(2)

    def untouched_all(o):
        (pr, prp), (cf, cfp), (pb, pbp), (cm, cmp_), (ct, ctp) = o
        torch.cuda.synchronize()
        all_nan("conf", cfp)
        all_nan("probs", pbp)
        for q in (prp, cmp_, ctp):
            assert (q == SENT).all()

    cases = {
        "C must be >= 1": lambda o: L.fer_cls_stats(ptr(zv), zv.stride(0), ptr(y), B, 0, ptr(o[0][0]), ptr(o[1][0]),
                                                    ptr(o[2][0]), o[2][0].stride(0), ptr(o[3][0]), ptr(o[4][0]), st),
        "row stride must be >= C": lambda o: L.fer_cls_stats(ptr(zv), C - 1, ptr(y), B, C, ptr(o[0][0]), ptr(o[1][0]),
                                                             ptr(o[2][0]), o[2][0].stride(0), ptr(o[3][0]), ptr(o[4][0]), st),
        "probabilities' row stride": lambda o: L.fer_cls_stats(ptr(zv), zv.stride(0), ptr(y), B, C, ptr(o[0][0]),
                                                               ptr(o[1][0]), ptr(o[2][0]), C - 1, ptr(o[3][0]),
                                                               ptr(o[4][0]), st),
        "logits and labels are required": lambda o: L.fer_cls_stats(None, zv.stride(0), ptr(y), B, C, ptr(o[0][0]),
                                                                    ptr(o[1][0]), ptr(o[2][0]), o[2][0].stride(0),
                                                                    ptr(o[3][0]), ptr(o[4][0]), st),
        "labels are required": lambda o: L.fer_cls_stats(ptr(zv), zv.stride(0), None, B, C, ptr(o[0][0]), ptr(o[1][0]),
                                                         ptr(o[2][0]), o[2][0].stride(0), ptr(o[3][0]), ptr(o[4][0]), st),
    }
    for msg, f in cases.items():
        L.fer_set_persistent_mode(0)  # a success does not clear the message
        o = outs()
        assert f(o) != 0, msg
        assert last_error().startswith("cls_stats:") and msg in last_error(), (msg, last_error())
        untouched_all(o)
    out = torch.full((4 + 4 * C + 8,), NAN, dtype=torch.float64, device=DEV)
    cm = torch.zeros(C, C, dtype=torch.int64, device=DEV)
    for args, msg in (((ptr(cm), 0, ptr(out[4:])), "C must be >= 1"), ((None, C, ptr(out[4:])), "are required"),
                      ((ptr(cm), C, None), "are required")):
        assert L.fer_cls_report(*args, st) != 0
        assert last_error().startswith("cls_report:") and msg in last_error(), last_error()
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


def report_matrices():
    g = np.random.default_rng(3)
    m = {}
    for C in (1, 2, 7, 33, 1000):
        m[f"random C={C}"] = g.integers(0, 50, (C, C))
        m[f"empty C={C}"] = np.zeros((C, C), np.int64)
    a = g.integers(0, 50, (7, 7))
    a[4, :] = 0
    a[:, 4] = 0
    m["class absent from labels and predictions"] = a
    b = g.integers(1, 50, (7, 7))
    b[:, 2] = 0
    m["class never predicted"] = b
    c = g.integers(1, 50, (7, 7))
    c[5, :] = 0
    m["class never a label"] = c
    m["issue example"] = np.array([[1, 1, 0, 0], [0, 1, 0, 0], [0, 0, 0, 0], [0, 1, 0, 0]])
    d = np.zeros((300, 300), np.int64)
    d[257, 3] = 5  # one class beyond the first 256 threads' first pass
    d[3, 3] = 2
    m["sparse C=300"] = d
    m["large counts"] = g.integers(2 ** 39, 2 ** 40, (7, 7))
    return m


@pytest.mark.parametrize("name", list(report_matrices()))
def test_cls_report_against_the_restatement(name):
    cm = np.asarray(report_matrices()[name], np.int64)
    C = cm.shape[0]
    ref = R.report_ref(cm)
    dcm, dcmp = intview(C * C)
    dcm.copy_(torch.from_numpy(cm.reshape(-1)))
    parent = torch.full((4 + 4 * C + 8,), NAN, dtype=torch.float64, device=DEV)
    out = parent[4:4 + 4 + 4 * C]
    outs = []
    for _ in range(2):
        assert lib().fer_cls_report(ptr(dcm), C, ptr(out), ops().stream()) == 0, last_error()
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy().copy())
    got = outs[0]
    assert np.array_equal(outs[0], outs[1]), "repeat differs"
    assert not np.isnan(got).any()
    err, bound = np.abs(got - ref), (C + 8) * 2.0 ** -52 * np.abs(ref)
    assert (err <= bound).all(), (name, int((err > bound).sum()), float((err / np.maximum(bound, 1e-300)).max()))
    if cm.sum() == 0:
        assert (got == 0).all()
    assert torch.isnan(parent[:4]).all() and torch.isnan(parent[8 + 4 * C:]).all(), "out's guards were written"
    int_untouched("confusion", dcmp, C * C)
    assert np.array_equal(dcm.cpu().numpy().reshape(C, C), cm)


def test_meter_update_compute_and_reset():
    from fervit.metrics import ClassificationMeter

    B, C = 65, 7
    meter = ClassificationMeter(C, DEV)
    tot = np.zeros((C, C), np.int64)
    skipped = 0
    for n in range(3):
        z, y = logits_of("randn", B, C, 20 + n), labels_of(B, C, 20 + n, "some")
        preds, conf, probs = meter.update(z.to(DEV), y.to(DEV), want_probs=True)
        ref = R.cls_stats_ref(z.numpy(), y.numpy())
        assert preds.cpu().tolist() == ref["preds"].tolist() and probs.shape == (B, C) and conf.shape == (B,)
        tot += ref["confusion"]
        skipped += int(ref["counters"][1])
    assert len(meter.update(z.to(DEV), y.to(DEV))) == 2
    tot += ref["confusion"]
    skipped += int(ref["counters"][1])
    r = meter.compute()
    want = R.report_ref(tot)
    assert np.array_equal(r["confusion"], tot) and r["skipped"] == skipped and r["n"] == int(tot.sum())
    got = np.array([r["accuracy"], r["f1_macro"], r["f1_weighted"]])
    assert (np.abs(got - want[:3]) <= (C + 8) * 2.0 ** -52 * np.abs(want[:3])).all()
    per = want[4:].reshape(C, 4)
    for k, col in (("precision", 0), ("recall", 1), ("f1", 2), ("support", 3)):
        assert np.abs(np.array(r["per_class"][k]) - per[:, col]).max() <= (C + 8) * 2.0 ** -52
    meter.reset()
    z0 = meter.compute()
    assert z0["n"] == 0 and z0["skipped"] == 0 and z0["accuracy"] == 0 and z0["f1_macro"] == 0


def test_meter_update_under_graph_capture_replayed_three_times():
    """One stream, no parallel branches: the captured update replayed three times adds three times the batch."""
    from fervit.metrics import ClassificationMeter

    B, C = 64, 7
    z, y = logits_of("randn", B, C, 31), labels_of(B, C, 31, "some")
    zd, yd = z.to(DEV), y.to(DEV)
    meter = ClassificationMeter(C, DEV)
    meter.update(zd, yd)  # warm-up outside the capture (code object load)
    meter.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        preds, conf = meter.update(zd, yd)
    torch.cuda.synchronize()
    assert int(meter.counters.sum()) == 0  # capturing ran nothing
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    ref = R.cls_stats_ref(z.numpy(), y.numpy())
    r = meter.compute()
    assert np.array_equal(r["confusion"], 3 * ref["confusion"])
    assert r["n"] == 3 * int(ref["counters"][0]) and r["skipped"] == 3 * int(ref["counters"][1])
    assert preds.cpu().tolist() == ref["preds"].tolist()
