"""Highway forward / backward kernels (csrc/grouped.hip) element-wise against float64 on the CPU
(tests/afs_ref.py), with the bound of DESIGN.md section 2.1 (tests/elemwise.py). c is measured per case from
float32 torch on the CPU. The scales are first-order error propagation of the formulas: an element's
scale is the sum of the absolute terms behind it, with the error of the normalised value
xh = (pn - mean) rstd taken as rstd (|pn| + |mean|) (the subtraction cancels on a large mean).

Operands are views into NaN-filled parents with guard rows and padded strides; launches are repeated
and must give the same bits."""
import numpy as np
import pytest
import torch

import afs_ref as R
from abi_harness import NAN, out_round, parent, untouched_parent
from elemwise import assert_bits_equal, assert_close, measure_c

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = {"bf16": torch.bfloat16, "fp32": torch.float32}
EPS = 1e-5
KINDS = ["randn", "const_col", "plus100", "gate30", "neg_n"]


def vecs(G, n, data=None, dtype=torch.float32):
    p = torch.zeros((G, n + 8), dtype=dtype, device=DEV)
    v = p[:, :n]
    if data is not None:
        v.copy_(data)
    return v


def make(kind, dtype, G, Bn, C, seed=0):
    g = np.random.default_rng(seed + 31 * G + 7 * Bn + C)
    dt = DT[dtype]

    def r(*s):
        return torch.from_numpy(g.standard_normal(s))

    pn, pl, pg, dy = r(G, Bn, C), r(G, Bn, C), r(G, Bn, C), r(G, Bn, C)
    gamma, beta = 1 + 0.1 * r(G, C), 0.1 * r(G, C)
    if kind == "const_col":      # variance 0, rstd = eps^-1/2
        pn[:, :, 0] = 1.5
        pn[:, :, C - 1] = -0.25
    elif kind == "plus100":      # large mean, small spread
        pn = pn + 100.0
    elif kind == "gate30":       # the sigmoid saturates, dg underflows
        pg = torch.where(r(G, Bn, C) > 0, torch.full_like(pg, 30.0), torch.full_like(pg, -30.0))
    elif kind == "neg_n":        # the activation's negative branch on every element
        gamma, beta = 0.1 * r(G, C).abs() + 0.05, -5.0 - r(G, C).abs()
    rd = lambda t: t.to(dt).double()
    return dict(pn=rd(pn), pl=rd(pl), pg=rd(pg), dy=rd(dy), gamma=gamma.float().double(), beta=beta.float().double(),
                rm=(0.1 * r(G, C)).float().double(), rv=(0.5 + r(G, C).abs()).float().double())


def reference(d, train, act, momentum, f):
    """All outputs in precision f (torch.float64 reference or torch.float32 for c)."""
    t = {k: v.to(f) for k, v in d.items()}
    y, mean, rstd, rm, rv = R.highway(t["pn"], t["pl"], t["pg"], t["gamma"], t["beta"], t["rm"], t["rv"], train,
                                      momentum, EPS, act)
    dpn, dpl, dpg, dgam, dbet = R.highway_bwd(t["dy"], t["pn"], t["pl"], t["pg"], mean, rstd, t["gamma"], t["beta"],
                                              train, act)
    return dict(y=y, mean=mean, rstd=rstd, rm=rm, rv=rv, dpn=dpn, dpl=dpl, dpg=dpg, dgamma=dgam, dbeta=dbet)


def scales(d, ref, train, act, momentum):
    pn, pl, pg, dy, gam, bet = d["pn"], d["pl"], d["pg"], d["dy"], d["gamma"], d["beta"]
    Bn = pn.shape[1]
    mean, rstd = ref["mean"][:, None], ref["rstd"][:, None]
    s, sc = torch.sigmoid(pg), torch.sigmoid(-pg)
    s_mean = pn.abs().mean(1)
    s_var = ((pn.abs() + mean.abs()) ** 2).mean(1)
    s_rstd = ref["rstd"] + 0.5 * ref["rstd"] ** 3 * s_var
    if not train:  # the statistics are inputs
        s_mean, s_var, s_rstd = d["rm"].abs(), d["rv"].abs(), ref["rstd"]
    xh = (pn - mean) * rstd
    s_xh = rstd * (pn.abs() + mean.abs()) + (pn - mean).abs() * s_rstd[:, None]
    s_v = gam.abs()[:, None] * s_xh + bet.abs()[:, None]
    v = xh * gam[:, None] + bet[:, None]
    dv = dy * s * R.act_grad(v, act)
    k = (gam.abs() * ref["rstd"])[:, None]
    mg = (dv * xh).sum(1, keepdim=True) / Bn if train else torch.zeros_like(mean)
    s_dg = (dv.abs() * s_xh).sum(1)
    s_db = dv.abs().sum(1)
    s_dpn = k * (dv.abs() + (s_db[:, None] + xh.abs() * s_dg[:, None] + s_xh * (mg * Bn).abs()) / Bn * float(train))
    s_dpn = s_dpn + (gam.abs() * s_rstd)[:, None] * (dv.abs() + float(train) * (s_db[:, None] / Bn + xh.abs() * mg.abs()))
    return dict(y=s * s_v + sc * pl.abs(), mean=s_mean, rstd=s_rstd,
                rm=d["rm"].abs() + momentum * s_mean, rv=d["rv"].abs() + momentum * s_var * Bn / max(Bn - 1, 1),
                dpn=s_dpn, dpl=(dy * sc).abs(), dpg=dy.abs() * s * sc * (s_v + pl.abs()), dgamma=s_dg, dbeta=s_db)


def run_native(d, dtype, train, act, momentum):
    from fervit import ops

    dt = DT[dtype]
    G, Bn, C = d["pn"].shape
    (_, pn), (_, pl), (_, pg), (_, dy) = (parent(G, Bn, C, dt, d[k]) for k in ("pn", "pl", "pg", "dy"))
    gamma, beta, rm, rv = vecs(G, C, d["gamma"]), vecs(G, C, d["beta"]), vecs(G, C, d["rm"]), vecs(G, C, d["rv"])
    nbt = vecs(G, 1, torch.full((G, 1), 5), dtype=torch.int64)[:, 0]
    py, y = parent(G, Bn, C, dt)
    _, mean, rstd = ops.highway_fwd(pn, pl, pg, gamma, beta, rm, rv, nbt, train, momentum, EPS, act, out=y)
    dgam, dbet = vecs(G, C), vecs(G, C)
    dgam.fill_(NAN)
    dbet.fill_(NAN)
    dpn, dpl, dpg = ops.highway_bwd(dy, pn, pl, pg, mean, rstd, gamma, beta, train, act, dgamma=dgam, dbeta=dbet)
    untouched_parent("highway_fwd y", py, C)
    return dict(y=y, mean=mean, rstd=rstd, rm=rm, rv=rv, dpn=dpn, dpl=dpl, dpg=dpg, dgamma=dgam, dbeta=dbet, nbt=nbt)


def check(name, d, dtype, train, act, momentum=0.1):
    dt = DT[dtype]
    ref = reference(d, train, act, momentum, torch.float64)
    f32 = reference(d, train, act, momentum, torch.float32)
    sc = scales(d, ref, train, act, momentum)
    got = run_native(d, dtype, train, act, momentum)
    again = run_native(d, dtype, train, act, momentum)
    for k in ("y", "mean", "rstd", "rm", "rv", "dpn", "dpl", "dpg", "dgamma", "dbeta"):
        c = measure_c(f"highway {name} {k}", dtype, [(f32[k], ref[k], sc[k])])
        assert_close(f"{name} {k}", got[k], ref[k], sc[k], c, out_round(dt) if k in ("y", "dpn", "dpl", "dpg") else 0.0)
        assert_bits_equal(f"{name} {k}", got[k], again[k])
    assert got["nbt"].tolist() == [5 + int(train)] * d["pn"].shape[0]


@pytest.mark.parametrize("C", [8, 256, 72])  # 72: not a multiple of the 64-channel tile
@pytest.mark.parametrize("Bn", [2, 3, 8, 65])
@pytest.mark.parametrize("G", [1, 3, 18])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_shape_grid(dtype, G, Bn, C):
    for act, train in (("lrelu", True), ("relu", False), ("relu", True), ("lrelu", False)):
        check(f"{dtype} G{G} B{Bn} C{C} {act} train{train}", make("randn", dtype, G, Bn, C), dtype, train, act)


@pytest.mark.parametrize("kind", KINDS[1:])
@pytest.mark.parametrize("act", ["lrelu", "relu"])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_hard_inputs(dtype, act, kind):
    for train in (True, False):
        for G, Bn, C in ((3, 8, 72), (1, 65, 8)):
            check(f"{kind} {dtype} {act} train{train} G{G} B{Bn} C{C}", make(kind, dtype, G, Bn, C), dtype, train, act)


def test_constant_column_has_rstd_eps_to_the_minus_half():
    d = make("const_col", "fp32", 3, 8, 72)
    got = run_native(d, "fp32", True, "lrelu", 0.1)
    want = np.float32(1.0) / np.sqrt(np.float32(EPS))
    for c in (0, 71):
        assert np.allclose(got["rstd"][:, c].cpu().numpy(), want, rtol=1e-6, atol=0)
        assert np.array_equal(got["mean"][:, c].cpu().numpy(), d["pn"][:, 0, c].float().numpy())


@pytest.mark.parametrize("momentum", [0.1, 0.37])
def test_running_statistics_over_repeated_calls(momentum):
    """Three train calls on different batches against the float64 recurrence; num_batches_tracked counts
    them; an eval call moves nothing."""
    from fervit import ops

    G, Bn, C = 3, 8, 72
    ds = [make("randn", "fp32", G, Bn, C, seed=s) for s in range(3)]
    rm, rv = vecs(G, C, ds[0]["rm"]), vecs(G, C, ds[0]["rv"])
    nbt = vecs(G, 1, dtype=torch.int64)[:, 0]
    rm64, rv64 = ds[0]["rm"].clone(), ds[0]["rv"].clone()
    rm32, rv32 = rm64.float(), rv64.float()  # the same recurrence in float32 torch, for c
    s_rm, s_rv = rm64.abs(), rv64.abs()
    for d in ds:
        args = [d[k].float().to(DEV) for k in ("pn", "pl", "pg")]
        ops.highway_fwd(*args, vecs(G, C, d["gamma"]), vecs(G, C, d["beta"]), rm, rv, nbt, True, momentum, EPS, "lrelu")
        mean = d["pn"].mean(1)
        var = ((d["pn"] - mean[:, None]) ** 2).sum(1) / (Bn - 1)
        rm64 = (1 - momentum) * rm64 + momentum * mean
        rv64 = (1 - momentum) * rv64 + momentum * var
        p32 = d["pn"].float()
        rm32 = (1 - momentum) * rm32 + momentum * p32.mean(1)
        rv32 = (1 - momentum) * rv32 + momentum * p32.var(1, unbiased=True)
        s_rm = s_rm + momentum * d["pn"].abs().mean(1)
        s_rv = s_rv + momentum * ((d["pn"].abs() + mean.abs()[:, None]) ** 2).sum(1) / (Bn - 1)
    assert_close("running_mean", rm, rm64, s_rm, measure_c("running_mean x3", "fp32", [(rm32, rm64, s_rm)]), 0.0)
    assert_close("running_var", rv, rv64, s_rv, measure_c("running_var x3", "fp32", [(rv32, rv64, s_rv)]), 0.0)
    assert nbt.tolist() == [3] * G
    before = (rm.clone(), rv.clone())
    ops.highway_fwd(*args, vecs(G, C, d["gamma"]), vecs(G, C, d["beta"]), rm, rv, nbt, False, momentum, EPS, "lrelu")
    assert torch.equal(rm, before[0]) and torch.equal(rv, before[1]) and nbt.tolist() == [3] * G


def test_training_with_one_row_raises_as_batchnorm_does():
    from fervit import ops

    z = torch.zeros(1, 1, 8, device=DEV)
    v = torch.ones(1, 8, device=DEV)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        ops.highway_fwd(z, z, z, v, v, v.clone(), v.clone(), None, True)


def test_backward_accumulate_and_skip_mask_element_wise():
    """dgamma / dbeta added onto previous values (which join the reference and the scale); a skipped group's
    parameter gradients stay untouched while its dpn / dpl / dpg are still produced."""
    from fervit import ops

    G, Bn, C = 3, 8, 72
    d = make("randn", "fp32", G, Bn, C)
    ref = reference(d, True, "lrelu", 0.1, torch.float64)
    f32 = reference(d, True, "lrelu", 0.1, torch.float32)
    sc = scales(d, ref, True, "lrelu", 0.1)
    prev = torch.from_numpy(np.random.default_rng(3).standard_normal((2, G, C))).float()
    args = [parent(G, Bn, C, torch.float32, d[k])[1] for k in ("dy", "pn", "pl", "pg")]
    mean, rstd = ref["mean"].float().to(DEV), ref["rstd"].float().to(DEV)
    gamma, beta = vecs(G, C, d["gamma"]), vecs(G, C, d["beta"])
    dgam, dbet = vecs(G, C, prev[0]), vecs(G, C, prev[1])
    dps = ops.highway_bwd(*args, mean, rstd, gamma, beta, True, "lrelu", dgamma=dgam, dbeta=dbet, accumulate=True,
                          skip_mask=0b010)
    for k, got, p in (("dgamma", dgam, prev[0]), ("dbeta", dbet, prev[1])):
        c = measure_c(f"highway accumulate {k}", "fp32", [(f32[k] + p, ref[k] + p.double(), sc[k] + p.abs().double())])
        for g in (0, 2):
            assert_close(f"accumulate {k} group {g}", got[g], ref[k][g] + p[g].double(), sc[k][g] + p[g].abs().double(),
                         c, 0.0)
        assert torch.equal(got[1].cpu(), p[1]), f"{k}: the skipped group was written"
    for k, got in zip(("dpn", "dpl", "dpg"), dps):
        assert_close(f"skip {k}", got, ref[k], sc[k], measure_c(f"highway skip {k}", "fp32", [(f32[k], ref[k], sc[k])]), 0.0)


def test_rejections_return_an_error_with_a_message():
    from fervit._lib import SIGNATURES, FerError, lib
    from fervit import ops

    L = lib()
    z = torch.zeros(1, 2, 8, device=DEV)
    v = torch.ones(1, 8, device=DEV)
    with pytest.raises(KeyError):
        ops.highway_fwd(z, z, z, v, v, v.clone(), v.clone(), None, True, act="gelu")
    with pytest.raises(FerError, match="eval needs the running statistics"):
        ops.highway_fwd(z, z, z, v, v, None, None, None, False)

    def raw(name, **over):
        args = [None if t is ctypes.c_void_p else (0.0 if t is ctypes.c_float else 0) for t in SIGNATURES[name][1]]
        for pos, val in over.items():
            args[int(pos[1:])] = val
        rc = getattr(L, name)(*args)
        return rc, L.fer_last_error().decode()

    import ctypes

    p = z.data_ptr()
    # fer_highway_fwd: G, B, C at 23, 24, 25; act at 17; mean / rstd at 21 / 22; gamma / beta at 6 / 7
    base = dict(a1=p, a2=p, a3=p, a4=8, a6=v.data_ptr(), a7=v.data_ptr(), a9=v.data_ptr(), a10=v.data_ptr(), a18=p,
                a19=8, a23=1, a24=2, a25=8)
    rc, msg = raw("fer_highway_fwd", **dict(base, a17=5))
    assert rc != 0 and "unknown activation" in msg
    rc, msg = raw("fer_highway_fwd", **dict(base, a21=v.data_ptr()))
    assert rc != 0 and "mean and rstd go together" in msg
    rc, msg = raw("fer_highway_fwd", **dict(base, a14=1, a24=1))
    assert rc != 0 and "more than 1 row" in msg
    rc, msg = raw("fer_highway_fwd", **dict(base, a4=4))
    assert rc != 0 and "stride >= C" in msg
    # fer_highway_bwd: skip_mask at 24, G at 25
    rc, msg = raw("fer_highway_bwd", a24=1, a25=65, a26=2, a27=8)
    assert rc != 0 and "skip_mask covers at most 64 groups" in msg
    rc, msg = raw("fer_highway_bwd", a15=7, a25=1, a26=2, a27=8)
    assert rc != 0 and "unknown activation" in msg
