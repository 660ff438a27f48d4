"""The three mixup kernels (csrc/mixup.hip) through the C ABI, DESIGN.md section 2.14.

fer_mixup_draw: the permutation element-exact against the integer mirror (tests/mixup_ref.py), lam against the
float64 mirror within LAM_TOL, the Kolmogorov-Smirnov and cell-count gates of tests/test_mixup_ref_cpu.py on the
device's own draws, the host checks, and the device step counter (as tests/test_gpu_step_seed_kernels.py drives it).
fer_mixup_apply: per element against float64 with the bound 4 * 2^-24 * (|lam x| + |(1 - lam) x_p|) -- four fp32
roundings: 1 - lam, two products, one sum -- on both the 16-byte and the element path, operands inside NaN parents
whose guards must keep their bits. fer_cross_entropy_mix: loss and dlogits against float64 torch with the bound
form and constant of fer_cross_entropy's test (tests/test_gpu_rowops.py): c 2^-23 |loss| and c 2^-23 / B, c
measured from fp32 torch on the CPU."""
import functools

import numpy as np
import pytest
import torch

import mixup_ref as R
from abi_harness import NAN, last_error, nanflat, nanview, ops, untouched, untouched_flat
from abi_harness import lib as L
from elemwise import assert_bits_equal, assert_close, measure_c

pytestmark = pytest.mark.gpu

DEV = "cuda"
LAM_TOL = R.LAM_TOL
GUARD = -7


def draw(alpha, B, seed, n_sets=1):
    """fer_mixup_draw into guarded buffers; returns (lam [n_sets], perm [n_sets][B]) on the host."""
    lam_p = torch.full((n_sets + 8,), NAN, device=DEV)
    perm_p = torch.full((n_sets * B + 16,), GUARD, dtype=torch.int32, device=DEV)
    lam, perm = lam_p[4:4 + n_sets], perm_p[8:8 + n_sets * B]
    rc = L().fer_mixup_draw(float(alpha), B, ops().seed64(seed), n_sets, lam.data_ptr(), perm.data_ptr(), ops().stream())
    assert rc == 0, last_error()
    torch.cuda.synchronize()
    assert torch.isnan(lam_p[:4]).all() and torch.isnan(lam_p[4 + n_sets:]).all(), "lam guards"
    assert (perm_p[:8] == GUARD).all() and (perm_p[8 + n_sets * B:] == GUARD).all(), "perm guards"
    return lam.cpu().numpy().astype(np.float64), perm.cpu().numpy().reshape(n_sets, B)


@functools.lru_cache(maxsize=None)
def device_draws(alpha):
    """One n_sets = 4096 launch at B = 5 under the fixed seed of the gates."""
    return draw(alpha, 5, R.SEED, R.N_DRAWS)


@functools.lru_cache(maxsize=None)
def mirror_draws(alpha):
    return R.lam_draws(alpha)


# ---------------------------------------------------------------------- fer_mixup_draw
@pytest.mark.parametrize("n_sets", [1, 3])
@pytest.mark.parametrize("B", [1, 2, 5, 64, 257, 1024, 2048])
def test_draw_perm_is_the_mirrors(B, n_sets):
    seed = 0xA5A5_0000_1234_0000 + B
    _, perm = draw(1.0, B, seed, n_sets)
    for s in range(n_sets):
        want = R.perm(R.stream_seed(seed, s), B)
        assert (perm[s] == want).all(), (B, s, np.nonzero(perm[s] != want)[0][:5])
        assert sorted(perm[s].tolist()) == list(range(B))
    if n_sets > 1 and B > 2:
        assert (perm[0] != perm[1]).any()


def test_draw_host_checks():
    o = ops()
    lam, perm = torch.full((4,), NAN, device=DEV), torch.full((4096,), GUARD, dtype=torch.int32, device=DEV)
    for B, n_sets, lp, pp, msg in ((0, 1, lam.data_ptr(), perm.data_ptr(), "1 <= B <= 2048"),
                                   (2049, 1, lam.data_ptr(), perm.data_ptr(), "1 <= B <= 2048"),
                                   (8, 0, lam.data_ptr(), perm.data_ptr(), "n_sets >= 1"),
                                   (8, 1, None, perm.data_ptr(), "null output"),
                                   (8, 1, lam.data_ptr(), None, "null output")):
        rc = L().fer_mixup_draw(1.0, B, 5, n_sets, lp, pp, o.stream())
        assert rc != 0 and last_error() == "mixup_draw: " + msg, (B, n_sets, rc, last_error())
    torch.cuda.synchronize()
    assert torch.isnan(lam).all() and (perm == GUARD).all()
    with pytest.raises(ValueError):
        o.mixup_draw(1.0, 8, 5, lam, perm[:7])


@pytest.mark.parametrize("alpha", [0.5, 1.0, 2.0])
def test_draw_lam_is_beta_and_the_mirrors(alpha):
    lam, _ = device_draws(alpha)
    assert ((lam >= 0) & (lam <= 1)).all()
    D = R.ks_statistic(lam, R.CDF[alpha])
    print(f"KS device alpha={alpha}: D = {D:.4f} (limit {R.KS_LIMIT:.4f})")
    assert D < R.KS_LIMIT
    want, capped, margin = mirror_draws(alpha)
    keep = margin >= R.MARGIN
    assert not capped.any() and 1 - keep.mean() <= 0.01
    diff = np.abs(lam - want)
    print(f"lam-measure alpha={alpha}: worst |device - mirror| = {diff[keep].max():.3e} over {keep.sum()} draws "
          f"({(~keep).sum()} left out, worst among them {diff[~keep].max() if (~keep).any() else 0:.3e})")
    assert diff[keep].max() <= LAM_TOL


def test_draw_ks_gate_can_fail_on_device_draws():
    assert R.ks_statistic(device_draws(0.5)[0], R.CDF[1.0]) > R.KS_LIMIT


def test_draw_perm_cells_are_even_and_the_mirrors():
    _, perm = device_draws(1.0)
    R.cell_gate(perm)
    for s in (0, 1, 4095):
        assert (perm[s] == R.perm(R.stream_seed(R.SEED, s), 5)).all()


@pytest.mark.parametrize("alpha", [0.0, -1.0])
def test_draw_without_mixup_is_exactly_one(alpha):
    lam, perm = draw(alpha, 64, 99, 3)
    assert (lam == 1.0).all()
    assert all(sorted(p.tolist()) == list(range(64)) for p in perm)


def test_draw_follows_the_step_counter():
    """With a counter registered, launches with one seed at counters r and r + 1 differ and each is the mirror's
    draw at step_seed(seed, r); unregistered, the launch is the mirror's at the plain seed."""
    seed, B, r = 0x0123_4567_89AB_CDEF, 64, 41
    for c in (r, r + 1, None):
        assert R.lam(R.stream_seed(seed, 0, c), 1.0)[2] >= R.MARGIN  # none of the three sits on a boundary
    counter = torch.tensor([r], dtype=torch.int64, device=DEV)  # the ABI's uint64_t
    try:
        assert L().fer_set_step_counter(counter.data_ptr()) == 0
        got = {r: draw(1.0, B, seed)}
        counter.fill_(r + 1)
        got[r + 1] = draw(1.0, B, seed)
        held = int(counter.item())
        assert L().fer_set_step_counter(None) == 0
        got[None] = draw(1.0, B, seed)
    finally:
        assert L().fer_set_step_counter(None) == 0
        torch.cuda.synchronize()
    assert held == r + 1, "the draw does not advance the counter"
    for c, (lam, perm) in got.items():
        want_lam, want_perm = R.draw(seed, 1.0, B, counter=c)
        assert (perm[0] == want_perm).all(), c
        assert abs(lam[0] - want_lam) <= LAM_TOL, (c, lam[0], want_lam)
    assert (got[r][1] != got[r + 1][1]).any() and got[r][0] != got[r + 1][0]
    assert (got[r][1] != got[None][1]).any()


# ---------------------------------------------------------------------- fer_mixup_apply
def apply_case(B, Ln, lam, shift=0):
    g = torch.Generator().manual_seed(B * 131 + Ln)
    x0 = torch.randn(B, Ln, generator=g) * 3
    perm = torch.randperm(B, generator=g).to(torch.int32)
    if shift:  # contiguous rows whose first element is only 4-byte aligned
        xv, xp = nanflat(B * Ln, torch.float32, x0, shift=shift)
        ov, op = nanflat(B * Ln, torch.float32, shift=shift)
        assert xv.data_ptr() % 16 == 4 * shift and ov.data_ptr() % 16 == 4 * shift
    else:
        align = 16 if Ln % 4 == 0 else 4
        xv, xp = nanview(B, Ln, 0, torch.float32, x0, align=align)
        ov, op = nanview(B, Ln, 0, torch.float32, align=align)
    lam_d = torch.tensor([lam], dtype=torch.float32, device=DEV)
    pd = perm.to(DEV)
    x_before = xp.clone()
    rc = L().fer_mixup_apply(xv.data_ptr(), pd.data_ptr(), lam_d.data_ptr(), ov.data_ptr(), B, Ln, ops().stream())
    assert rc == 0, last_error()
    torch.cuda.synchronize()
    name = f"mixup_apply B={B} L={Ln} lam={lam} shift={shift}"
    assert_bits_equal(name + " input", xp, x_before)
    if shift:
        untouched_flat(name, op, B * Ln, shift=shift)
    else:
        untouched(name, op, B, Ln)
    x = x0.double()
    l = float(np.float32(lam))
    a, b = l * x, (1.0 - l) * x[perm.long()]
    # 4 * 2^-24 = 2 * 2^-23
    assert_close(name, ov.reshape(B, Ln), a + b, a.abs() + b.abs(), 2.0, 0.0)
    return ov.reshape(B, Ln).cpu(), x0, perm


@pytest.mark.parametrize("lam", [0.0, 1.0, 0.3])
@pytest.mark.parametrize("B,Ln", [(1, 7), (5, 7), (5, 9216), (64, 512 * 18), (3, 4 * 1 + 2)])
def test_apply(B, Ln, lam):
    out, x0, perm = apply_case(B, Ln, lam)
    if lam == 1.0:
        assert_bits_equal("lam = 1 keeps the batch", out, x0)
    if lam == 0.0:
        assert_bits_equal("lam = 0 is the gather", out, x0[perm.long()])


@pytest.mark.parametrize("lam", [0.0, 1.0, 0.3])
def test_apply_row_pointer_only_4_byte_aligned(lam):
    apply_case(5, 8, lam, shift=1)  # L % 4 == 0, but no 16-byte alignment: the element path


def test_apply_in_place_is_an_error():
    x = torch.ones(4, 8, device=DEV)
    perm = torch.arange(4, dtype=torch.int32, device=DEV)
    lam = torch.ones(1, device=DEV)
    for out in (x, x.reshape(-1)[8:]):
        rc = L().fer_mixup_apply(x.data_ptr(), perm.data_ptr(), lam.data_ptr(), out.data_ptr(), 4, 8, ops().stream())
        assert rc != 0 and last_error() == "mixup_apply: out must not overlap x"
    with pytest.raises(Exception, match="must not overlap"):
        ops().mixup_apply(x, perm, lam, out=x)
    torch.cuda.synchronize()
    assert (x == 1).all()


def test_apply_bad_perm_entry_takes_the_row_itself():
    x = torch.arange(12, dtype=torch.float32, device=DEV).reshape(3, 4)
    perm = torch.tensor([2, -1, 3], dtype=torch.int32, device=DEV)
    lam = torch.zeros(1, device=DEV)
    out = ops().mixup_apply(x, perm, lam)
    assert_bits_equal("rows", out.cpu(), x[[2, 1, 2]].cpu())


# ---------------------------------------------------------------------- fer_cross_entropy_mix
def ce_mix_torch(logits, y, y2, lam, w, ls, prec):
    F = torch.nn.functional
    lg = logits.clone().to(prec).requires_grad_(True)
    wt = None if w is None else w.to(prec)
    loss = lam * F.cross_entropy(lg, y, weight=wt, label_smoothing=ls) + \
        (1 - lam) * F.cross_entropy(lg, y2, weight=wt, label_smoothing=ls)
    loss.backward()
    return loss.detach(), lg.grad * 0.25


@pytest.mark.parametrize("C", [2, 7])
@pytest.mark.parametrize("B", [1, 5, 256, 300])
def test_cross_entropy_mix(B, C):
    o = ops()
    g = torch.Generator().manual_seed(B * 977 + C)
    logits = torch.randn(B, C, generator=g)
    logits[B // 2] = torch.randn(C, generator=g) * 1e4  # a row near 1e4: expf overflows without the max
    y = torch.randint(0, C, (B,), generator=g)
    w = torch.rand(C, generator=g) + 0.5
    perm = torch.roll(torch.arange(B), 1) if B > 1 else torch.zeros(1, dtype=torch.int64)
    if B > 2:
        y[1] = (y[0] + 1) % C  # y[perm] differs from y somewhere
    ld, yd, wd, pd = logits.to(DEV), y.to(DEV), w.to(DEV), perm.to(torch.int32).to(DEV)
    for lam in (0.3, 1.0, 0.0):
        lam32 = float(np.float32(lam))
        lam_d = torch.tensor([lam], dtype=torch.float32, device=DEV)
        for ls in (0.0, 0.1):
            for wt in (None, w):
                name = f"cross_entropy_mix B={B} C={C} lam={lam} ls={ls} weight={'on' if wt is not None else 'off'}"
                rl, rg = ce_mix_torch(logits, y, y[perm], lam32, wt, ls, torch.float64)
                fl, fg = ce_mix_torch(logits, y, y[perm], lam32, wt, ls, torch.float32)
                s_loss, s_grad = rl.abs().reshape(1), torch.full((B, C), 1.0 / B, dtype=torch.float64)
                c_l = measure_c("cross_entropy_mix.loss", "fp32", [(fl.reshape(1), rl.reshape(1), s_loss)])
                c_g = measure_c("cross_entropy_mix.grad", "fp32", [(fg, rg, s_grad)])
                wdev = None if wt is None else wd
                loss, dl = o.cross_entropy_mix(ld, yd, pd, lam_d, wdev, ls, grad_scale=0.25)
                assert_close(name + " loss", loss.reshape(1), rl.reshape(1), s_loss, c_l, 0.0)
                assert_close(name + " dlogits", dl, rg, s_grad, c_g, 0.0)
                loss2, none = o.cross_entropy_mix(ld, yd, pd, lam_d, wdev, ls, grad_scale=0.25, want_grad=False)
                assert none is None
                assert_bits_equal(name + " loss without dlogits", loss2.reshape(1).cpu(), loss.reshape(1).cpu())
                # lam = 1, and perm = None at any lam, are fer_cross_entropy
                plain_l, plain_g = o.cross_entropy(ld, yd, wdev, ls, grad_scale=0.25)
                pl64, pg64 = plain_l.double().cpu().reshape(1), plain_g.double().cpu()
                if lam == 1.0:
                    assert_close(name + " loss against fer_cross_entropy", loss.reshape(1), pl64, pl64.abs(), c_l, 0.0)
                    assert_close(name + " dlogits against fer_cross_entropy", dl, pg64, s_grad, c_g, 0.0)
                loss_id, dl_id = o.cross_entropy_mix(ld, yd, None, lam_d, wdev, ls, grad_scale=0.25)
                assert_close(name + " identity loss against fer_cross_entropy", loss_id.reshape(1), pl64, pl64.abs(),
                             c_l, 0.0)
                assert_close(name + " identity dlogits against fer_cross_entropy", dl_id, pg64, s_grad, c_g, 0.0)
                if lam == 0.3 and B > 2:  # the gate can fail: the second target taken from y instead of y[perm]
                    wl, wg = ce_mix_torch(logits, y, y, lam32, wt, ls, torch.float64)
                    with pytest.raises(AssertionError):
                        assert_close(name + " loss, wrong reference", loss.reshape(1), wl.reshape(1), wl.abs().reshape(1),
                                     c_l, 0.0)
                    with pytest.raises(AssertionError):
                        assert_close(name + " dlogits, wrong reference", dl, wg, s_grad, c_g, 0.0)


def test_cross_entropy_mix_empty_and_null():
    o = ops()
    assert L().fer_cross_entropy_mix(None, None, None, None, None, 0, 7, 0.0, 1.0, None, None, o.stream()) == 0
    z = torch.zeros(2, 7, device=DEV)
    y = torch.zeros(2, dtype=torch.int64, device=DEV)
    rc = L().fer_cross_entropy_mix(z.data_ptr(), y.data_ptr(), None, None, None, 2, 7, 0.0, 1.0, None, None, o.stream())
    assert rc != 0 and last_error() == "cross_entropy_mix: null operand"
