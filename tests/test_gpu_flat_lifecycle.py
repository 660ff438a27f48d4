"""Lifecycle of the flat parameter store between torch and the kernels: parameter edits after the
bf16 shadow exists, no-op moves under an optimizer, deep copies, a child module run before / beside
its owner.

One comparison throughout, with no tolerance: after each scenario a fresh twin of the same class loads
the scenario model's state_dict() before its own first forward; with the same runtime.manual_seed and
the same input, logits and every parameter gradient must be torch.equal, in bf16 and in fp32. Both
models run the same kernels on the same shapes and the library's reductions are bitwise reproducible,
so any difference is the store handing a kernel something other than the parameters' current values.
Every case first asserts that the change is visible (the twin's logits differ from the logits before
it), so a case cannot pass because its edit did nothing.

Every scenario starts from a model that ran one forward, one backward and one FusedAdamW step in bf16,
so the bf16 shadow and its transposed copies exist.
"""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

from detparams import det_directions

pytestmark = pytest.mark.gpu

SEED = 20240
PRECS = ["bf16", "fp32"]
B, L, LAT = 4, 18, 64


# ---------------------------------------------------------------------------- models, inputs
def make_flat(seed=0):
    from models_fer_vit.latent_vit import LatentViT

    torch.manual_seed(seed)
    return LatentViT(embed_dim=128, depth=2, heads=2, mlp_dim=256, dropout=0.0)


def make_nested(seed=0):
    """ExpressionAwareViT over the tiny HybridLatentViT with adapters: the child `vit` is a FerModule
    (whose blocks and adapters are FerModules too). Biases / norms / alphas are moved off their
    constant init so that scaling them is visible."""
    from models_fer_vit.expression_aware_vit import ExpressionAwareViT
    from models_fer_vit.hybrid_latent_vit import HybridLatentViT
    from models_fer_vit.latent_decomposer import LatentDecomposer

    torch.manual_seed(seed)
    vit = HybridLatentViT(latent_dim=LAT, seq_len=L, pretrained_model_name="vit_tiny_patch16_224", num_classes=7,
                          use_pretrained=False, adapter_dim=32)
    dirs = det_directions(7, L, LAT)
    m = ExpressionAwareViT(LatentDecomposer({i: dirs[i] for i in range(7)}, seq_len=L, latent_dim=LAT), vit)
    with torch.no_grad():
        g = torch.Generator().manual_seed(seed + 11)
        for n, p in m.named_parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
    return m


MODELS = {"flat": (make_flat, 512), "nested": (make_nested, LAT)}


def data(dim, seed=1):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(B, L, dim, device="cuda", generator=g), torch.randint(0, 7, (B,), device="cuda", generator=g)


def run(m, x, y):
    """One seeded forward + backward from `.grad = None`: (logits, {name: grad})."""
    from fervit import runtime

    runtime.manual_seed(SEED)
    m.zero_grad(set_to_none=True)
    logits = m(x)
    F.cross_entropy(logits.float(), y, label_smoothing=0.1).backward()
    return logits.detach().clone(), {n: p.grad.detach().clone() for n, p in m.named_parameters()
                                     if p.grad is not None}


def warm(m, x, y, lr=1e-3):
    """The state every scenario starts from: one bf16 forward, backward and FusedAdamW step."""
    from fervit.optim import FusedAdamW

    m.set_precision("bf16")
    opt = FusedAdamW(m.parameters(), lr=lr, weight_decay=0.05, model=m)
    run(m, x, y)
    opt.step()
    flat = m.fer_flat()
    assert flat.half is not None and flat.half_t is not None
    return opt


def twin_of(m, make, prec):
    t = make(seed=97)  # another init: everything must come from the state_dict
    t.load_state_dict(m.state_dict())
    return t.cuda().train(m.training).set_precision(prec)


def assert_same(got, want, what):
    (lg, gg), (lw, gw) = got, want
    assert torch.equal(lg, lw), f"{what}: logits differ, max |d| = {(lg.float() - lw.float()).abs().max().item():.3e}"
    assert gg.keys() == gw.keys() and len(gg) > 0, what
    bad = [n for n in gg if not torch.equal(gg[n], gw[n])]
    assert not bad, f"{what}: gradients differ for {bad[:5]} ({len(bad)} of {len(gg)})"


def assert_matches_twin(m, make, prec, x, y, before, what, sub=None):
    """m (or its child `sub`) against a fresh twin; `before`: logits from before the change."""
    t = twin_of(m, make, prec)
    pick = (lambda mod: getattr(mod, sub)) if sub else (lambda mod: mod)
    want = run(pick(t), x, y)
    if before is not None:
        assert want[0].shape == before.shape and not torch.equal(want[0], before), f"{what}: the change is not visible"
    got = run(pick(m), x, y)
    assert_same(got, want, what)
    return got[0]


def assert_shadow_is_current(m):
    """bf16 shadow = the parameters rounded to bf16, bit for bit; transposed copies = its transposes."""
    flat = m.fer_flat()
    n2d = 0
    for n, p in m.named_parameters():
        h = flat.half_view(p)
        assert torch.equal(h.view(torch.int16), p.detach().to(torch.bfloat16).view(torch.int16)), f"stale shadow: {n}"
        if p.dim() == 2:
            n2d += 1
            assert torch.equal(flat.half_t_view(p), h.t()), f"stale transposed shadow: {n}"
    assert n2d > 0


# ---------------------------------------------------------------------------- A. parameter edits
W, BIAS = "transformer.layers.0.linear1.weight", "transformer.layers.0.linear1.bias"


def _edited_state(m):
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    for n in (W, BIAS):
        sd[n] = sd[n] * 1.5
    return sd


def _no_grad_mul(m, ps):
    with torch.no_grad():
        for p in ps:
            p.mul_(1.5)


def _init_normal(m, ps):
    for p in ps:
        torch.nn.init.normal_(p)


def _sgd_step(m, ps):
    assert all(p.grad is not None and p.grad.abs().max().item() > 0 for p in ps)
    torch.optim.SGD(ps, lr=10.0).step()


def _data_mul(m, ps):
    for p in ps:
        p.data.mul_(1.5)
    m.fer_params_changed()  # an in-place write through .data leaves no trace the host can see


def _data_copy(m, ps):
    for p in ps:
        p.data.copy_(p.detach() * 1.5)
    m.fer_params_changed()


def _data_assign(m, ps):
    for p in ps:
        p.data = (p.detach() * 1.5).clone()


EDITS = {
    "no_grad_mul_": _no_grad_mul,
    "nn_init_normal_": _init_normal,
    "sgd_step": _sgd_step,
    "load_state_dict": lambda m, ps: m.load_state_dict(_edited_state(m)),
    "load_state_dict_assign": lambda m, ps: m.load_state_dict(_edited_state(m), assign=True),
    "data_mul_": _data_mul,
    "data_copy_": _data_copy,
    "data_assign": _data_assign,
}


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("kind", list(EDITS))
def test_edit_after_the_shadow_exists(kind, prec):
    m = make_flat().cuda()
    x, y = data(512)
    warm(m, x, y)
    m.set_precision(prec)
    before, _ = run(m, x, y)
    params = dict(m.named_parameters())
    old = {n: params[n].detach().clone() for n in (W, BIAS)}
    EDITS[kind](m, [params[W], params[BIAS]])
    params = dict(m.named_parameters())  # assign=True replaces the objects
    for n in (W, BIAS):
        moved = params[n].detach().to(torch.bfloat16) != old[n].to(torch.bfloat16)
        if kind in ("nn_init_normal_", "sgd_step"):
            assert moved.any(), n
        else:  # x1.5 moves the bf16 value of every non-zero element, so no stale element can hide
            assert moved[old[n] != 0].all() and (old[n] != 0).any(), n
    assert_matches_twin(m, make_flat, prec, x, y, before, f"{kind}/{prec}")
    if prec == "bf16":
        assert_shadow_is_current(m)


# ---------------------------------------------------------------------------- B. idempotent moves
MOVES = {"cuda": lambda m: m.cuda(), "to_cuda": lambda m: m.to("cuda"), "float": lambda m: m.float()}


def _optimizer(kind, m):
    from fervit.optim import FusedAdamW

    if kind == "torch_adamw":
        return torch.optim.AdamW(m.parameters(), lr=1e-2, weight_decay=0.05)
    return FusedAdamW(m.parameters(), lr=1e-2, weight_decay=0.05, model=m)


def _steps(m, o, x, y, n):
    for _ in range(n):
        run(m, x, y)
        o.step()


def _snapshot(m, o):
    st = o.state_dict()["state"]
    return ([p.detach().clone() for p in m.parameters()],
            [(st[i]["exp_avg"].detach().clone().cuda(), st[i]["exp_avg_sq"].detach().clone().cuda(),
              float(st[i]["step"])) for i in range(len(st))])


@functools.lru_cache(maxsize=None)
def _uninterrupted(torch_adamw):
    """(after two steps, after four steps) of the run nothing interrupts; computed once per optimizer."""
    m = make_flat().cuda().set_precision("bf16")
    x, y = data(512)
    o = _optimizer("torch_adamw" if torch_adamw else "fused", m)
    _steps(m, o, x, y, 2)
    two = _snapshot(m, o)
    _steps(m, o, x, y, 2)
    return two, _snapshot(m, o)


@pytest.mark.parametrize("opt_kind", ["fused", "torch_adamw", "fused_reloaded"])
@pytest.mark.parametrize("move", list(MOVES))
def test_noop_move_keeps_the_optimizer_state(move, opt_kind):
    two, four = _uninterrupted(opt_kind == "torch_adamw")
    # the guard: the moments carry weight -- two more steps move every parameter and both moments
    assert all(not torch.equal(a, b) for a, b in zip(two[0], four[0]))
    assert all(m2.abs().max() > 0 and not torch.equal(m2, m4) and s2 == 2.0 and s4 == 4.0
               for (m2, _, s2), (m4, _, s4) in zip(two[1], four[1]))

    m = make_flat().cuda().set_precision("bf16")
    x, y = data(512)
    o = _optimizer(opt_kind, m)
    _steps(m, o, x, y, 2)
    if opt_kind == "fused_reloaded":
        sd = o.state_dict()
        o = _optimizer(opt_kind, m)
        o.load_state_dict(sd)
    assert MOVES[move](m) is m
    _steps(m, o, x, y, 2)
    got_p, got_s = _snapshot(m, o)
    names = [n for n, _ in m.named_parameters()]
    bad = [n for n, a, b in zip(names, got_p, four[0]) if not torch.equal(a, b)]
    assert not bad, f"parameters differ from the uninterrupted run: {bad[:5]} ({len(bad)} of {len(names)})"
    for n, (ea, es, st), (ra, rs, rt) in zip(names, got_s, four[1]):
        assert st == rt == 4.0, (n, st)
        assert torch.equal(ea, ra), f"exp_avg differs: {n}"
        assert torch.equal(es, rs), f"exp_avg_sq differs: {n}"


# ---------------------------------------------------------------------------- C. copy.deepcopy
def _ranges(flat):
    return [(t.data_ptr(), t.data_ptr() + t.numel() * t.element_size())
            for t in (flat.data, flat.grad, flat.half, flat.half_t) if t is not None]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("which", list(MODELS))
def test_deepcopy_after_the_first_forward(which, prec):
    from fervit.optim import FusedAdamW

    make, dim = MODELS[which]
    m = make().cuda()
    x, y = data(dim)
    opt = warm(m, x, y, lr=1e-2)
    m.set_precision(prec)
    first, _ = run(m, x, y)
    opt.step()
    at_copy, _ = run(m, x, y)
    assert not torch.equal(at_copy, first)
    c = copy.deepcopy(m)
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(1.5)

    # the copy computes with its own weights: those of the moment it was taken
    got = assert_matches_twin(c, make, prec, x, y, first, f"copy of {which}/{prec}")
    assert torch.equal(got, at_copy), "the copy does not reproduce the original's logits from before the edit"

    # ... in storage of its own
    held = _ranges(m.fer_flat())
    for n, p in c.named_parameters():
        for t in (p, p.grad):
            if t is not None:
                assert not any(lo <= t.data_ptr() < hi for lo, hi in held), f"{n} lives in the original's buffers"
    assert c.fer_flat() is not m.fer_flat()

    # a training step on the copy leaves the original alone, bit for bit
    now_m = assert_matches_twin(m, make, prec, x, y, at_copy, f"original of {which}/{prec} after the edit")
    keep_p = [p.detach().clone() for p in m.parameters()]
    keep_g = [p.grad.detach().clone() for p in m.parameters()]
    oc = FusedAdamW(c.parameters(), lr=1e-2, weight_decay=0.05, model=c)
    run(c, x, y)
    oc.step()
    torch.cuda.synchronize()
    for (n, p), kp, kg in zip(m.named_parameters(), keep_p, keep_g):
        assert torch.equal(p.detach(), kp) and torch.equal(p.grad, kg), f"a step on the copy changed the original's {n}"

    # and each still is its own model (copied hooks must not flip the other's owner_active)
    assert_matches_twin(c, make, prec, x, y, at_copy, f"copy of {which}/{prec} after its step")
    again = run(m, x, y)[0]
    assert torch.equal(again, now_m)
    assert_matches_twin(m, make, prec, x, y, at_copy, f"original of {which}/{prec} at the end")


# ---------------------------------------------------------------------------- D. child first, child alone
CHILD_W, CHILD_B = "vit.transformer.0.mlp.fc1.weight", "vit.transformer.0.mlp.fc1.bias"


@pytest.mark.parametrize("prec", PRECS)
def test_child_run_before_and_beside_its_owner(prec):
    from fervit.optim import FusedAdamW

    m = make_nested().cuda().set_precision(prec)
    opt = FusedAdamW(m.parameters(), lr=1e-2, weight_decay=0.05, model=m)  # before any forward
    x, y = data(LAT)
    xc = data(LAT, seed=2)[0]

    # the child before the model ever ran (nothing came before it: no earlier logits to differ from), then the model
    child0 = assert_matches_twin(m, make_nested, prec, xc, y, None, "child first", sub="vit")
    assert torch.isfinite(child0.float()).all() and child0.float().abs().max().item() > 0
    assert m.vit._fer_flat is not None and m._fer_flat is None  # the child's own store, for now
    owner0 = assert_matches_twin(m, make_nested, prec, x, y, child0, "owner after the child ran alone")
    assert m.vit._fer_flat is None and m._fer_flat is not None  # one store: the owner's

    # the optimizer built before any forward steps the buffers the kernels read
    pre = [p.detach().clone() for p in m.parameters()]
    opt.step()
    assert all(not torch.equal(a, p.detach()) for a, p in zip(pre, m.parameters()) if p.requires_grad)
    owner1 = assert_matches_twin(m, make_nested, prec, x, y, owner0, "owner after the optimizer step")

    # a child parameter edited in place: the child alone, then the owner
    params = dict(m.named_parameters())
    with torch.no_grad():
        params[CHILD_W].mul_(1.5)
        params[CHILD_B].mul_(1.5)
    child1 = assert_matches_twin(m, make_nested, prec, xc, y, child0, "child alone after the edit", sub="vit")
    assert_matches_twin(m, make_nested, prec, x, y, owner1, "owner after the edit")
    # ... and the other way round
    with torch.no_grad():
        params[CHILD_W].mul_(1.5)
    owner2 = run(m, x, y)[0]
    assert_matches_twin(m, make_nested, prec, xc, y, child1, "child alone after the owner saw the edit", sub="vit")
    assert_matches_twin(m, make_nested, prec, x, y, owner1, "owner at the end")
    assert not torch.equal(owner2, owner1)
    if prec == "bf16":
        assert_shadow_is_current(m)
