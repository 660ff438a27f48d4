"""The gate of tests/test_gpu_layers_elementwise.py checked without a GPU: the float32
and bf16 emulations of tests/layer_ref.py must pass the very comparison the modules get on the GPU, with the
constants measured here, and seven wrong variants of the post-norm layer's backward (each a way the pairing of a
forward and a backward kernel can break) must fail it on at least one tensor, in fp32 and in bf16. The seeds
the GPU test uses must give every dropout site a keep rate near 1 - p."""
import pytest
import torch

import layer_ref as L
from elemwise import assert_close

DTYPES = ("fp32", "bf16")
ALL = [c for cs in L.CASES.values() for c in cs]
SLIPS = ("seeds_1_3_swapped_bwd", "out_mask_ld_plus4_bwd", "fc2_scale_missing_bwd", "dx1_residual_from_dh2",
         "gb1_ungated", "attn_mask_transposed")
P01 = [c for c in L.POST_NORM_CASES if c.p == 0.1 and c.passes == 1 and c.D == 96 and c.act == "gelu"]
TWO_PASS = [c for c in L.POST_NORM_CASES if c.passes == 2]


class Slip(L.Numerics):
    """The emulation with one slip. The mask slips only change the masks one side of a site sees; the other two
    use the hooks of the formula."""

    def __init__(self, dtype, slip):
        super().__init__(L.emulate(dtype).kind)
        self.slip = slip
        self.fc2 = None

    def masks_of(self, case, pas, device="cpu"):
        m = L.case_masks(case, pas, device)
        s = L.site_seeds(case.seed, 4 * (pas + 1))[4 * pas:]
        B, N, D, p = case.B, case.N, case.D, case.p
        out, fc2 = m["out"], m["fc2"]
        self.fc2 = fc2
        if self.slip == "seeds_1_3_swapped_bwd":
            m["out"], m["fc2"] = (out, fc2), (fc2, out)
        elif self.slip == "out_mask_ld_plus4_bwd":
            m["out"] = (out, L.epilogue_mask(s[1], B * N, D, p, drop_ld=D + 4).view(B, N, D))
        elif self.slip == "fc2_scale_missing_bwd":
            m["fc2"] = (fc2, (fc2 > 0).to(fc2.dtype))
        elif self.slip == "attn_mask_transposed":
            m["attn"] = m["attn"].transpose(-1, -2).contiguous()
        return m

    def residual(self, t, site):
        if self.slip == "dx1_residual_from_dh2" and site == "ffn":
            return L._MaskMul.apply(t, torch.ones_like(t), self.fc2.to(t.dtype))
        return t

    def gate(self, lin, b, fn, site):
        if self.slip == "gb1_ungated" and site == "fc1":
            return fn(lin + b.detach()) + (b - b.detach())
        return fn(lin + b)


def failing(got, ref, c, dtype):
    bad = []
    for k, r in ref.items():
        try:
            assert_close(k, got[k], r, L.scale_of(k, r), c, L.out_round(dtype))
        except AssertionError:
            bad.append(k)
    return bad


@pytest.fixture(scope="module")
def refs():
    return {c: L.run_case(c, L.REF) for c in ALL}


@pytest.mark.parametrize("kind,act", [(k, a) for k in sorted(L.CASES) for a in sorted({c.act for c in L.CASES[k]})])
def test_clean_emulation_within_gate(kind, act, refs):
    c = L.c_table(kind, act)
    print(f"c-table {kind} {act} fp32 {c['fp32']:.1f} bf16 {c['bf16']:.1f}")
    for case in (c_ for c_ in L.CASES[kind] if c_.act == act):
        for dtype in case.dtypes:
            w = L.compare(f"{case.id} {dtype}", L.run_case(case, L.emulate(dtype)), refs[case], c[dtype], dtype)
            k = max(w, key=w.get)
            print(f"worst err/bound {case.id} {dtype}: {w[k]:.3f} ({k})")
            assert w[k] <= 1.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("slip", SLIPS)
@pytest.mark.parametrize("case", P01, ids=lambda c: c.id)
def test_slip_fails_the_gate(case, slip, dtype, refs):
    num = Slip(dtype, slip)
    bad = failing(L.run_case(case, num, masks_of=num.masks_of), refs[case], L.c_table("post_norm")[dtype], dtype)
    print(f"slip {slip} {dtype} {case.id}: {len(bad)} tensors out of bound: {' '.join(bad)}")
    assert bad, f"{slip} passes the {dtype} gate"


@pytest.mark.parametrize("dtype", DTYPES)
def test_fc2_scale_slip_at_half(dtype, refs):
    """At p = 0.5 a missing 1 / (1 - p) is a factor 2."""
    case = next(c for c in L.POST_NORM_CASES if c.p == 0.5)
    num = Slip(dtype, "fc2_scale_missing_bwd")
    bad = failing(L.run_case(case, num, masks_of=num.masks_of), refs[case], L.c_table("post_norm")[dtype], dtype)
    print(f"slip fc2_scale_missing_bwd {dtype} {case.id}: {len(bad)} tensors out of bound: {' '.join(bad)}")
    assert bad


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", TWO_PASS, ids=lambda c: c.id)
def test_overwriting_second_backward_fails_the_gate(case, dtype, refs):
    got = L.run_case(case, L.emulate(dtype), accumulate=False)
    bad = failing(got, refs[case], L.c_table("post_norm")[dtype], dtype)
    print(f"slip second_backward_overwrites {dtype} {case.id}: {len(bad)} tensors out of bound: {' '.join(bad)}")
    assert bad
    assert not {"out", "dx"} & set(bad)  # those belong to the last pass either way


@pytest.mark.parametrize("case", [c for c in ALL if c.p > 0], ids=lambda c: c.id)
def test_keep_rates_of_the_gpu_seeds(case):
    """A condition on the inputs: each site of each pass keeps 1 - p of its elements within 0.05 ([0.85, 0.95]
    at p = 0.1), so no mask is degenerate and none is another site's."""
    for pas in range(case.passes):
        m = L.case_masks(case, pas)
        sites = {"layer": m}
        if case.kind == "image_vit":
            sites = {"tokens": {"tokens": m[0]}, "layer0": m[1], "layer1": m[2]}
        for where, ms in sites.items():
            for site, rate in L.keep_rates(ms).items():
                assert abs(rate - (1.0 - case.p)) <= 0.05, (case.id, pas, where, site, rate)


def test_site_seeds_replicate_the_global_stream():
    import fervit
    from fervit import runtime

    saved = (runtime.SEEDS.base, runtime.SEEDS.counter)
    try:
        fervit.manual_seed(11)
        drawn = [runtime.next_seed() for _ in range(18)]
    finally:
        runtime.SEEDS.base, runtime.SEEDS.counter = saved
    assert drawn == L.site_seeds(11, 18)
    assert len(set(drawn)) == 18
