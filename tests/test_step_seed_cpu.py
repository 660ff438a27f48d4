"""The device step counter's seed mix without a GPU: the host replica
dropmask.step_seed against known answers; the table of step_seed( call sites of
tests/test_gpu_step_seed_kernels.py against the sources, and a GPU case for every one of them; and, for the
replayed step of tests/test_gpu_graph_dropout.py, the constant of its gate measured with the replays' masks, the
emulations inside that gate, replays that the gate tells apart, and the keep rates of the mixed seeds."""
import os
import re

import pytest

import layer_ref as L
import test_gpu_step_seed_kernels as K
from dropmask import step_seed

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fer-vit_amd", "csrc")
GOLDEN = 0x9E3779B97F4A7C15
CASE = L.IMAGE_VIT_CASES[0]
DRAWN, REPLAYS = 9, 3  # StepGraph(warmup=1): nine host seeds before the capture; three replays


# ---------------------------------------------------------------------- the replica
def splitmix64_stream(state, n):
    """The textbook generator: state += golden; output = finaliser(state)."""
    out = []
    for _ in range(n):
        state = (state + GOLDEN) & (2 ** 64 - 1)
        z = state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1)
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2 ** 64 - 1)
        out.append(z ^ (z >> 31))
    return out


def test_step_seed_known_answers():
    first, second = splitmix64_stream(0, 2)
    assert first == 0xE220A8397B1DCDAF  # the first output of splitmix64 from state 0
    assert step_seed(0, 1) == first  # 0 ^ (1 * golden) is that generator's first state
    assert step_seed(0, 2) == second  # 2 * golden its second
    assert step_seed(GOLDEN, 0) == first  # counter 0: the finaliser of the seed itself
    s = 0xC3A51F0E9D2764B1
    assert step_seed(s, 0) != s  # a registered counter at 0 still mixes
    assert step_seed(s, 1) != step_seed(s, 2 ** 32 + 1)  # the counter's high word counts
    assert step_seed(s, 2 ** 64 + 3) == step_seed(s, 3)  # 64-bit arithmetic
    for c in (0, 1, 2 ** 32 + 5, 2 ** 64 - 1):
        assert 0 <= step_seed(s, c) < 2 ** 64
        assert 0 <= step_seed(2 ** 64 - 1, c) < 2 ** 64


def test_step_seed_is_the_formula_of_the_header():
    """The constants and shifts the replica uses are the ones csrc/step_seed.h spells out."""
    src = open(os.path.join(CSRC, "step_seed.h")).read()
    for text in ("seed ^ (c * 0x9E3779B97F4A7C15ull)", "(z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull",
                 "(z ^ (z >> 27)) * 0x94D049BB133111EBull", "return z ^ (z >> 31);", "if (!p) return seed;"):
        assert text in src, text


# ---------------------------------------------------------------------- call sites and their cases
def sites_in(path):
    """The __global__ function around every step_seed( occurrence of a source file, in file order; a kernel
    with several occurrences is numbered name#1, name#2, ..."""
    src = open(path).read()
    kernels = [(m.start(), m.group(1)) for m in re.finditer(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", src, re.S)]
    names = []
    for m in re.finditer(r"step_seed\(", src):
        before = [name for pos, name in kernels if pos < m.start()]
        assert before, f"{path}: step_seed( ahead of the first kernel"
        names.append(before[-1])
    return [n if names.count(n) == 1 else f"{n}#{names[:i].count(n) + 1}" for i, n in enumerate(names)]


def test_site_table_matches_the_sources():
    found = {f: sites_in(os.path.join(CSRC, f)) for f in sorted(os.listdir(CSRC)) if f.endswith(".hip")}
    found = {f: s for f, s in found.items() if s}
    assert {f: len(s) for f, s in found.items()} == K.SITES, \
        "a step_seed( call site was added or removed: update SITES, SITE_KERNELS and CASES of tests/test_gpu_step_seed_kernels.py"
    assert found == K.SITE_KERNELS


def test_every_site_has_a_gpu_case():
    assert len(K.CASES) >= sum(K.SITES.values())
    for f, kernels in K.SITE_KERNELS.items():
        assert len(kernels) == K.SITES[f]
        claimed = {s for c in K.CASES.values() if c.file == f for s in c.sites}
        assert claimed == set(kernels), f"{f}: sites without a case {set(kernels) - claimed}, unknown {claimed - set(kernels)}"
    for name, c in K.CASES.items():
        assert c.file in K.SITES and c.sites, name


# ---------------------------------------------------------------------- the replayed step's gate
def masks_of(r):
    return lambda case, pas, device="cpu": L.replay_masks(case, DRAWN, r, device)


@pytest.fixture(scope="module")
def replay_refs():
    return {r: L.run_case(CASE, L.REF, masks_of=masks_of(r), accumulate=False) for r in range(1, REPLAYS + 1)}


def test_replay_seeds_are_the_captured_pass_mixed():
    host = L.site_seeds(CASE.seed, 18)
    assert len({step_seed(h, r) for h in host[9:] for r in (0, 1, 2, 3)} | set(host)) == 18 + 9 * 4
    a = L.replay_masks(CASE, DRAWN, 1)
    b = L.image_vit_masks(CASE, [step_seed(h, 1) for h in host[9:]])
    assert all((x == y).all() for x, y in zip([a[0], *a[1].values(), *a[2].values()], [b[0], *b[1].values(), *b[2].values()]))


@pytest.mark.parametrize("dtype", CASE.dtypes)
def test_replayed_emulation_within_gate_and_replays_told_apart(dtype, replay_refs):
    """c of the replayed step: the table's (eager masks) unless the same measurement with the replays' masks is
    larger. Both emulations pass the gate against their own replay's reference and fail it against the next
    replay's and against the unmixed seeds 10 to 18: the gate tells the mask sets apart."""
    c, own = L.replay_c_table(CASE, DRAWN, REPLAYS)[dtype]
    table = L.c_table(CASE.kind, CASE.act)[dtype]
    print(f"c-replay {CASE.id} {dtype}: measured {own:.1f}, table {table:.1f}, used {c:.1f}")
    assert c == max(table, own)
    unmixed = L.run_case(CASE, L.REF, masks_of=lambda case, pas, device="cpu": L.case_masks(case, 1, device),
                         accumulate=False)
    for r in range(1, REPLAYS + 1):
        got = L.run_case(CASE, L.emulate(dtype), masks_of=masks_of(r), accumulate=False)
        w = L.compare(f"replay {r} {dtype}", got, replay_refs[r], c, dtype)
        k = max(w, key=w.get)
        print(f"worst err/bound replay {r} {dtype}: {w[k]:.3f} ({k})")
        with pytest.raises(AssertionError):
            L.compare(f"replay {r} against replay {r % REPLAYS + 1}", got, replay_refs[r % REPLAYS + 1], c, dtype)
        with pytest.raises(AssertionError):
            L.compare(f"replay {r} against the unmixed seeds", got, unmixed, c, dtype)


@pytest.mark.parametrize("r", range(1, REPLAYS + 1))
def test_keep_rates_of_the_replay_seeds(r):
    """As tests/test_layer_bound_cpu.py for the eager seeds: every site keeps 1 - p within 0.05."""
    m = L.replay_masks(CASE, DRAWN, r)
    for where, ms in {"tokens": {"tokens": m[0]}, "layer0": m[1], "layer1": m[2]}.items():
        for site, rate in L.keep_rates(ms).items():
            assert abs(rate - (1.0 - CASE.p)) <= 0.05, (CASE.id, r, where, site, rate)
