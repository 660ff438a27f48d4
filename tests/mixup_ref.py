"""Host mirrors of fer_mixup_draw (csrc/mixup.hip): the permutation in integers (exact) and lam in float64 from
the kernel's own float32 uniforms, with the hash, the step-counter mix and the uniform map of tests/dropmask.py.
Shared by tests/test_mixup_ref_cpu.py and the GPU tests, together with the gates both apply to the draws
(DESIGN.md section 2.14)."""
import math

import numpy as np

from dropmask import fer_hash, step_seed, u01

PERM_XOR = 0x2545F4914F6CDD1D
GAMMA_XOR = (0x9FB21C651E98DF25, 0xD6E8FEB86659FD93)
ATTEMPTS = 16  # csrc/mixup.hip MIXUP_ATTEMPTS
MAX_B = 2048

SEED = 0x1F3D5B79A2C4E608  # the fixed seed of the statistical gates; its sets 0..N_DRAWS-1 are the draws
N_DRAWS = 4096
KS_LIMIT = math.sqrt(math.log(2e6) / 2) / math.sqrt(N_DRAWS)  # 0.0421: the 1e-6 level at n = 4096
# |device lam - mirror| over the 4,096 draws of each alpha in (0.5, 1, 2), draws on an accept / reject boundary left
# out: 8 x the worst difference of the first GPU run, LAM_WORST
LAM_WORST = 2.885e-7  # alpha 1; 2.462e-7 at alpha 0.5, 1.802e-7 at alpha 2
LAM_TOL = 8 * LAM_WORST
MARGIN = 1e-4  # a draw whose accept / reject margin is below this may go the other way in float32
CDF = {0.5: lambda x: (2 / math.pi) * np.arcsin(np.sqrt(x)), 1.0: lambda x: x, 2.0: lambda x: 3 * x ** 2 - 2 * x ** 3}


def stream_seed(seed: int, s: int = 0, counter=None) -> int:
    """csrc/step_seed.h step_stream_seed: the seed mixed with the step counter (None: none registered), then
    with the set index by the same finaliser."""
    return step_seed(seed if counter is None else step_seed(seed, counter), s)


def perm(ss: int, B: int) -> np.ndarray:
    """perm[i] = rank of (fer_hash(ss ^ PERM_XOR, i), i)."""
    idx = np.arange(B, dtype=np.uint64)
    keys = fer_hash(ss ^ PERM_XOR, idx)
    order = np.lexsort((idx, keys))  # by key, ties by index
    rank = np.empty(B, dtype=np.int32)
    rank[order] = np.arange(B, dtype=np.int32)
    return rank


def perm_by_definition(ss: int, B: int) -> np.ndarray:
    """The same, counted pair by pair as the kernel does."""
    keys = [int(k) for k in fer_hash(ss ^ PERM_XOR, np.arange(B, dtype=np.uint64))]
    return np.array([sum(1 for j in range(B) if (keys[j], j) < (keys[i], i)) for i in range(B)], dtype=np.int32)


def log_gamma(alpha: float, seed: int):
    """(log of the Gamma(alpha) draw, attempts used or None when all were rejected, smallest accept / reject
    margin met on the way)."""
    a = alpha + 1.0 if alpha < 1.0 else alpha
    d = a - 1.0 / 3.0
    c = 1.0 / math.sqrt(9.0 * d)
    u = u01(fer_hash(seed, np.arange(3 * ATTEMPTS + 1, dtype=np.uint64))).astype(np.float64)
    g, used, margin = d, None, math.inf
    for t in range(ATTEMPTS):
        x = math.sqrt(-2.0 * math.log(u[3 * t])) * math.cos(2.0 * math.pi * u[3 * t + 1])
        w = 1.0 + c * x
        margin = min(margin, abs(w))
        if w <= 0.0:
            continue
        v = w ** 3
        lhs, rhs = math.log(u[3 * t + 2]), 0.5 * x * x + d - d * v + d * math.log(v)
        margin = min(margin, abs(rhs - lhs))
        if lhs < rhs:
            g, used = d * v, t + 1
            break
    lg = math.log(g)
    if alpha < 1.0:
        lg += math.log(u[3 * ATTEMPTS]) / alpha
    return lg, used, margin


def lam(ss: int, alpha: float):
    """(lam, capped: a Gamma draw ran out of attempts, margin)."""
    alpha = float(np.float32(alpha))
    if not alpha > 0.0:
        return 1.0, False, math.inf
    (l1, n1, m1), (l2, n2, m2) = (log_gamma(alpha, ss ^ x) for x in GAMMA_XOR)
    e = l2 - l1
    return (0.0 if e > 700 else 1.0 / (1.0 + math.exp(e))), n1 is None or n2 is None, min(m1, m2)


def draw(seed: int, alpha: float, B: int, s: int = 0, counter=None):
    """(lam, perm) of set s as fer_mixup_draw(alpha, B, seed, ...) gives them with the device counter holding
    `counter` (None: no counter registered)."""
    ss = stream_seed(seed, s, counter)
    return lam(ss, alpha)[0], perm(ss, B)


def lam_draws(alpha: float, seed: int = SEED, n: int = N_DRAWS):
    """lam, capped and margin of sets 0..n-1 as arrays."""
    rows = [lam(stream_seed(seed, s), alpha) for s in range(n)]
    return (np.array([r[0] for r in rows]), np.array([r[1] for r in rows]), np.array([r[2] for r in rows]))


def ks_statistic(samples, cdf) -> float:
    x = np.sort(np.asarray(samples, dtype=np.float64))
    n = len(x)
    f = cdf(x)
    return float(max((np.arange(1, n + 1) / n - f).max(), (f - np.arange(n) / n).max()))


def cell_counts(perms: np.ndarray) -> np.ndarray:
    """perms [n][B] -> counts [B][B] of (i, perm[i])."""
    n, B = perms.shape
    counts = np.zeros((B, B), dtype=np.int64)
    for i in range(B):
        counts[i] = np.bincount(perms[:, i], minlength=B)
    return counts


def cell_gate(perms: np.ndarray) -> None:
    """B = 5 over 4,096 draws: every (i, perm[i]) cell within 6 sigma of n / B (819.2, sigma 25.6)."""
    n, B = perms.shape
    sigma = math.sqrt(n * (1 / B) * (1 - 1 / B))
    counts = cell_counts(perms)
    worst = np.abs(counts - n / B).max()
    assert worst <= 6 * sigma, (counts.tolist(), worst, 6 * sigma)
