"""Host replica of the kernels' counter-based dropout hash (csrc/common.h fer_hash /
drop_keep), so tests can rebuild the exact keep-mask a kernel used."""
import numpy as np
import torch

_M32 = np.uint64(0xFFFFFFFF)


def _u32(x):
    return np.asarray(x, dtype=np.uint64) & _M32


def fer_hash(seed: int, pair: np.ndarray) -> np.ndarray:
    """csrc/common.h fer_hash: x = (pair ^ seed_lo) + seed_hi, then the lowbias32 finaliser."""
    pair = _u32(pair)
    s_lo, s_hi = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    with np.errstate(over="ignore"):
        x = _u32((pair ^ s_lo) + s_hi)
        x ^= x >> np.uint64(16)
        x = _u32(x * np.uint64(0x7FEB352D))
        x ^= x >> np.uint64(15)
        x = _u32(x * np.uint64(0x846CA68B))
        x ^= x >> np.uint64(16)
    return x


_M64 = 0xFFFFFFFFFFFFFFFF


def step_seed(seed: int, counter: int) -> int:
    """csrc/step_seed.h step_seed with a device counter registered and holding `counter`: the splitmix64
    finaliser of seed ^ (counter * 0x9E3779B97F4A7C15), everything in 64 bits. A counter of 0 still mixes (the
    finaliser of the seed itself); only an unregistered counter leaves the seed as it is."""
    z = ((seed & _M64) ^ ((counter & _M64) * 0x9E3779B97F4A7C15)) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def thresh(p: float) -> int:
    return max(1, min(65535, int(round(p * 65536.0))))


def keep_mask(seed: int, shape, p: float, base: int = 0) -> torch.Tensor:
    n = int(np.prod(shape))
    idx = np.arange(base, base + n, dtype=np.uint64) & _M32  # element indices are 32-bit
    h = fer_hash(seed, idx >> np.uint64(1))
    u = (h >> ((idx & np.uint64(1)) * np.uint64(16))) & np.uint64(0xFFFF)
    return torch.from_numpy((u >= np.uint64(thresh(p))).reshape(shape))


def keep_mask_torch(seed: int, shape, p: float, device="cuda") -> torch.Tensor:
    """keep_mask computed with int64 torch ops on `device` (large masks: a GPU test's attention
    dropout over B*H*N*N elements). 32-bit products are split into 16-bit halves so no int64
    product overflows."""
    n = int(np.prod(shape))
    m32 = 0xFFFFFFFF
    idx = torch.arange(n, dtype=torch.int64, device=device) & m32

    def mul32(x, c):
        return ((x * (c & 0xFFFF)) + (((x * (c >> 16)) & 0xFFFF) << 16)) & m32

    x = ((idx >> 1) ^ (seed & m32)) + ((seed >> 32) & m32)
    x &= m32
    x ^= x >> 16
    x = mul32(x, 0x7FEB352D)
    x ^= x >> 15
    x = mul32(x, 0x846CA68B)
    x ^= x >> 16
    u = (x >> ((idx & 1) * 16)) & 0xFFFF
    return (u >= thresh(p)).reshape(shape)


# ---------------------------------------------------------------------- latent augmentation draws
# csrc/wplus.hip latent_augment_kernel: three streams keyed by sub-seeds of the call's seed (step counter
# unset), each a fer_hash of a 32-bit counter mapped to (0, 1] by u01.
SCALE_XOR = 0x5851F42D4C957F2D
MASK_XOR = 0x14057B7EF767814F


def sub_seeds(seed: int):
    """(noise, scale, mask) seeds of fer_latent_augment."""
    return seed, seed ^ SCALE_XOR, seed ^ MASK_XOR


def u01(h: np.ndarray) -> np.ndarray:
    """csrc/wplus.hip u01 in the kernel's own float32 arithmetic: ((float)(h >> 8) + 0.5f) * 2^-24. The sum
    is rounded to float32 (to even above 2^23), so the top value is 1.0 and the bottom one 2^-25."""
    k = (_u32(h) >> np.uint64(8)).astype(np.float32)
    return (k + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def augment_draws(seed: int, n: int, B: int):
    """float32 (u1, u2) of the Box-Muller noise and the mask uniform of elements 0..n-1, and the scale
    uniform of samples 0..B-1."""
    s_noise, s_scale, s_mask = sub_seeds(seed)
    e = np.arange(n, dtype=np.uint64)
    u1 = u01(fer_hash(s_noise, 2 * e))
    u2 = u01(fer_hash(s_noise, 2 * e + 1))
    um = u01(fer_hash(s_mask, e))
    us = u01(fer_hash(s_scale, np.arange(B, dtype=np.uint64)))
    return u1, u2, um, us
