"""numpy restatement of libbnn's stochastic binarization (csrc/bnn_common.h ssign):

    seed' = seed + ctr * 0xD1B54A32D192ED03          (ctr: the device step counter, 0 without one)
    h     = fmix32(i * 0x9E3779B1 ^ key(seed'))      (the dropout passes' counter hash, element i mod 2^32)
    p     = min(max(fmaf(x, 0.5, 0.5), 0), 1)
    t     = uint32(p * 2^24)
    s     = 0 if isnan(x) else (+1 if (h >> 8) < t else -1)

Shared by test_stochastic.py (CPU) and test_gpu_stochastic.py.
"""
import numpy as np

M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF
CTR_GOLDEN = 0xD1B54A32D192ED03
SALT_GOLDEN = 0x9E3779B97F4A7C15


def fmix32(h):
    h = np.asarray(h, dtype=np.uint64) & M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    return h ^ (h >> 16)


def key(seed):
    seed = int(seed) & M64
    return (seed & M32) ^ int(fmix32(((seed >> 32) ^ 0x5BD1E995) & M32))


def hash32(seed, n, ctr=0):
    """drop_hash(seed + ctr * golden, i) for i = 0 .. n-1 (uint64 array of 32-bit values)."""
    k = key((int(seed) + int(ctr) * CTR_GOLDEN) & M64)
    i = np.arange(n, dtype=np.uint64) & M32
    return fmix32(((i * 0x9E3779B1) & M32) ^ np.uint64(k))


def threshold(x):
    """t = uint32(clamp(fmaf(x, .5, .5), 0, 1) * 2^24) per element; NaN -> 0 (masked by the caller).
    x * 0.5 + 0.5 in float64 is exact for every float32 x the sum does not absorb, so the one rounding
    to float32 is fmaf's."""
    x = np.asarray(x, dtype=np.float32)
    nan = np.isnan(x)
    with np.errstate(invalid="ignore", over="ignore"):
        p = (np.where(nan, 0.0, x).astype(np.float64) * 0.5 + 0.5).astype(np.float32)
    p = np.clip(p, np.float32(0), np.float32(1))
    return np.where(nan, 0, (p.astype(np.float64) * 16777216.0).astype(np.uint64)).astype(np.uint64)


def binarize(x, seed, ctr=0):
    """The draw for a contiguous float32 array x (any shape; element index = flat index): float32 +-1 / 0."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    h = hash32(seed, x.size, ctr).reshape(x.shape)
    s = np.where((h >> 8) < threshold(x), 1.0, -1.0).astype(np.float32)
    s[np.isnan(x)] = 0.0
    return s


def site_seed(base, salt):
    return (int(base) + int(salt) * SALT_GOLDEN) & M64
