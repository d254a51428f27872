"""numpy restatement of libbnn's Bop element (bop_elem, csrc/bnn_common.h), in fp32 with one rounding per
operation, exactly as the kernels evaluate it:

    gi = g * gscale
    m' = m + gamma * (gi - m)           three roundings: sub, mul, add (no fma)
    s  = -1 if w < 0 else +1            0, -0 and NaN count as +1
    flip = s * m' > threshold           strict: a tie or a NaN average does not flip
    w' = -s if flip else s              exactly +-1

Bop is the binary optimizer of Helwegen et al., "Latent Weights Do Not Exist: Rethinking Binarized Neural
Network Optimization" (NeurIPS 2019).  tests/test_bop.py holds this restatement to the same formula written
in torch CPU fp32 ops bit for bit.

Shared by test_bop.py (CPU) and test_gpu_bop.py.
"""
import numpy as np

F32 = np.float32

# The makers' setting.  With standard normal gradients the average after two steps from m = 0 is
# 0.1875 g1 + 0.25 g2 ~ N(0, 0.3125^2) at gscale 1 and N(0, 0.104^2) at gscale 1/3, so
# P(s m' > 0.125) = P(z > 0.4) = 34 % and P(z > 1.2) = 12 %: inside the 5 to 50 % band the tests ask for.
GAMMA = 0.25
THRESHOLD = 0.125
GSCALES = [1.0, 1.0 / 3.0]


def bop_step(w, g, m, gamma, threshold, gscale=1.0):
    """One step on fp32 arrays; returns (w_new, m_new, flips)."""
    w, g, m = np.asarray(w, F32), np.asarray(g, F32), np.asarray(m, F32)
    gamma, thr, gs = F32(gamma), F32(threshold), F32(gscale)
    with np.errstate(invalid="ignore", over="ignore"):
        gi = (g * gs).astype(F32)
        d = (gi - m).astype(F32)
        m2 = (m + (gamma * d).astype(F32)).astype(F32)
        s = np.where(w < 0, F32(-1), F32(1)).astype(F32)
        flip = (s * m2).astype(F32) > thr
    w2 = np.where(flip, -s, s).astype(F32)
    return w2, m2, int(flip.sum())


def make_w0(n, rng):
    """Latent-like initial values: uniform in +-1.1, with exact 0.0 and -0.0 (both count as +1) and values
    that are already +-1."""
    w = rng.uniform(-1.1, 1.1, n).astype(F32)
    u = rng.random(n)
    w[u < 0.02] = F32(0.0)
    w[(u >= 0.02) & (u < 0.04)] = F32(-0.0)
    w[(u >= 0.04) & (u < 0.14)] = F32(1.0)
    w[(u >= 0.14) & (u < 0.24)] = F32(-1.0)
    return w


def make_grad(n, rng):
    return rng.standard_normal(n).astype(F32)


def make_tie(n, rng, threshold=2.0 ** -7):
    """The tie cases: m = 0, gamma = 0.5, gscale = 1 and a power-of-two threshold.  g = +-2 * threshold makes
    m' exactly +-threshold (no flip: the comparison is strict); g = +-4 * threshold makes it +-2 * threshold,
    which flips exactly where it has the weight's sign.  Returns (w, g, must_flip, settings)."""
    w = make_w0(n, rng)
    sign = np.where(rng.random(n) < 0.5, F32(-1), F32(1))
    big = rng.random(n) < 0.5
    g = (sign * np.where(big, F32(4 * threshold), F32(2 * threshold))).astype(F32)
    s = np.where(w < 0, F32(-1), F32(1))
    must_flip = big & (sign == s)
    return w, g, must_flip, dict(gamma=0.5, threshold=threshold, gscale=1.0)
