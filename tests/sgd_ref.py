"""numpy restatement of libbnn's SGD element (sgd_elem, csrc/bnn_common.h), in fp32 with one rounding per
operation, exactly as the kernels evaluate it:

    g   = g * gscale
    g   = fmaf(wd, p, g)                                  if wd != 0
    buf = g if first else fmaf(omd, g, mu * buf)          if mu != 0     (omd = (float)(1 - dampening))
    g   = fmaf(mu, buf, g) if nesterov else buf           if mu != 0
    p   = fmaf(-lr, g, p)
    p   = fminf(fmaxf(p, -1), 1)                          if clamp

This is torch.optim.SGD's arithmetic with one fused multiply-add wherever torch has an add(.., alpha=..);
tests/test_sgd.py holds it to torch's CPU fp32 result bit for bit.  The fma is bn_ref's exactly rounded one
(float64 product, sum corrected to round-to-odd before the cast: no double rounding).

Shared by test_sgd.py (CPU) and test_gpu_sgd.py.
"""
import numpy as np

from bn_ref import fma

F32 = np.float32

# (momentum, dampening, weight_decay, nesterov)
SETTINGS = [(0.0, 0.0, 0.0, False), (0.0, 0.0, 1e-2, False), (0.9, 0.0, 0.0, False), (0.9, 0.1, 5e-4, False),
            (0.95, 0.0, 5e-4, True)]
GSCALES = [1.0, 1.0 / 3.0]


def omd_of(dampening):
    """The multiplier the C entries take: 1 - dampening in double, then float (torch's alpha)."""
    return F32(1.0 - float(dampening))


def sgd_step(p, g, buf, lr, mu=0.0, dampening=0.0, wd=0.0, nesterov=False, first=False, gscale=1.0, clamp=True):
    """One step on fp32 arrays; returns (p_new, buf_new).  buf_new is None when mu == 0; ``buf`` is not
    read when ``first``."""
    p = np.asarray(p, F32)
    lr, mu, wd, gs, omd = F32(lr), F32(mu), F32(wd), F32(gscale), omd_of(dampening)
    g = (np.asarray(g, F32) * gs).astype(F32)
    if wd != 0:
        g = fma(wd, p, g)
    if mu != 0:
        buf = g.copy() if first else fma(omd, g, (mu * np.asarray(buf, F32)).astype(F32))
        g = fma(mu, buf, g) if nesterov else buf
    else:
        buf = None
    p = fma(-lr, g, p)
    if clamp:
        p = np.minimum(np.maximum(p, F32(-1)), F32(1))
    return p, buf


def make_p0(n, rng):
    """p0 uniform in +-1.1 with 1 % exact zeros: the clamp and the zero sign both occur."""
    p0 = rng.uniform(-1.1, 1.1, n).astype(F32)
    p0[rng.random(n) < 0.01] = 0
    return p0


def make_grad(n, rng):
    return rng.standard_normal(n).astype(F32)
