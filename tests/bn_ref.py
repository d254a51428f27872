"""numpy restatement of libbnn's BatchNorm element functions (csrc/bnn_common.h, csrc/bnn_bn2d.h), in
fp32 with one rounding per operation, exactly as the kernels evaluate them:

    xh  = ((x - mean) - mean_lo) * invstd                       bn_xh1   (three roundings)
    y   = fmaf(xh, gamma, beta)                                 bn_y1    (one rounding)
    v   = fminf(fmaxf(y, -1), 1)                                Hardtanh (a NaN y clamps to -1: fmaxf
                                                                          returns its non-NaN operand)
    g   = dy if (no Hardtanh or -1 < y < 1) else 0              strict mask
    dz  = (gamma * invstd) * ((g - a0) - xh * a1)               bn_dz1   (contraction off: 5 roundings)
          a0 = k0 * inv_n, a1 = k1 * inv_n, inv_n = 1.f / (float)M (0 in eval mode)
    2d: dz = (gamma * invstd) * fmaf(-xh, m1, g - m0)           bn2_window_dz / bn2d_bwd_apply_k: these
          are compiled with the default contraction, which fuses the product into the subtraction;
          inv_n = (float)(1.0 / ((double)N * (double)(H * W)))
    dropout: x' = x * mask where mask != 0 else 0, dx = dz * mask where mask != 0 else 0, with the
          mask bnn_dropout_mask returns (1 / (1 - p) or 0 per element)
    2x2 window (bn2_window): the four values in (h, w) scan order, best = -inf, arg = 0; value j
          replaces best when v_j > best or v_j is NaN (first strictly greater, NaN wins)

The fma is exact: the product of two fp32 values is exact in float64, the float64 sum is corrected to
round-to-odd with its TwoSum error term, and round-to-odd at 53 bits followed by round-to-nearest at 24
bits is the correctly rounded result (53 >= 2 * 24 + 2).  Rounding the float64 sum twice instead is
wrong exactly where it lands on an fp32 halfway case; tests/test_bn_ref.py constructs those.

Shared by test_bn_ref.py (CPU) and test_gpu_bn_elementwise.py.
"""
import numpy as np

F32 = np.float32


def f32(a):
    return np.asarray(a, dtype=np.float32)


def fma(a, b, c):
    """Correctly rounded fp32 a * b + c, element-wise (fmaf)."""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b                                   # exact: 48 significant bits
        s = p + c
        bb = s - p                                  # TwoSum: s + err == p + c exactly
        err = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0)
        bits = np.ascontiguousarray(np.broadcast_to(s, np.broadcast(s, err).shape)).copy().view(np.int64)
        even = (bits & 1) == 0
        step = np.where((err > 0) == (bits >= 0), 1, -1)   # one ulp towards the exact value
        bits += np.where(fix & even, step, 0)               # the odd one of the two bracketing doubles
        return bits.view(np.float64).astype(np.float32)


def xh1(x, m, lo, istd):
    with np.errstate(invalid="ignore", over="ignore"):
        return ((f32(x) - f32(m)) - f32(lo)) * f32(istd)


def y1(x, m, lo, istd, ga, be):
    return fma(xh1(x, m, lo, istd), ga, be)


def clamp(y):
    """fminf(fmaxf(y, -1), 1): NaN -> -1."""
    y = f32(y)
    return np.where(np.isnan(y), F32(-1), np.minimum(np.maximum(y, F32(-1)), F32(1))).astype(np.float32)


def forward(x, m, lo, istd, ga, be, hardtanh):
    y = y1(x, m, lo, istd, ga, be)
    return clamp(y) if hardtanh else y


def mask_g(y, dy, hardtanh):
    dy = f32(dy)
    if not hardtanh:
        return np.broadcast_to(dy, np.broadcast(y, dy).shape)
    with np.errstate(invalid="ignore"):
        return np.where((y > F32(-1)) & (y < F32(1)), dy, F32(0)).astype(np.float32)


def inv_n_1d(M):
    return F32(1) / F32(M)


def inv_n_2d(N, H, W):
    return F32(1.0 / (float(N) * float(H * W)))


def dz1(x, dy, m, lo, istd, ga, be, k0, k1, inv_n, hardtanh):
    """bn_dz1 (BatchNorm1d backward apply); inv_n = 0 in eval mode."""
    xh = xh1(x, m, lo, istd)
    g = mask_g(fma(xh, ga, be), dy, hardtanh)
    with np.errstate(invalid="ignore", over="ignore"):
        a0, a1 = f32(k0) * F32(inv_n), f32(k1) * F32(inv_n)
        return (f32(ga) * f32(istd)) * ((g - a0) - xh * a1)


def dz2_flat(x, dy, m, istd, ga, be, k0, k1, inv_n, hardtanh):
    """bn2d_bwd_apply_k<0>: the unpooled BatchNorm2d backward apply (contracted form)."""
    xh = xh1(x, m, 0, istd)
    g = mask_g(fma(xh, ga, be), dy, hardtanh)
    with np.errstate(invalid="ignore", over="ignore"):
        m0, m1 = f32(k0) * F32(inv_n), f32(k1) * F32(inv_n)
        return (f32(ga) * f32(istd)) * fma(-xh, m1, g - m0)


def dropout_in(x, mask):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(f32(mask) != 0, f32(x) * f32(mask), F32(0)).astype(np.float32)


dropout_out = dropout_in   # dx = dz * mask where kept, else 0


def windows(a):
    """[..., H, W] -> [..., H/2, W/2, 4]: each 2x2 window's elements in (h, w) scan order."""
    a = np.asarray(a)
    H, W = a.shape[-2:]
    v = a.reshape(a.shape[:-2] + (H // 2, 2, W // 2, 2))
    return np.moveaxis(v, -3, -2).reshape(a.shape[:-2] + (H // 2, W // 2, 4))


def unwindows(w):
    """Inverse of windows()."""
    PH, PW = w.shape[-3:-1]
    v = w.reshape(w.shape[:-3] + (PH, PW, 2, 2))
    return np.moveaxis(v, -2, -3).reshape(w.shape[:-3] + (2 * PH, 2 * PW))


def window_argmax(v):
    """bn2_window's scan over [..., 4]: (best, arg)."""
    v = f32(v)
    best = np.full(v.shape[:-1], -np.inf, dtype=np.float32)
    arg = np.zeros(v.shape[:-1], dtype=np.int64)
    for j in range(4):
        vj = v[..., j]
        with np.errstate(invalid="ignore"):
            take = (vj > best) | np.isnan(vj)
        best = np.where(take, vj, best)
        arg = np.where(take, j, arg)
    return best, arg


def pool_forward(x, m, istd, ga, be, hardtanh):
    """x [N, C, H, W], per-channel vectors [C] -> (pooled out, xh windows, y windows, arg)."""
    ch = lambda v: f32(v).reshape(1, -1, 1, 1, 1)   # noqa: E731
    xw = windows(f32(x))
    xh = xh1(xw, ch(m), 0, ch(istd))
    y = fma(xh, ch(ga), ch(be))
    out, arg = window_argmax(clamp(y) if hardtanh else y)
    return out, xh, y, arg


def pool_routed_g(y, arg, gp, hardtanh):
    """The full-resolution masked gradient of the pooled backward, as windows [..., 4]."""
    sel = np.arange(4).reshape((1,) * arg.ndim + (4,)) == arg[..., None]
    with np.errstate(invalid="ignore"):
        ok = sel & ((y > F32(-1)) & (y < F32(1)) if hardtanh else True)
    return np.where(ok, f32(gp)[..., None], F32(0)).astype(np.float32)


def pool_backward(x, gp, m, istd, ga, be, k0, k1, inv_n, hardtanh):
    """bn2_window_dz over every window: dx [N, C, H, W]."""
    ch = lambda v: f32(v).reshape(1, -1, 1, 1, 1)   # noqa: E731
    _, xh, y, arg = pool_forward(x, m, istd, ga, be, hardtanh)
    g = pool_routed_g(y, arg, gp, hardtanh)
    with np.errstate(invalid="ignore", over="ignore"):
        m0, m1 = ch(k0) * F32(inv_n), ch(k1) * F32(inv_n)
        return unwindows((ch(ga) * ch(istd)) * fma(-xh, m1, g - m0))


def split_mean(mean64):
    """The fp32 pair (hi, lo) bn_fwd_final_k stores for a float64 mean."""
    hi = np.asarray(mean64, np.float64).astype(np.float32)
    with np.errstate(invalid="ignore"):
        lo = (np.asarray(mean64, np.float64) - hi.astype(np.float64)).astype(np.float32)
    return hi, lo


def ulp_diff(a, b):
    """|a - b| in fp32 units in the last place (finite, same-sign-or-zero values)."""
    def key(v):
        i = f32(v).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def same_bits(a, b):
    """Bit equality with every NaN equal to every NaN."""
    a, b = f32(a), f32(b)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
