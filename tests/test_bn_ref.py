"""CPU checks of tests/bn_ref.py, the numpy restatement the element-wise BatchNorm GPU tests compare
against: its fma against exact rational arithmetic on constructed fp32 halfway cases (where rounding
the float64 sum a second time gives the wrong answer) and on random operands, and its 2x2 window rule
against torch's CPU max_pool2d on inputs that tie."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import bn_ref as R

F32 = np.float32


def round_f32_exact(q):
    """Round-to-nearest-even of a Fraction to fp32 (normal range), by integer arithmetic."""
    if q == 0:
        return F32(0)
    sign = -1 if q < 0 else 1
    q = abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1                                  # 2^e <= q < 2^(e+1)
    scaled = q / Fraction(2) ** (e - 23)        # in [2^23, 2^24)
    n, rem = divmod(scaled.numerator, scaled.denominator)
    twice = 2 * rem
    if twice > scaled.denominator or (twice == scaled.denominator and n & 1):
        n += 1
    return F32(sign * float(n) * 2.0 ** (e - 23))


def exact_fma(a, b, c):
    return round_f32_exact(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def halfway_cases():
    """a * b + c around the fp32 halfway points above c = 1 + k 2^-23: the product is half an ulp of c
    (2^-24) exactly, or that plus / minus a residue -- 2^-47, 2^-48 (visible to a float64 sum) or
    2^-70 (below it: the float64 sum lands exactly on the halfway point, and rounding it a second time
    goes to even whatever the residue's sign)."""
    h = 2.0 ** -12
    e = 2.0 ** -23
    products = [
        (F32(2.0 ** -24), F32(1.0)),                         # the exact tie: to even
        (F32(2.0 ** -24 * (1 + e)), F32(1.0)),               # 2^-47 above
        (F32(2.0 ** -24 * (1 - e / 2)), F32(1.0)),           # 2^-48 below
        (F32(h * (1 + e)), F32(h * (1 - e))),                # 2^-24 (1 - 2^-46): 2^-70 below
        (F32(h * (1 + e)), F32(h * (1 + e))),                # 2^-24 (1 + 2^-22 + 2^-46): above
        (F32(h * (1 + 2 * e)), F32(h * (1 - 2 * e))),        # 2^-24 (1 - 2^-44): below
    ]
    cases = []
    for k in (0, 1, 2, 3, 1001, 2 ** 22 + 1, 2 ** 23 - 2, 2 ** 23 - 1):
        c = F32(1.0 + k * e)
        for a, b in products:
            cases.append((a, b, c))
            cases.append((a, F32(-float(b)), F32(-float(c))))     # mirrored
            cases.append((F32(-float(a)), b, c))                   # the halfway point below c
    return cases


def test_fma_is_exact_on_halfway_cases():
    cases = halfway_cases()
    a, b, c = (np.array([t[i] for t in cases], dtype=np.float32) for i in range(3))
    got = R.fma(a, b, c)
    want = np.array([exact_fma(*t) for t in cases], dtype=np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the cases do include ones that double rounding gets wrong (else this test proves nothing)
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    assert (naive != want).sum() >= 4


def test_fma_is_exact_on_random_operands():
    rng = np.random.default_rng(0)
    n = 4000
    a = (rng.standard_normal(n) * np.exp(rng.standard_normal(n) * 4)).astype(np.float32)
    b = (rng.standard_normal(n) * np.exp(rng.standard_normal(n) * 4)).astype(np.float32)
    c = (-a.astype(np.float64) * b.astype(np.float64) * (1 + rng.standard_normal(n) * 1e-3)).astype(np.float32)
    c[::3] = rng.standard_normal(len(c[::3])).astype(np.float32)
    got = R.fma(a, b, c)
    want = np.array([exact_fma(*t) for t in zip(a, b, c)], dtype=np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_fma_broadcasts_and_passes_non_finite_values():
    a = np.array([[1.0, np.inf, np.nan, 2.0]], dtype=np.float32)
    got = R.fma(a, F32(3), np.array([[1.0], [2.0]], dtype=np.float32))
    assert got.shape == (2, 4) and got.dtype == np.float32
    assert got[0, 0] == 4 and got[1, 3] == 8 and np.isinf(got[0, 1]) and np.isnan(got[1, 2])


def test_clamp_and_mask_edges():
    one = F32(1)
    below, above = np.nextafter(one, F32(0)), np.nextafter(one, F32(2))
    y = np.array([-above, -one, -below, 0, below, one, above, np.nan], dtype=np.float32)
    assert np.array_equal(R.clamp(y), np.array([-1, -1, -below, 0, below, 1, 1, -1], dtype=np.float32))
    g = R.mask_g(y, F32(5), True)
    assert np.array_equal(g, np.array([0, 0, 5, 5, 5, 0, 0, 0], dtype=np.float32))
    assert np.array_equal(R.mask_g(y, F32(5), False), np.full(8, 5, dtype=np.float32))


def test_windows_round_trip():
    a = np.arange(2 * 3 * 4 * 6, dtype=np.float32).reshape(2, 3, 4, 6)
    w = R.windows(a)
    assert w.shape == (2, 3, 2, 3, 4)
    assert list(w[0, 0, 0, 0]) == [0, 1, 6, 7] and list(w[0, 0, 1, 2]) == [16, 17, 22, 23]
    assert np.array_equal(R.unwindows(w), a)


@pytest.mark.parametrize("seed", [0, 1])
def test_window_rule_matches_torch_max_pool_on_ties(seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(-2, 3, (3, 5, 8, 12)).astype(np.float32)      # 5 values over 4 slots: ties abound
    x[0, 0, :2, :2] = 1.0                                            # an all-equal window
    x[1, 2, 2, 3] = np.nan
    x[1, 3, 4:6, 6:8] = np.nan                                       # several NaNs in one window
    x[2, 0, 0, 0] = -np.inf
    xt = torch.from_numpy(x).requires_grad_(True)
    yt = torch.nn.functional.max_pool2d(xt, 2, 2)
    best, arg = R.window_argmax(R.windows(x))
    assert R.same_bits(best, yt.detach().numpy()).all()
    gp = rng.integers(1, 9, best.shape).astype(np.float32)
    yt.backward(torch.from_numpy(gp))
    routed = R.unwindows(R.pool_routed_g(R.windows(x), arg, gp, False))
    assert np.array_equal(routed, xt.grad.numpy())
    assert (np.sort(R.windows(x), -1)[..., -1] == np.sort(R.windows(x), -1)[..., -2]).mean() > 0.3   # real ties


def test_split_mean_and_ulp_helpers():
    m = np.array([1 / 3, -40.123456789, 0.0, 2.0 ** -30], dtype=np.float64)
    hi, lo = R.split_mean(m)
    assert hi.dtype == lo.dtype == np.float32
    assert np.all(np.abs(hi.astype(np.float64) + lo.astype(np.float64) - m) <= np.abs(m) * 2.0 ** -47)
    one = F32(1)
    assert R.ulp_diff(one, np.nextafter(one, F32(2))) == 1
    assert R.ulp_diff(F32(0), np.nextafter(F32(0), F32(-1))) == 1
    assert R.ulp_diff(F32(-1), F32(-1)) == 0
