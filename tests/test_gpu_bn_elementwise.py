"""The plain BatchNorm entries (csrc/bnn_bn.hip) element for element, at every reduction schedule of
tests/bn_cases.py (tests/test_bn_plan.py proves on the CPU which schedules those are).

The entries are called through the C ABI, so the statistics the kernels return are in hand, and every
output element is compared with tests/bn_ref.py -- the numpy fp32 restatement of the per-element
functions, one rounding per operation, exact fma -- applied to the same inputs and the GPU's own
returned statistics (save_mean, save_mean_lo, save_invstd; dbeta / dgamma as the k0 / k1 of the
backward apply).  The count of differing elements must be 0; NaNs compare as NaN.

Bars and where they come from ("BatchNorm element-wise tests"):
  * exact-input statistics (x integer in [-40, 40], optionally + a per-column bias that is a multiple
    of 2^-12, so that x and every difference from a chunk's first row are exact in fp32): every fp32
    partial (of differences and their squares) is an exact integer below 2^24 and the merges are double, so
    the batch sum is exact -- save_mean / save_mean_lo equal the fp32 split of float64 sum / M bit for bit
    -- and invstd, running_mean, running_var carry double rounding noise plus one rounding to fp32:
    within 1 fp32 ulp of the float64 values;
  * real-input statistics: hi + lo within M 2^-52 max|x| + 2^-47 |mean| of the float64 mean (two
    recursive double sums of M terms, the GPU's and the reference's, and the fp32 pair's 2^-48
    relative split error), invstd / running statistics per column at rtol 1e-5 (the bar of
    test_gpu_parity.py::test_batchnorm_hardtanh_vs_oracle, there norm-wise);
  * column sums of the backward: integer dy gives integer sums (bit-equal); a one-hot dy gives the
    single term (bit-equal; every other column exactly 0); random dy within 2^-19 sum|term| +
    2^-24 |ref| of the float64 sum of the restated fp32 terms (fp32 partials of at most 32 terms:
    32 2^-24 = 2^-19, then double, then one rounding to fp32).
"""
from fractions import Fraction

import numpy as np
import pytest
import torch

import bn_cases as BC
import bn_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32
EPS = 1e-5
EPS_D = float(F32(EPS))            # the float the entry receives, as the kernels widen it
MOM = 0.1
MOM_D = float(F32(MOM))
MAXIMA = {}                        # measured per-column maxima of (b), printed by the last test


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from bnn_amd import _lib
    _lib.lib()
    return _lib


@pytest.fixture()
def rows_restored(L):
    prev = BC.rows_setting(L.lib())
    yield
    L.lib().bnn_bn2d_set_rows(prev)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def zeros(*shape):
    return torch.zeros(*shape, device="cuda")


def bits_equal(a, b):
    """GPU tensors equal bit for bit."""
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def assert_same(got, want, what):
    bad = int((~R.same_bits(got, want)).sum())
    assert bad == 0, f"{what}: {bad} of {np.asarray(got).size} elements differ from the restatement"


def assert_ulp(got, want64, n, what):
    d = R.ulp_diff(got, np.asarray(want64, np.float64).astype(np.float32))
    assert int(d.max()) <= n, f"{what}: {int(d.max())} ulp from the float64 value (bar {n})"


# ----------------------------------------------------------------------------------- BatchNorm1d runs
def work1(L, M, C):
    return torch.empty(L.lib().bnn_bn_workspace(M, C) + 256, dtype=torch.uint8, device="cuda")


def fwd_train(L, x, ga, be, ht, rm0, rv0, drop=None, want_y=True, twice=True):
    M, C = x.shape
    out = None
    for _ in range(2 if twice else 1):
        o = dict(mean=zeros(C), lo=zeros(C), invstd=zeros(C), rm=rm0.clone(), rv=rv0.clone(),
                 y=torch.empty_like(x) if want_y else None)
        ws = work1(L, M, C)
        if drop is None:
            L.call("bnn_bn_fwd_train", L.ptr(x), M, C, L.ptr(ga), L.ptr(be), L.ptr(o["rm"]), L.ptr(o["rv"]), MOM, EPS,
                   L.ptr(o["mean"]), L.ptr(o["invstd"]), L.ptr(o["lo"]), L.ptr(o["y"]), int(ht), L.ptr(ws), L.stream())
        else:
            L.call("bnn_bn_dropout_fwd_train", L.ptr(x), M, C, L.ptr(ga), L.ptr(be), L.ptr(o["rm"]), L.ptr(o["rv"]),
                   MOM, EPS, L.ptr(o["mean"]), L.ptr(o["invstd"]), L.ptr(o["lo"]), L.ptr(o["y"]), int(ht),
                   float(drop[0]), int(drop[1]), None, L.ptr(ws), L.stream())
        if out is not None:
            for k, v in o.items():
                assert v is None or bits_equal(v, out[k]), f"forward: {k} differs between two runs"
        out = o
    return out


def bwd(L, x, dy, ga, be, mean, invstd, lo, ht, drop=None, evalmode=False, twice=True):
    M, C = x.shape
    out = None
    for _ in range(2 if twice else 1):
        o = dict(dx=torch.empty_like(x), dgamma=zeros(C), dbeta=zeros(C))
        ws = work1(L, M, C)
        tail = (L.ptr(o["dx"]), L.ptr(o["dgamma"]), L.ptr(o["dbeta"]), L.ptr(ws), L.stream())
        if evalmode:
            L.call("bnn_bn_bwd_eval", L.ptr(x), L.ptr(dy), M, C, L.ptr(ga), L.ptr(be), L.ptr(mean), L.ptr(invstd),
                   int(ht), *tail)
        elif drop is None:
            L.call("bnn_bn_bwd", L.ptr(x), L.ptr(dy), M, C, L.ptr(ga), L.ptr(be), L.ptr(mean), L.ptr(invstd),
                   L.ptr(lo), int(ht), *tail)
        else:
            L.call("bnn_bn_dropout_bwd", L.ptr(x), L.ptr(dy), M, C, L.ptr(ga), L.ptr(be), L.ptr(mean), L.ptr(invstd),
                   L.ptr(lo), int(ht), float(drop[0]), int(drop[1]), *tail)
        if out is not None:
            for k, v in o.items():
                assert bits_equal(v, out[k]), f"backward: {k} differs between two runs"
        out = o
    return out


def fwd_eval(L, x, ga, be, rm, rv, ht, eps=EPS):
    M, C = x.shape
    y, ws = torch.empty_like(x), work1(L, M, C)
    L.call("bnn_bn_fwd_eval", L.ptr(x), M, C, L.ptr(ga), L.ptr(be), L.ptr(rm), L.ptr(rv), eps, L.ptr(y), int(ht),
           L.ptr(ws), L.stream())
    y2, ws2 = torch.empty_like(x), work1(L, M, C)
    L.call("bnn_bn_fwd_eval", L.ptr(x), M, C, L.ptr(ga), L.ptr(be), L.ptr(rm), L.ptr(rv), eps, L.ptr(y2), int(ht),
           L.ptr(ws2), L.stream())
    assert bits_equal(y, y2), "eval forward differs between two runs"
    return y, ws[:4 * C].view(torch.float32).clone()       # invstd sits at the start of the workspace


def dropout_mask(L, n, p, seed):
    m = torch.empty(n, device="cuda")
    L.call("bnn_dropout_mask", n, float(p), int(seed), L.ptr(m), L.stream())
    return m


def params(rng, C):
    ga = rng.uniform(0.5, 1.5, C).astype(np.float32)
    ga[::5] *= -1                                          # negative scales too
    be = rng.uniform(-0.2, 0.2, C).astype(np.float32)
    rm0 = rng.standard_normal(C).astype(np.float32)
    rv0 = rng.uniform(0.5, 2.0, C).astype(np.float32)
    return ga, be, rm0, rv0


def exact_x(rng, M, C, bias):
    x = rng.integers(-40, 41, (M, C)).astype(np.float32)
    if bias:
        x += (np.round(rng.standard_normal(C) * 3 * 4096) / 4096).astype(np.float32)      # exact: 19 bits
    return x


def real_x(rng, M, C):
    """test_batchnorm_hardtanh_vs_oracle's recipe, plus a column block offset by 3000 with unit spread."""
    x = (rng.integers(-40, 40, (M, C)) + rng.standard_normal(C) * 3).astype(np.float32)
    blk = slice(C // 2, C // 2 + min(max(4, min(64, C // 4)), C - C // 2))
    x[:, blk] = (3000 + rng.standard_normal((M, blk.stop - blk.start))).astype(np.float32)
    return x, blk


def stats64(x):
    """float64 (mean, biased var, unbiased var) per column, two-pass."""
    xd = np.asarray(x, np.float64)
    n = xd.shape[0]
    mean = xd.sum(0) / n
    m2 = ((xd - mean) ** 2).sum(0)
    return mean, m2 / n, (m2 / (n - 1) if n > 1 else m2 / n)


def running64(r0, new):
    return (1.0 - MOM_D) * np.asarray(r0, np.float64) + MOM_D * new


def check_exact_stats(o, x, rm0, rv0, lo=True):
    mean, var, unb = stats64(x)
    hi_ref, lo_ref = R.split_mean(mean)
    assert np.array_equal(host(o["mean"]).view(np.uint32), hi_ref.view(np.uint32)), "save_mean != fl32(sum / n)"
    if lo:
        assert np.array_equal(host(o["lo"]), lo_ref), "save_mean_lo != fl32(mean - fl32(mean))"
    assert_ulp(host(o["invstd"]), 1.0 / np.sqrt(var + EPS_D), 1, "save_invstd")
    assert_ulp(host(o["rm"]), running64(rm0, mean), 1, "running_mean")
    assert_ulp(host(o["rv"]), running64(rv0, unb), 1, "running_var")


def check_real_stats(o, x, rm0, rv0, key, blk=None):
    mean, var, unb = stats64(x)
    n = x.shape[0]
    got = host(o["mean"]).astype(np.float64) + host(o["lo"]).astype(np.float64)
    bar = n * 2.0 ** -52 * np.abs(x).max(0).astype(np.float64) + 2.0 ** -47 * np.abs(mean)
    err = np.abs(got - mean)
    rel = {"invstd": np.abs(host(o["invstd"]) / (1.0 / np.sqrt(var + EPS_D)) - 1),
           "running_mean": np.abs(host(o["rm"]) - running64(rm0, mean)) / np.maximum(np.abs(running64(rm0, mean)), 1e-1),
           "running_var": np.abs(host(o["rv"]) / running64(rv0, unb) - 1)}
    m = {"mean err / bar": float((err / bar).max())}
    m.update({k: float(v.max()) for k, v in rel.items()})
    if blk is not None:
        m["offset block invstd"] = float(rel["invstd"][blk].max())
    MAXIMA[key] = m
    print(f"[bn stats {key}] " + ", ".join(f"{k} {v:.3g}" for k, v in m.items()))
    assert (err <= bar).all(), f"hi + lo: {float((err / bar).max()):.3g} x the bar"
    np.testing.assert_allclose(host(o["invstd"]), 1.0 / np.sqrt(var + EPS_D), rtol=1e-5, atol=0)
    np.testing.assert_allclose(host(o["rm"]), running64(rm0, mean), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(host(o["rv"]), running64(rv0, unb), rtol=1e-5, atol=1e-6)


def check_sums(got_b, got_g, g, xh, what):
    """Random-dy column sums against the float64 sum of the restated fp32 terms."""
    with np.errstate(invalid="ignore", over="ignore"):
        tg = (g * xh).astype(np.float32).astype(np.float64)
    for got, t in ((got_b, g.astype(np.float64)), (got_g, tg)):
        ref = t.sum(0)
        bar = 2.0 ** -19 * np.abs(t).sum(0) + 2.0 ** -24 * np.abs(ref)
        err = np.abs(got.astype(np.float64) - ref)
        assert (err <= bar).all(), f"{what}: column sum {float((err / np.maximum(bar, 1e-300)).max()):.3g} x the bar"


def one_hot_rows(c):
    """The rows whose gradient the statistics pass must not lose: chunk edges, the short last chunk's
    first row, the batch's last row, a row of a partial 8-row batch."""
    k = 1 if c.R > 2 else 0
    rows = {k * c.chunk, min((k + 1) * c.chunk, c.M) - 1, (c.R - 1) * c.chunk, c.M - 1}
    last = BC.last_rows(c)
    if last % 8:
        rows.add((c.R - 1) * c.chunk + (last // 8) * 8)           # first row of the last, partial batch
    if c.chunk >= 16:
        rows.update({k * c.chunk + 7, k * c.chunk + 8, k * c.chunk + 15, k * c.chunk + 16 if c.chunk > 16 else 0})
    return sorted(r for r in rows if 0 <= r < c.M)


def check_one_hot(L, c, xd, x, ga, be, o, ht):
    M, C = x.shape
    rows = one_hot_rows(c)
    K = len(rows)
    dy = np.zeros((M, C), np.float32)
    cols = np.arange(C)
    gval = (1.0 + (cols % 7) * 0.37).astype(np.float32) * np.where(cols % 2, -1, 1).astype(np.float32)
    hot = cols % (2 * K) < K                                        # the other columns stay all-zero
    r_of = np.array(rows)[cols % (2 * K) % K]
    dy[r_of[hot], cols[hot]] = gval[hot]
    b = bwd(L, xd, dev(dy), dev(ga), dev(be), o["mean"], o["invstd"], o["lo"], ht, twice=False)
    mean, lo, istd = host(o["mean"]), host(o["lo"]), host(o["invstd"])
    xr = x[r_of, cols]
    xh = R.xh1(xr, mean, lo, istd)
    g = np.where(hot, R.mask_g(R.fma(xh, ga, be), gval, ht), F32(0)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        want_g = np.where(hot, (g * xh).astype(np.float32), F32(0))
    assert np.array_equal(host(b["dbeta"]), g), "one-hot dy: dbeta is not the single masked term"
    assert np.array_equal(host(b["dgamma"]), want_g), "one-hot dy: dgamma is not fl32(g * xhat)"
    assert (host(b["dbeta"])[~hot] == 0).all() and (host(b["dgamma"])[~hot] == 0).all()
    assert (g[hot] != 0).sum() >= K                                 # the mask left something to see


def run_case_1d(L, c, kind):
    rng = np.random.default_rng(c.M * 131 + c.C + (kind == "real"))
    M, C = c.M, c.C
    ga, be, rm0, rv0 = params(rng, C)
    blk = None
    if kind == "real":
        x, blk = real_x(rng, M, C)
        ht = 1
        dy = rng.standard_normal((M, C)).astype(np.float32)
    else:
        x = exact_x(rng, M, C, bias=(kind == "exact+bias"))
        ht = 0
        dy = rng.integers(-8, 9, (M, C)).astype(np.float32)
    xd, dyd, gad, bed = dev(x), dev(dy), dev(ga), dev(be)
    o = fwd_train(L, xd, gad, bed, ht, dev(rm0), dev(rv0))
    if kind == "real":
        check_real_stats(o, x, rm0, rv0, f"{M}x{C}", blk)
    else:
        check_exact_stats(o, x, rm0, rv0)
    mean, lo, istd = host(o["mean"]), host(o["lo"]), host(o["invstd"])
    assert_same(host(o["y"]), R.forward(x, mean, lo, istd, ga, be, ht), "train y")
    b = bwd(L, xd, dyd, gad, bed, o["mean"], o["invstd"], o["lo"], ht)
    k0, k1 = host(b["dbeta"]), host(b["dgamma"])
    assert_same(host(b["dx"]), R.dz1(x, dy, mean, lo, istd, ga, be, k0, k1, R.inv_n_1d(M), ht), "train dx")
    xh = R.xh1(x, mean, lo, istd)
    g = np.ascontiguousarray(R.mask_g(R.fma(xh, ga, be), dy, ht))
    if kind == "real":
        check_sums(k0, k1, g, xh, "train")
    else:
        assert np.array_equal(k0, dy.astype(np.float64).sum(0).astype(np.float32)), "integer dy: dbeta is not the sum"
        check_sums(k0, k1, g, xh, "train")
    check_one_hot(L, c, xd, x, ga, be, o, 1)
    del xh, g
    # eval mode, on the running statistics the train call left
    ye, ie = fwd_eval(L, xd, gad, bed, o["rm"], o["rv"], ht)
    rm, rv, ie_h = host(o["rm"]), host(o["rv"]), host(ie)
    assert_ulp(ie_h, 1.0 / np.sqrt(rv.astype(np.float64) + EPS_D), 1, "eval invstd")
    assert_same(host(ye), R.forward(x, rm, 0, ie_h, ga, be, ht), "eval y")
    be_ = bwd(L, xd, dyd, gad, bed, o["rm"], ie, None, ht, evalmode=True)
    assert_same(host(be_["dx"]), R.dz1(x, dy, rm, 0, ie_h, ga, be, host(be_["dbeta"]), host(be_["dgamma"]), 0.0, ht),
                "eval dx")
    xh = R.xh1(x, rm, 0, ie_h)
    check_sums(host(be_["dbeta"]), host(be_["dgamma"]), np.ascontiguousarray(R.mask_g(R.fma(xh, ga, be), dy, ht)), xh,
               "eval")


# the cases of 8 M and 17 M elements take the biased exact variant as their only exact one (time)
CASE_KINDS_1D = [(c, k) for c in BC.SMALL_1D for k in ("exact", "exact+bias", "real")
                 if k != "exact" or c.M * c.C <= (5 << 20)]


@pytest.mark.parametrize("case,kind", CASE_KINDS_1D, ids=[f"{BC.id_1d(c)}-{k}" for c, k in CASE_KINDS_1D])
def test_bn1d_case(L, case, kind):
    """fwd_train, bwd, fwd_eval and bwd_eval of one schedule: statistics (a) / (b), every element of y
    and dx (c), the column sums under integer, random and one-hot gradients (d), two runs identical."""
    run_case_1d(L, case, kind)


@pytest.mark.parametrize("case", BC.DROPOUT_1D, ids=BC.id_1d)
def test_bn1d_dropout_case(L, case):
    """bnn_bn_dropout_fwd_train / bnn_bn_dropout_bwd with p = 0.3 at the 16- and 32-row schedules, with
    the mask bnn_dropout_mask returns."""
    rng = np.random.default_rng(case.M + case.C)
    M, C, p, seed = case.M, case.C, 0.3, 20240607
    ga, be, rm0, rv0 = params(rng, C)
    x, _ = real_x(rng, M, C)
    dy = rng.standard_normal((M, C)).astype(np.float32)
    xd, dyd, gad, bed = dev(x), dev(dy), dev(ga), dev(be)
    mask = host(dropout_mask(L, M * C, p, seed)).reshape(M, C)
    keep = float((mask != 0).mean())
    assert abs(keep - 0.7) < 0.01 and set(np.unique(mask)) == {F32(0), F32(1) / (F32(1) - F32(p))}
    xs = R.dropout_in(x, mask)
    o = fwd_train(L, xd, gad, bed, 1, dev(rm0), dev(rv0), drop=(p, seed))
    check_real_stats(o, xs, rm0, rv0, f"{M}x{C} dropout")
    mean, lo, istd = host(o["mean"]), host(o["lo"]), host(o["invstd"])
    assert_same(host(o["y"]), R.forward(xs, mean, lo, istd, ga, be, 1), "dropout y")
    b = bwd(L, xd, dyd, gad, bed, o["mean"], o["invstd"], o["lo"], 1, drop=(p, seed))
    k0, k1 = host(b["dbeta"]), host(b["dgamma"])
    dz = R.dz1(xs, dy, mean, lo, istd, ga, be, k0, k1, R.inv_n_1d(M), 1)
    assert_same(host(b["dx"]), R.dropout_out(dz, mask), "dropout dx")
    xh = R.xh1(xs, mean, lo, istd)
    check_sums(k0, k1, np.ascontiguousarray(R.mask_g(R.fma(xh, ga, be), dy, 1)), xh, "dropout")


# ------------------------------------------------------------------ the 8205 x 8192 case, on the GPU
def t_fma(a, b, c):
    """bn_ref.fma on GPU tensors (same construction: exact product, TwoSum, round to odd)."""
    a, b, c = a.double(), b.double(), c.double()
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    fix = torch.isfinite(s) & torch.isfinite(err) & (err != 0)
    bits = s.contiguous().view(torch.int64)
    step = torch.where((err > 0) == (bits >= 0), 1, -1)
    bits = bits + torch.where(fix & ((bits & 1) == 0), step, torch.zeros_like(step))
    return bits.view(torch.float64).float()


def t_forward(x, m, lo, istd, ga, be, ht):
    y = t_fma(((x - m) - lo) * istd, ga, be)
    return torch.where(torch.isnan(y), torch.full_like(y, -1), y.clamp(-1, 1)) if ht else y


def t_dz1(x, dy, m, lo, istd, ga, be, k0, k1, inv_n, ht):
    xh = ((x - m) - lo) * istd
    y = t_fma(xh, ga, be)
    g = torch.where((y > -1) & (y < 1), dy, torch.zeros_like(dy)) if ht else dy
    return (ga * istd) * ((g - k0 * inv_n) - xh * (k1 * inv_n))


def t_same(a, b):
    return int((~((a.view(torch.int32) == b.view(torch.int32)) | (torch.isnan(a) & torch.isnan(b)))).sum())


def test_bn1d_large_case(L):
    """The 256-row schedule at [8205, 8192] (33 chunks, the last of 13 rows; 32-row apply blocks, the last
    of 13), once per pass.  Its float64 statistics and its restatement are taken with torch on the GPU
    in slabs of rows (as oracle/bnn_t64.py does at the bench size); the torch restatement is the one of
    bn_ref, which is checked here against bn_ref itself on the first and last rows."""
    c = BC.LARGE_1D
    M, C, ht = c.M, c.C, 1
    rng = np.random.default_rng(5)
    ga, be, rm0, rv0 = params(rng, C)
    g = torch.Generator(device="cuda").manual_seed(8205)
    xd = torch.randint(-40, 40, (M, C), generator=g, device="cuda").float() + dev((rng.standard_normal(C) * 3).astype(np.float32))
    xd[:, 4096:4160] = 3000 + torch.randn(M, 64, generator=g, device="cuda")
    dyd = torch.randn(M, C, generator=g, device="cuda")
    gad, bed = dev(ga), dev(be)
    o = fwd_train(L, xd, gad, bed, ht, dev(rm0), dev(rv0), twice=False)
    # (b) statistics against float64 on the GPU
    mean = torch.zeros(C, dtype=torch.float64, device="cuda")
    for r in range(0, M, 1024):
        mean += xd[r:r + 1024].double().sum(0)
    mean /= M
    m2 = torch.zeros_like(mean)
    for r in range(0, M, 1024):
        m2 += ((xd[r:r + 1024].double() - mean) ** 2).sum(0)
    mean_h, var_h, unb_h = host(mean), host(m2) / M, host(m2) / (M - 1)
    got = host(o["mean"]).astype(np.float64) + host(o["lo"]).astype(np.float64)
    bar = M * 2.0 ** -52 * host(xd.abs().amax(0)).astype(np.float64) + 2.0 ** -47 * np.abs(mean_h)
    err = np.abs(got - mean_h)
    inv_rel = np.abs(host(o["invstd"]) * np.sqrt(var_h + EPS_D) - 1)
    MAXIMA[f"{M}x{C}"] = {"mean err / bar": float((err / bar).max()), "invstd": float(inv_rel.max()),
                          "offset block invstd": float(inv_rel[4096:4160].max())}
    print(f"[bn stats {M}x{C}] {MAXIMA[f'{M}x{C}']}")
    assert (err <= bar).all()
    np.testing.assert_allclose(host(o["invstd"]), 1.0 / np.sqrt(var_h + EPS_D), rtol=1e-5, atol=0)
    np.testing.assert_allclose(host(o["rm"]), running64(rm0, mean_h), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(host(o["rv"]), running64(rv0, unb_h), rtol=1e-5, atol=1e-6)
    # (c) every element, in slabs
    b = bwd(L, xd, dyd, gad, bed, o["mean"], o["invstd"], o["lo"], ht, twice=False)
    ye, ie = fwd_eval(L, xd, gad, bed, o["rm"], o["rv"], ht)
    assert_ulp(host(ie), 1.0 / np.sqrt(host(o["rv"]).astype(np.float64) + EPS_D), 1, "eval invstd")
    be_ = bwd(L, xd, dyd, gad, bed, o["rm"], ie, None, ht, evalmode=True, twice=False)
    inv_n = float(R.inv_n_1d(M))
    zero = torch.zeros(C, device="cuda")
    bad = dict(y=0, dx=0, ye=0, dxe=0)
    sb = torch.zeros(C, dtype=torch.float64, device="cuda")
    sg, ab, ag = torch.zeros_like(sb), torch.zeros_like(sb), torch.zeros_like(sb)
    for r in range(0, M, 1024):
        s = slice(r, r + 1024)
        x, dy = xd[s], dyd[s]
        bad["y"] += t_same(o["y"][s], t_forward(x, o["mean"], o["lo"], o["invstd"], gad, bed, ht))
        bad["dx"] += t_same(b["dx"][s], t_dz1(x, dy, o["mean"], o["lo"], o["invstd"], gad, bed, b["dbeta"], b["dgamma"],
                                            inv_n, ht))
        bad["ye"] += t_same(ye[s], t_forward(x, o["rm"], zero, ie, gad, bed, ht))
        bad["dxe"] += t_same(be_["dx"][s], t_dz1(x, dy, o["rm"], zero, ie, gad, bed, be_["dbeta"], be_["dgamma"], 0.0, ht))
        xh = ((x - o["mean"]) - o["lo"]) * o["invstd"]
        yv = t_fma(xh, gad, bed)
        gm = torch.where((yv > -1) & (yv < 1), dy, torch.zeros_like(dy))
        t = (gm * xh).double()
        sb += gm.double().sum(0)
        ab += gm.double().abs().sum(0)
        sg += t.sum(0)
        ag += t.abs().sum(0)
    assert bad == dict(y=0, dx=0, ye=0, dxe=0), bad
    for got_t, ref, ab_ in ((b["dbeta"], sb, ab), (b["dgamma"], sg, ag)):     # (d), random dy
        e = (got_t.double() - ref).abs()
        assert bool((e <= 2.0 ** -19 * ab_ + 2.0 ** -24 * ref.abs()).all())
    # the torch restatement is bn_ref's: the first and the last rows through both
    for s in (slice(0, 40), slice(M - 40, M)):
        x, dy = host(xd[s]), host(dyd[s])
        mean_, lo_, is_ = host(o["mean"]), host(o["lo"]), host(o["invstd"])
        assert_same(host(o["y"][s]), R.forward(x, mean_, lo_, is_, ga, be, ht), "train y (bn_ref)")
        assert_same(host(b["dx"][s]), R.dz1(x, dy, mean_, lo_, is_, ga, be, host(b["dbeta"]), host(b["dgamma"]),
                                            R.inv_n_1d(M), ht), "train dx (bn_ref)")
        assert_same(host(t_fma(xd[s], gad, dyd[s])), R.fma(x, ga, dy), "t_fma vs bn_ref.fma")


# ----------------------------------------------------------------------------------- BatchNorm2d runs
def work2(L, N, C):
    return torch.empty(L.lib().bnn_bn2d_workspace(N, C) + 256, dtype=torch.uint8, device="cuda")


def out_shape(x, pool):
    N, C, H, W = x.shape
    return (N, C, H // 2, W // 2) if pool else (N, C, H, W)


def fwd2_train(L, x, ga, be, ht, pool, rm0, rv0, q=None):
    """q = (xq tensor, xbias tensor, xfmt): the compact-input entry on the same values."""
    N, C, H, W = x.shape
    out = None
    for _ in range(2):
        o = dict(mean=zeros(C), invstd=zeros(C), rm=rm0.clone(), rv=rv0.clone(),
                 y=torch.empty(out_shape(x, pool), device="cuda"))
        ws = work2(L, N, C)
        tail = (N, C, H, W, L.ptr(ga), L.ptr(be), L.ptr(o["rm"]), L.ptr(o["rv"]), MOM, EPS, L.ptr(o["mean"]),
                L.ptr(o["invstd"]), L.ptr(o["y"]), int(ht), int(pool), L.ptr(ws), L.stream())
        if q is None:
            L.call("bnn_bn2d_fwd_train", L.ptr(x), *tail)
        else:
            L.call("bnn_bn2d_fwd_train_q", L.ptr(q[0]), L.ptr(q[1]), q[2], *tail)
        if out is not None:
            for k, v in o.items():
                assert bits_equal(v, out[k]), f"2d forward: {k} differs between two runs"
        out = o
    return out


def bwd2(L, x, dy, ga, be, mean, invstd, ht, pool, evalmode=False, q=None):
    N, C, H, W = x.shape
    out = None
    for _ in range(2):
        o = dict(dx=torch.empty_like(x), dgamma=zeros(C), dbeta=zeros(C))
        ws = work2(L, N, C)
        tail = (L.ptr(dy), N, C, H, W, L.ptr(ga), L.ptr(be), L.ptr(mean), L.ptr(invstd), int(ht), int(pool),
                L.ptr(o["dx"]), L.ptr(o["dgamma"]), L.ptr(o["dbeta"]), L.ptr(ws), L.stream())
        if q is not None:
            L.call("bnn_bn2d_bwd_q", L.ptr(q[0]), L.ptr(q[1]), q[2], *tail)
        else:
            L.call("bnn_bn2d_bwd_eval" if evalmode else "bnn_bn2d_bwd", L.ptr(x), *tail)
        if out is not None:
            for k, v in o.items():
                assert bits_equal(v, out[k]), f"2d backward: {k} differs between two runs"
        out = o
    return out


def fwd2_eval(L, x, ga, be, rm, rv, ht, pool, eps=EPS):
    N, C, H, W = x.shape
    y, ws = torch.empty(out_shape(x, pool), device="cuda"), work2(L, N, C)
    L.call("bnn_bn2d_fwd_eval", L.ptr(x), N, C, H, W, L.ptr(ga), L.ptr(be), L.ptr(rm), L.ptr(rv), eps, L.ptr(y),
           int(ht), int(pool), L.ptr(ws), L.stream())
    return y, ws[:4 * C].view(torch.float32).clone()


def ch(v):
    return np.asarray(v, np.float32).reshape(1, -1, 1, 1)


def ref2_forward(x, m, istd, ga, be, ht, pool):
    if pool:
        return R.pool_forward(x, m, istd, ga, be, ht)[0]
    return R.forward(x, ch(m), 0, ch(istd), ch(ga), ch(be), ht)


def ref2_backward(x, dy, m, istd, ga, be, k0, k1, inv_n, ht, pool):
    if pool:
        return R.pool_backward(x, dy, m, istd, ga, be, k0, k1, inv_n, ht)
    return R.dz2_flat(x, dy, ch(m), ch(istd), ch(ga), ch(be), ch(k0), ch(k1), inv_n, ht)


def ref2_terms(x, dy, m, istd, ga, be, ht, pool):
    """The statistics pass's fp32 terms (g, xhat) per channel: [C, terms]."""
    C = x.shape[1]
    if pool:
        _, xh, y, arg = R.pool_forward(x, m, istd, ga, be, ht)
        g = R.pool_routed_g(y, arg, dy, ht)
    else:
        xh = R.xh1(x, ch(m), 0, ch(istd))
        g = np.ascontiguousarray(R.mask_g(R.fma(xh, ch(ga), ch(be)), dy, ht))
    return np.moveaxis(g, 1, 0).reshape(C, -1).T, np.moveaxis(xh, 1, 0).reshape(C, -1).T


def run_case_2d(L, c, pool, kind, rows, ht):
    N, C, H, W = c.N, c.C, c.H, c.W
    rng = np.random.default_rng(N * C + H + pool + 7 * ht)
    ga, be, rm0, rv0 = params(rng, C)
    if kind == "exact":
        x = rng.integers(-40, 41, (N, C, H, W)).astype(np.float32)
        x += ch(np.round(rng.standard_normal(C) * 3 * 4096) / 4096) * (C % 2 == 0)
        if ht:
            x = rng.integers(-3, 4, (N, C, H, W)).astype(np.float32)     # ties inside and at the clamp
        dy = rng.integers(-8, 9, out_shape(x, pool)).astype(np.float32)
    else:
        x = (rng.standard_normal((N, C, H, W)) * 2 + rng.standard_normal((1, C, 1, 1))).astype(np.float32)
        dy = rng.standard_normal(out_shape(x, pool)).astype(np.float32)
    xd, dyd, gad, bed = dev(x), dev(dy), dev(ga), dev(be)
    o = fwd2_train(L, xd, gad, bed, ht, pool, dev(rm0), dev(rv0))
    xc = np.moveaxis(x, 1, 0).reshape(C, -1).T                       # [N H W, C]
    tag = f"{BC.id_2d(c)} pool{pool} rows{rows} ht{ht} {kind}"
    if kind == "exact":
        check_exact_stats(o, xc, rm0, rv0, lo=False)
    else:
        mean, var, unb = stats64(xc)
        np.testing.assert_allclose(host(o["mean"]), mean, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(host(o["invstd"]), 1.0 / np.sqrt(var + EPS_D), rtol=1e-5, atol=0)
        np.testing.assert_allclose(host(o["rm"]), running64(rm0, mean), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(host(o["rv"]), running64(rv0, unb), rtol=1e-5, atol=1e-6)
    mean, istd = host(o["mean"]), host(o["invstd"])
    assert_same(host(o["y"]), ref2_forward(x, mean, istd, ga, be, ht, pool), f"{tag}: train y")
    if pool and kind == "exact":
        w = np.sort(R.windows(R.forward(x, ch(mean), 0, ch(istd), ch(ga), ch(be), ht)), -1)
        assert (w[..., 3] == w[..., 2]).mean() > 0.02, "the input was meant to tie"
    b = bwd2(L, xd, dyd, gad, bed, o["mean"], o["invstd"], ht, pool)
    k0, k1 = host(b["dbeta"]), host(b["dgamma"])
    inv_n = R.inv_n_2d(N, H, W)
    assert_same(host(b["dx"]), ref2_backward(x, dy, mean, istd, ga, be, k0, k1, inv_n, ht, pool), f"{tag}: train dx")
    g, xh = ref2_terms(x, dy, mean, istd, ga, be, ht, pool)
    check_sums(k0, k1, g, xh, tag)
    if kind == "exact" and not ht:
        assert np.array_equal(k0, np.moveaxis(dy, 1, 0).reshape(C, -1).astype(np.float64).sum(1).astype(np.float32))
    # eval
    ye, ie = fwd2_eval(L, xd, gad, bed, o["rm"], o["rv"], ht, pool)
    rm, ie_h = host(o["rm"]), host(ie)
    assert_ulp(ie_h, 1.0 / np.sqrt(host(o["rv"]).astype(np.float64) + EPS_D), 1, "2d eval invstd")
    assert_same(host(ye), ref2_forward(x, rm, ie_h, ga, be, ht, pool), f"{tag}: eval y")
    e = bwd2(L, xd, dyd, gad, bed, o["rm"], ie, ht, pool, evalmode=True)
    assert_same(host(e["dx"]), ref2_backward(x, dy, rm, ie_h, ga, be, host(e["dbeta"]), host(e["dgamma"]), 0.0, ht, pool),
                f"{tag}: eval dx")
    return o, b


@pytest.mark.parametrize("pool", [0, 2])
@pytest.mark.parametrize("case", BC.CASES_2D, ids=BC.id_2d)
def test_bn2d_case(L, rows_restored, case, pool):
    """Every BatchNorm2d case under bnn_bn2d_set_rows 0, 1 and 2, Hardtanh off and on, with an
    integer-valued input (exact statistics; real ties off the clamp, saturated ties on it) and a
    tie-free real one: statistics, every element of y and dx (train and eval), the column sums."""
    for rows in (0, 1, 2):
        L.call("bnn_bn2d_set_rows", rows)
        assert BC.plan_2d(L.lib(), case.N, case.C, case.H, case.W, pool) == case.plans[(rows, pool)]
        for ht in (0, 1):
            for kind in ("exact", "real"):
                run_case_2d(L, case, pool, kind, rows, ht)


@pytest.mark.parametrize("pool", [0, 2])
@pytest.mark.parametrize("case", BC.CASES_2D, ids=BC.id_2d)
def test_bn2d_one_hot(L, rows_restored, case, pool):
    """A one-hot gradient at the first and last image of a chunk and the first and last (pooled) row:
    dbeta is the masked g, dgamma fl32(g * xhat), every other channel exactly 0."""
    N, C, H, W = case.N, case.C, case.H, case.W
    CR, Rn = case.plans[(1, pool)][:2]
    rng = np.random.default_rng(N + C + H)
    ga, be, rm0, rv0 = params(rng, C)
    ga = (np.sign(ga) * F32(0.4)).astype(np.float32)               # |y| < 1 for most elements: the mask passes them
    x = (rng.standard_normal((N, C, H, W)) * 0.7 + rng.standard_normal((1, C, 1, 1))).astype(np.float32)
    xd, gad, bed = dev(x), dev(ga), dev(be)
    oh, ow = out_shape(x, pool)[2:]
    images = sorted({0, CR - 1, (Rn - 1) * CR, N - 1})
    spots = [(n, r, w) for n in images for r, w in ((0, 0), (oh - 1, ow - 1), (0, ow - 1), (oh - 1, 0))]
    K = len(spots)
    for rows in (0, 1, 2):
        L.call("bnn_bn2d_set_rows", rows)
        o = fwd2_train(L, xd, gad, bed, 1, pool, dev(rm0), dev(rv0))
        mean, istd = host(o["mean"]), host(o["invstd"])
        dy = np.zeros(out_shape(x, pool), np.float32)
        cols = np.arange(C)
        hot = cols % (2 * K) < K if C >= 2 * K else cols < max(1, C // 2)
        gval = (1.0 + (cols % 7) * 0.37).astype(np.float32) * np.where(cols % 2, -1, 1).astype(np.float32)
        for cc in cols[hot]:
            n, r, w = spots[cc % K]
            dy[n, cc, r, w] = gval[cc]
        b = bwd2(L, xd, dev(dy), gad, bed, o["mean"], o["invstd"], 1, pool)
        g, xh = ref2_terms(x, dy, mean, istd, ga, be, 1, pool)        # [terms, C]: one non-zero per hot channel
        with np.errstate(invalid="ignore"):
            t = (g * xh).astype(np.float32)
        assert ((g != 0).sum(0) <= 1).all()
        want_b = g.astype(np.float64).sum(0).astype(np.float32)       # a single term: exact
        want_g = t.astype(np.float64).sum(0).astype(np.float32)
        assert np.array_equal(host(b["dbeta"]), want_b), f"rows {rows}: dbeta"
        assert np.array_equal(host(b["dgamma"]), want_g), f"rows {rows}: dgamma"
        assert (host(b["dbeta"])[~hot] == 0).all() and (host(b["dgamma"])[~hot] == 0).all()
        assert (want_b != 0).sum() >= max(1, hot.sum() // 2)            # the Hardtanh mask left terms to see


# ------------------------------------------------------------------------------------------ (e) edges
def exact_signs(x):
    """sign(x - mean) per element of [M, C] in exact rational arithmetic."""
    out = np.zeros(x.shape, np.int64)
    for c in range(x.shape[1]):
        col = [Fraction(float(v)) for v in x[:, c]]
        mean = sum(col) / len(col)
        out[:, c] = [(v > mean) - (v < mean) for v in col]
    return out


@pytest.mark.parametrize("M", [3, 4, 37, 259])
def test_near_tie_columns_get_the_sign_of_the_exact_difference(L, M):
    """Columns whose values sit within an ulp of their mean ({a, a, a + ulp(a)} and its kin, at several
    magnitudes, integer + bias included): with gamma = 1, beta = 0 the sign of y is the sign of the
    exact rational x - mean for every element (the hi / lo mean pair's purpose)."""
    mags = [1.0, 3.0, 40.5, 1000.25, 0.125, 12345.678, 17 + 0.3712, -23 + 0.3712, 2.0 ** 20 + 1, -7.0, 1e-3, 65504.0]
    cols = []
    for a in mags:
        a = F32(a)
        up, dn = np.nextafter(a, F32(np.inf)), np.nextafter(a, F32(-np.inf))
        for pat in ((a, a, up), (up, a, a), (a, up, up), (a, a, dn), (dn, a, up), (a, up, a)):
            col = np.full(M, a, np.float32)
            col[:3] = pat
            if M > 3:
                col[3::2] = pat[2]                                  # half of the rest at the neighbour
                col[M - 1] = pat[1]
            cols.append(col)
    x = np.stack(cols, 1)
    assert x.shape[1] % 4 == 0
    C = x.shape[1]
    o = fwd_train(L, dev(x), None, None, 0, zeros(C), torch.ones(C, device="cuda"))
    want = exact_signs(x)
    got = np.sign(host(o["y"])).astype(np.int64)
    assert (want != 0).mean() > 0.9
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{len(bad)} signs differ from the exact x - mean, first at (row, col) {bad[:4].tolist()}"
    # and the restatement agrees on this input too
    assert_same(host(o["y"]), R.forward(x, host(o["mean"]), host(o["lo"]), host(o["invstd"]), 1, 0, 0), "near-tie y")


def test_strict_hardtanh_mask_and_clamp_at_plus_minus_one(L):
    """mean 0, invstd 1, gamma 1, beta 0: y = x.  The eval backward passes g strictly inside (-1, 1) and
    exactly 0 at and beyond +-1; the eval forward clamps exactly."""
    one = F32(1)
    below, above = np.nextafter(one, F32(0)), np.nextafter(one, F32(2))
    vals = np.array([-above, -one, -below, below, one, above, 0.0, -0.0], np.float32)
    x = np.tile(vals[:, None], (1, 8))
    M, C = x.shape
    g = np.arange(1, M * C + 1, dtype=np.float32).reshape(M, C) * F32(0.25)
    mean, rv, ones = zeros(C), torch.ones(C, device="cuda"), torch.ones(C, device="cuda")
    b = bwd(L, dev(x), dev(g), ones, zeros(C), mean, ones, None, 1, evalmode=True)
    inside = (np.abs(x) < 1)
    assert np.array_equal(host(b["dx"]), np.where(inside, g, F32(0)))
    assert np.array_equal(host(b["dbeta"]), np.where(inside, g, F32(0)).sum(0))
    y, ie = fwd_eval(L, dev(x), ones, zeros(C), mean, rv, 1, eps=0.0)
    assert np.array_equal(host(ie), np.ones(C, np.float32))
    assert_same(host(y), R.forward(x, 0, 0, 1, 1, 0, 1), "clamp")
    assert np.array_equal(host(y), np.clip(x, -1, 1))               # by value (y = fma(-0, 1, +0) is +0)
    assert host(y)[2, 0] == -below and host(y)[3, 0] == below and host(y)[0, 0] == -1 and host(y)[5, 0] == 1


@pytest.mark.parametrize("M,C", [(300, 64), (1021, 2048), (2059, 512)])
def test_constant_and_zero_columns(L, M, C):
    """var < 0 -> 0 and xhat = 0: a constant column and an all-zero column get invstd = fl(1 / sqrt(eps)),
    y = beta exactly and dgamma = 0."""
    rng = np.random.default_rng(M)
    ga, be, rm0, rv0 = params(rng, C)
    x = rng.standard_normal((M, C)).astype(np.float32)
    x[:, 0], x[:, 5], x[:, C - 1], x[:, 17] = 0.0, 3.25, -40.0, 1e-3
    const = [0, 5, C - 1, 17]
    o = fwd_train(L, dev(x), dev(ga), dev(be), 0, dev(rm0), dev(rv0))
    want = F32(1.0 / np.sqrt(EPS_D))
    assert (host(o["invstd"])[const] == want).all()
    assert np.array_equal(host(o["mean"])[const], x[0, const]) and (host(o["lo"])[const] == 0).all()
    assert np.array_equal(host(o["y"])[:, const], np.tile(be[const], (M, 1)))
    dy = rng.standard_normal((M, C)).astype(np.float32)
    b = bwd(L, dev(x), dev(dy), dev(ga), dev(be), o["mean"], o["invstd"], o["lo"], 0)
    assert (host(b["dgamma"])[const] == 0).all()
    assert_ulp(host(o["rv"])[const], running64(rv0, 0.0)[const], 1, "running_var of a constant column")


def test_single_row_batch_uses_the_biased_variance(L):
    """M = 1: n > 1 ? m2 / (n - 1) : var -- the running variance moves towards 0, not towards inf / NaN."""
    C = 8
    rng = np.random.default_rng(1)
    ga, be, rm0, rv0 = params(rng, C)
    x = rng.standard_normal((1, C)).astype(np.float32)
    o = fwd_train(L, dev(x), dev(ga), dev(be), 0, dev(rm0), dev(rv0))
    assert np.array_equal(host(o["mean"]), x[0]) and (host(o["lo"]) == 0).all()
    assert (host(o["invstd"]) == F32(1.0 / np.sqrt(EPS_D))).all()
    assert_ulp(host(o["rv"]), running64(rv0, 0.0), 1, "running_var at M = 1")
    assert_ulp(host(o["rm"]), running64(rm0, x[0].astype(np.float64)), 1, "running_mean at M = 1")
    assert np.array_equal(host(o["y"])[0], be)


@pytest.mark.parametrize("M,C", [(131, 1028), (1021, 2048)])
def test_nan_and_inf_stay_in_their_columns(L, M, C):
    """One NaN and one Inf, each in a single column: every other column's statistics, y and dx are
    bit-identical to a run without them; the poisoned columns are non-finite."""
    rng = np.random.default_rng(C)
    ga, be, rm0, rv0 = params(rng, C)
    x, _ = real_x(rng, M, C)
    dy = rng.standard_normal((M, C)).astype(np.float32)
    xp = x.copy()
    cn, ci = 6, C - 3
    xp[M // 2, cn], xp[M - 1, ci] = np.nan, np.inf
    clean = np.ones(C, bool)
    clean[[cn, ci]] = False
    outs = []
    for xx in (x, xp):
        o = fwd_train(L, dev(xx), dev(ga), dev(be), 0, dev(rm0), dev(rv0))
        b = bwd(L, dev(xx), dev(dy), dev(ga), dev(be), o["mean"], o["invstd"], o["lo"], 0)
        outs.append({k: host(v) for k, v in {**o, **b}.items()})
    a, p = outs
    for k in a:
        assert np.array_equal(a[k][..., clean].view(np.uint32), p[k][..., clean].view(np.uint32)), k
    for k in ("mean", "rm", "rv", "dgamma"):
        assert not np.isfinite(p[k][[cn, ci]]).any(), k
    assert not np.isfinite(p["y"][:, [cn, ci]]).any() and not np.isfinite(p["dx"][:, [cn, ci]]).any()


@pytest.mark.parametrize("rows", [0, 1, 2])
def test_nan_wins_the_pooling_window(L, rows_restored, rows):
    """Eval-mode BatchNorm2d with pool (the statistics are inputs, so a NaN stays in its window): the
    window's output is NaN, the gradient goes to the (last) NaN, every other window is unchanged."""
    L.call("bnn_bn2d_set_rows", rows)
    N, C, H, W = 3, 8, 28, 28
    rng = np.random.default_rng(3)
    ga, be, rm, rv = params(rng, C)
    x = rng.integers(-3, 4, (N, C, H, W)).astype(np.float32)
    xp = x.copy()
    xp[1, 2, 5, 7] = np.nan                       # window (2, 3), slot 3
    xp[2, 7, 26, 0], xp[2, 7, 27, 1] = np.nan, np.nan   # window (13, 0): slots 0 and 3 -> the last wins
    dy = rng.integers(1, 9, (N, C, H // 2, W // 2)).astype(np.float32)
    ys = []
    for xx in (x, xp):
        y, ie = fwd2_eval(L, dev(xx), dev(ga), dev(be), dev(rm), dev(rv), 0, 2)
        e = bwd2(L, dev(xx), dev(dy), dev(ga), dev(be), dev(rm), ie, 0, 2, evalmode=True)
        ie_h = host(ie)
        assert_same(host(y), ref2_forward(xx, rm, ie_h, ga, be, 0, 2), "eval pooled y")
        assert_same(host(e["dx"]), ref2_backward(xx, dy, rm, ie_h, ga, be, host(e["dbeta"]), host(e["dgamma"]), 0.0, 0, 2),
                    "eval pooled dx")
        ys.append((host(y), host(e["dgamma"])))
    (y0, _), (y1, dg1) = ys
    assert np.isnan(y1[1, 2, 2, 3]) and np.isnan(y1[2, 7, 13, 0]) and np.isnan(y1).sum() == 2
    same = ~np.isnan(y1)
    assert np.array_equal(y0[same], y1[same])
    # dgamma = sum g * xhat[argmax]: NaN exactly where the gradient was routed to the NaN slot
    assert np.isnan(dg1[[2, 7]]).all() and np.isfinite(np.delete(dg1, [2, 7])).all()
    assert R.pool_forward(xp, rm, host(ie), ga, be, 0)[3][2, 7, 13, 0] == 3        # the last NaN of the window


# ------------------------------------------------------------------- (f) bnn_bn_fwd_final_parts directly
@pytest.mark.parametrize("M,chunk", [(40, 64), (35, 7), (48, 16), (700, 7), (1905, 13), (2400, 8), (2395, 8)])
@pytest.mark.parametrize("C", [20, 64])
def test_fwd_final_parts(L, M, chunk, C):
    """The forward merge on partials built in numpy float64: R = 1, 5, 3, 100, 147, 300, 300 (rounds of
    128 chunks with R % 16 != 0 among them), a full last chunk and a short one, C % 16 != 0."""
    rng = np.random.default_rng(M + chunk + C)
    Rn = -(-M // chunk)
    x = exact_x(rng, M, C, bias=True).astype(np.float64)
    p0, p1 = np.zeros((Rn, C)), np.zeros((Rn, C))
    for r in range(Rn):
        blk = x[r * chunk:(r + 1) * chunk]
        p0[r] = blk.sum(0)
        p1[r] = ((blk - blk.mean(0)) ** 2).sum(0)
    _, _, rm0, rv0 = params(rng, C)
    part = dev(np.stack([p0, p1]))
    outs = []
    for _ in range(2):
        o = dict(mean=zeros(C), lo=zeros(C), invstd=zeros(C), rm=dev(rm0), rv=dev(rv0))
        L.call("bnn_bn_fwd_final_parts", L.ptr(part), Rn, chunk, M, C, L.ptr(o["rm"]), L.ptr(o["rv"]), MOM, EPS,
               L.ptr(o["mean"]), L.ptr(o["invstd"]), L.ptr(o["lo"]), L.stream())
        outs.append(o)
    for k in outs[0]:
        assert bits_equal(outs[0][k], outs[1][k]), k
    check_exact_stats(outs[0], x, rm0, rv0)


# ------------------------------------------------------------------------------- (g) compact inputs
@pytest.mark.parametrize("xfmt", [1, 2])
@pytest.mark.parametrize("pool", [0, 2])
@pytest.mark.parametrize("case", BC.CASES_2D, ids=BC.id_2d)
def test_bn2d_compact_inputs_match_fp32(L, rows_restored, case, pool, xfmt):
    """bnn_bn2d_fwd_train_q / _bwd_q / _bwd_stats_q on int8 and int16 sums + xbias are bit-identical to
    the fp32 entries on fl(xq + xbias), under every bnn_bn2d_set_rows setting."""
    N, C, H, W = case.N, case.C, case.H, case.W
    rng = np.random.default_rng(N * C + W + xfmt)
    ga, be, rm0, rv0 = params(rng, C)
    lim = 100 if xfmt == 1 else 3000
    xq = rng.integers(-lim, lim + 1, (N, C, H, W)).astype(np.int8 if xfmt == 1 else np.int16)
    xb = (rng.standard_normal(C) * 3).astype(np.float32)
    x = (xq.astype(np.float32) + ch(xb)).astype(np.float32)
    dy = rng.standard_normal(out_shape(x, pool)).astype(np.float32)
    xd, dyd, gad, bed, q = dev(x), dev(dy), dev(ga), dev(be), (dev(xq), dev(xb), xfmt)
    for rows in (0, 1, 2):
        L.call("bnn_bn2d_set_rows", rows)
        a = fwd2_train(L, xd, gad, bed, 1, pool, dev(rm0), dev(rv0))
        b = fwd2_train(L, xd, gad, bed, 1, pool, dev(rm0), dev(rv0), q=q)
        for k in a:
            assert bits_equal(a[k], b[k]), f"rows {rows}: forward {k}"
        ba = bwd2(L, xd, dyd, gad, bed, a["mean"], a["invstd"], 1, pool)
        bb = bwd2(L, xd, dyd, gad, bed, a["mean"], a["invstd"], 1, pool, q=q)
        for k in ba:
            assert bits_equal(ba[k], bb[k]), f"rows {rows}: backward {k}"
        dg, db, sg, sgx, ws = zeros(C), zeros(C), zeros(C), zeros(C), work2(L, N, C)
        L.call("bnn_bn2d_bwd_stats_q", L.ptr(q[0]), L.ptr(q[1]), xfmt, L.ptr(dyd), N, C, H, W, L.ptr(gad), L.ptr(bed),
               L.ptr(a["mean"]), L.ptr(a["invstd"]), 1, int(pool), L.ptr(dg), L.ptr(db), L.ptr(sg), L.ptr(sgx),
               L.ptr(ws), L.stream())
        for got, want in ((dg, ba["dgamma"]), (db, ba["dbeta"]), (sg, ba["dbeta"]), (sgx, ba["dgamma"])):
            assert bits_equal(got, want), f"rows {rows}: bwd_stats_q"


@pytest.mark.parametrize("case", BC.SMALL_1D, ids=BC.id_1d)
def test_bn1d_i16_input_matches_fp32(L, case):
    """bnn_bn_fwd_train_i16 (int16 sums + xbias) gives the statistics of bnn_bn_fwd_train on
    fl(x16 + xbias) bit for bit, at every schedule."""
    M, C = case.M, case.C
    rng = np.random.default_rng(M + 3 * C)
    _, _, rm0, rv0 = params(rng, C)
    x16 = rng.integers(-3000, 3001, (M, C)).astype(np.int16)
    xb = (rng.standard_normal(C) * 3).astype(np.float32)
    x = (x16.astype(np.float32) + xb).astype(np.float32)
    a = fwd_train(L, dev(x), None, None, 0, dev(rm0), dev(rv0), want_y=False)
    o = dict(mean=zeros(C), lo=zeros(C), invstd=zeros(C), rm=dev(rm0), rv=dev(rv0))
    x16d, xbd, ws = dev(x16), dev(xb), work1(L, M, C)
    L.call("bnn_bn_fwd_train_i16", L.ptr(x16d), L.ptr(xbd), M, C, None, None, L.ptr(o["rm"]), L.ptr(o["rv"]), MOM,
           EPS, L.ptr(o["mean"]), L.ptr(o["invstd"]), L.ptr(o["lo"]), 0.0, 0, None, L.ptr(ws), L.stream())
    for k in o:
        assert bits_equal(o[k], a[k]), k


def test_zz_print_measured_maxima():
    """The per-column maxima of (b) over the table (DESIGN.md records them beside the shapes)."""
    for k, v in MAXIMA.items():
        print(f"[bn maxima] {k}: " + ", ".join(f"{n} {x:.3g}" for n, x in v.items()))
