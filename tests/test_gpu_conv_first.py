"""The first-layer (real-input) binary conv forward and filter / bias gradient (with the measured
figures) at the C ABI and through the module, against float64 F.conv2d and its autograd on the CPU."""
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from bnn_amd import _lib as L

gpu = pytest.mark.gpu
BAR = 1e-5                                    # the project's norm-wise bar (tests/test_gpu_parity.py)
SHAPES = [                                    # N, C, H, W, Co, KH, KW, pad
    (1, 3, 5, 7, 65, 3, 3, 1),                # the Co tail, a map smaller than a tile
    (3, 3, 9, 11, 129, 3, 3, 1),              # two channel tiles
    (2, 3, 10, 10, 65, 3, 3, 0),              # pad 0, 16-B dy loads
    (2, 3, 6, 6, 65, 3, 3, 2),                # pad = K - 1
    (2, 4, 6, 9, 70, 2, 4, 1),                # C = 4, Kt = 32: db's column opens a second block
    (2, 3, 9, 11, 65, 5, 5, 2),               # 5 k-steps, 3 column blocks
    (2, 3, 6, 8, 65, 1, 1, 0),                # 1x1
    (1, 3, 3, 132, 65, 3, 3, 1),              # a row longer than a position tile: chunks of 64 + 64 + 4 columns
    (1, 2, 2, 71, 65, 1, 3, 0),               # ... and of 64 + 5, an odd chunk width
    (1, 1, 601, 3, 65, 3, 3, 1),              # C = 1, tiles that wrap rows, 301 K slices with a short last one
]


def _out_hw(s):
    N, C, H, W, Co, KH, KW, pad = s
    return H + 2 * pad - KH + 1, W + 2 * pad - KW + 1


def _weight(s, g):
    N, C, H, W, Co, KH, KW, pad = s       # every sign, both zeros and NaN: tsign gives 0 for 0, -0 and NaN
    vals = torch.tensor([-0.7, 0.3, 1.5, -2.0, 0.0, -0.0, float("nan")])
    return vals[torch.randint(0, 7, (Co, C, KH, KW), generator=g)]


def _sign(w):
    return torch.nan_to_num(torch.sign(w), nan=0.0).double()


def _full(shape, g):
    v = torch.randn(shape, generator=g) * torch.exp2(torch.randint(-20, 21, shape, generator=g).float())
    return torch.where(v == 0, torch.ones_like(v), v)


def _inputs(s, kind, seed=0):
    """(x, w, bias, dy).  ints: small integers, every partial sum exact in any order.  lattice: x zero except one
    full-mantissa value per KH x KW lattice cell (one offset and one channel per sample), bias 0: y = +-v or 0.
    dyhot: one full-mantissa dy per output channel against x = +-2^e.  xhot: one full-mantissa x per input channel
    against dy = +-2^e, |e| <= 3: one term per dw element, db exact.  real: randn, full mantissas over 40 binades."""
    N, C, H, W, Co, KH, KW, pad = s
    OH, OW = _out_hw(s)
    g = torch.Generator().manual_seed(1000 * seed + N * 131 + C * 7 + Co + W)
    w = _weight(s, g)
    pow2 = lambda sh, e: torch.exp2(torch.randint(-e, e + 1, sh, generator=g).float()) * (torch.randint(0, 2, sh, generator=g) * 2 - 1)
    if kind == "ints":
        return (torch.randint(-4, 5, (N, C, H, W), generator=g).float(), w,
                torch.randint(-9, 10, (Co,), generator=g).float(), torch.randint(-8, 9, (N, Co, OH, OW), generator=g).float())
    if kind == "lattice":
        x = torch.zeros(N, C, H, W)
        for n in range(N):
            a, b = int(torch.randint(0, KH, (1,), generator=g)), int(torch.randint(0, KW, (1,), generator=g))
            sub = x[n, int(torch.randint(0, C, (1,), generator=g)), a::KH, b::KW]
            sub.copy_(_full(tuple(sub.shape), g))
        return x, w, torch.zeros(Co), None
    if kind == "dyhot":
        dy = torch.zeros(N, Co, OH * OW)
        dy[torch.randint(0, N, (Co,), generator=g), torch.arange(Co), torch.randint(0, OH * OW, (Co,), generator=g)] = _full((Co,), g)
        return pow2((N, C, H, W), 8), w, None, dy.view(N, Co, OH, OW)
    if kind == "xhot":
        x = torch.zeros(N, C, H * W)
        x[torch.randint(0, N, (C,), generator=g), torch.arange(C), torch.randint(0, H * W, (C,), generator=g)] = _full((C,), g)
        return x.view(N, C, H, W), w, None, pow2((N, Co, OH, OW), 3)
    return (torch.randn(N, C, H, W, generator=g), w, torch.randn(Co, generator=g), torch.randn(N, Co, OH, OW, generator=g))


def _ref_fwd(x, w, bias, pad):
    return TF.conv2d(x.double(), _sign(w), bias.double(), padding=pad)


def _ref_filt(x, dy, s):
    N, C, H, W, Co, KH, KW, pad = s
    return torch.nn.grad.conv2d_weight(x.double(), (Co, C, KH, KW), dy.double(), padding=pad), dy.double().sum((0, 2, 3))


def _guarded(numel):      # numel floats pre-filled with 0xFF bytes, followed by a guard of 64 more
    buf = torch.full(((numel + 64) * 4,), 0xFF, dtype=torch.uint8, device="cuda")
    return buf, buf[:numel * 4].view(torch.float32), buf[numel * 4:]


def _fwd(s, x, w, bias):
    N, C, H, W, Co, KH, KW, pad = s
    OH, OW = _out_hw(s)
    _, y, guard = _guarded(N * Co * OH * OW)
    L.call("bnn_conv2d_fwd_first", x.cuda(), w.cuda(), None if bias is None else bias.cuda(), y, N, C, H, W, Co, KH, KW,
           1, pad, 1, 1, L.stream())
    torch.cuda.synchronize()
    assert bool((guard == 0xFF).all())
    return y.view(N, Co, OH, OW).cpu()


def _filt(s, x, dy, with_db=True):
    N, C, H, W, Co, KH, KW, pad = s
    nws = L.lib().bnn_conv2d_bwd_filter_first_workspace(N, C, H, W, Co, KH, KW, pad)
    _, ws, wguard = _guarded(nws // 4)
    _, dw, guard = _guarded(Co * C * KH * KW)
    _, db, bguard = _guarded(Co)
    L.call("bnn_conv2d_bwd_filter_first", dy.cuda(), x.cuda(), dw, db if with_db else None, N, C, H, W, Co, KH, KW,
           1, pad, 1, 1, ws, nws, L.stream())
    torch.cuda.synchronize()
    assert bool((guard == 0xFF).all()) and bool((bguard == 0xFF).all()) and bool((wguard == 0xFF).all())
    assert with_db or bool((db.view(torch.int32) == -1).all())
    return dw.view(Co, C, KH, KW).cpu(), db.cpu()


def _rel(a, ref):
    return float((a.double() - ref).norm() / ref.norm())


@gpu
@pytest.mark.parametrize("s", SHAPES)
def test_exact_on_integers_and_on_full_mantissas(s):
    x, w, bias, dy = _inputs(s, "ints")
    assert torch.equal(_fwd(s, x, w, bias), _ref_fwd(x, w, bias, s[7]).float())
    rw, rb = _ref_filt(x, dy, s)
    assert float(rw.abs().max()) > 0 and float(_ref_filt(x.abs(), dy.abs(), s)[0].max()) < 2 ** 24
    dw, db = _filt(s, x, dy)
    assert torch.equal(dw, rw.float()) and torch.equal(db, rb.float())
    assert torch.equal(_filt(s, x, dy, with_db=False)[0], rw.float())
    # full mantissas, for which the order cannot matter
    x, w, bias, _ = _inputs(s, "lattice")
    assert bool((x.view(torch.int32) & 0xFF).ne(0).any())          # the third plane is exercised
    ref = _ref_fwd(x, w, bias, s[7])
    assert int(TF.conv2d(x.ne(0).double(), torch.ones_like(w).double(), padding=s[7]).max()) == 1
    assert torch.equal(_fwd(s, x, w, bias), ref.float()) and bool(ref.ne(0).any())
    for kind in ("dyhot", "xhot"):
        x, _, _, dy = _inputs(s, kind)
        rw, rb = _ref_filt(x, dy, s)
        assert int(_ref_filt(x.ne(0).float(), dy.ne(0).float(), s)[0].max()) <= 1 and bool(rw.ne(0).any())
        dw, db = _filt(s, x, dy)
        assert torch.equal(dw, rw.float()) and torch.equal(db, rb.float())


def _elementwise_bound(x, w, bias, s):      # 3 Kt exact products and the bias add, one bit of slack
    Kt = s[1] * s[5] * s[6]
    return (3 * Kt + 2) * 2.0 ** -23 * _ref_fwd(x.abs(), _sign(w).abs(), bias.abs(), s[7])


@gpu
@pytest.mark.parametrize("s", SHAPES)
def test_real_inputs_within_the_bars(s):
    x, w, bias, dy = _inputs(s, "real")
    ref = _ref_fwd(x, w, bias, s[7])
    y = _fwd(s, x, w, bias)
    rw, rb = _ref_filt(x, dy, s)
    dw, db = _filt(s, x, dy)
    excess = float(((y.double() - ref).abs() / _elementwise_bound(x, w, bias, s)).max())
    print(f"{s}: y {_rel(y, ref):.2e}  dw {_rel(dw, rw):.2e}  db {_rel(db, rb):.2e}  |y - ref| / bound {excess:.3f}")
    assert _rel(y, ref) < BAR and _rel(dw, rw) < BAR and _rel(db, rb) < BAR and excess <= 1.0


@pytest.mark.parametrize("s", SHAPES)
def test_a_float32_evaluation_of_the_reference_meets_the_bars(s):
    """On the CPU: the bars are attainable in fp32 on these seeds (numpy, tap after tap / sample after sample)."""
    N, C, H, W, Co, KH, KW, pad = s
    OH, OW = _out_hw(s)
    x, w, bias, dy = _inputs(s, "real")
    xp = np.pad(x.numpy(), ((0, 0), (0, 0), (pad, pad), (pad, pad)))
    sw, dyn = _sign(w).float().numpy(), dy.numpy()
    y = np.zeros((N, Co, OH, OW), np.float32)
    dw = np.zeros((Co, C, KH, KW), np.float32)
    for c in range(C):
        for kh in range(KH):
            for kw in range(KW):
                win = xp[:, c, kh:kh + OH, kw:kw + OW]
                y += win[:, None] * sw[None, :, c, kh, kw, None, None]
                dw[:, c, kh, kw] = np.einsum("nohw,nhw->o", dyn, win, dtype=np.float32)
    y += bias.numpy()[None, :, None, None]
    ref = _ref_fwd(x, w, bias, pad)
    rw, rb = _ref_filt(x, dy, s)
    assert _rel(torch.from_numpy(y), ref) < BAR and bool(((torch.from_numpy(y).double() - ref).abs() <= _elementwise_bound(x, w, bias, s)).all())
    assert _rel(torch.from_numpy(dw), rw) < BAR and _rel(torch.from_numpy(dyn.sum((0, 2, 3), dtype=np.float32)), rb) < BAR


@gpu
def test_slices_with_a_short_last_one_and_the_empty_batch():
    N, C, H, W, Co, KH, KW, pad = SHAPES[-1]
    f = {k: int(v) for k, v in re.findall(rb"(\w+)=(\d+)", L.lib().bnn_conv2d_bwd_filter_first_kernel(N, C, H, W, Co, KH, KW, 1, pad, 1, 1))}
    assert f[b"splits"] > 1 and (f[b"splits"] - 1) * f[b"slice"] < f[b"rows"] < f[b"splits"] * f[b"slice"]
    s, one = (0, 3, 8, 8, 65, 3, 3, 1), torch.ones(16)
    assert _fwd(s, one, torch.ones(65, 3, 3, 3), None).numel() == 0
    dw, db = _filt(s, one, one)
    assert bool((dw.view(torch.int32) == 0).all()) and bool((db.view(torch.int32) == 0).all())


@gpu
def test_module_takes_the_first_layer_path(monkeypatch):
    """The counters move only with the switch on, both runs meet the bars; a binarised 1-channel input stays out."""
    from bnn_amd import functional as BF
    from models.binarized_modules import BinarizeConv2d
    torch.manual_seed(5)
    conv = BinarizeConv2d(3, 65, 3, padding=1).cuda().train()
    x0, dy = torch.randn(4, 3, 9, 10, device="cuda"), torch.randn(4, 65, 9, 10, device="cuda")
    for on in (True, False):
        monkeypatch.setattr(BF, "CONV_FIRST", on)
        calls = (BF.CONV_FIRST_CALLS, BF.CONV_FIRST_FILTER_CALLS)
        conv.zero_grad()
        y = conv(x0.clone())
        y.backward(dy)
        torch.cuda.synchronize()
        assert (BF.CONV_FIRST_CALLS - calls[0], BF.CONV_FIRST_FILTER_CALLS - calls[1]) == (int(on), int(on))
        w, b, s = conv.weight.detach().cpu(), conv.bias.detach().cpu(), (4, 3, 9, 10, 65, 3, 3, 1)
        ref, (rw, rb) = _ref_fwd(x0.cpu(), w, b, 1), _ref_filt(x0.cpu(), dy.cpu(), s)
        errs = (_rel(y.detach().cpu(), ref), _rel(conv.weight.grad.cpu(), rw), _rel(conv.bias.grad.cpu(), rb))
        assert max(errs) < BAR, (on, errs)
        assert bool(((y.detach().cpu().double() - ref).abs() <= _elementwise_bound(x0.cpu(), w, b, s)).all())
    monkeypatch.setattr(BF, "CONV_FIRST", True)
    calls = (BF.CONV_FIRST_CALLS, BF.CONV_FIRST_FILTER_CALLS)
    mono = BinarizeConv2d(1, 65, 3, padding=1).cuda().train()
    mono(torch.randn(2, 1, 9, 10, device="cuda")).sum().backward()
    assert (BF.CONV_FIRST_CALLS, BF.CONV_FIRST_FILTER_CALLS) == calls
