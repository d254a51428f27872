"""The wide-channel binary conv forward (csrc/bnn_conv_wide.hip) against
F.conv2d(sign(x), sign(w)) + bias in float64 on the CPU, rounded once to fp32: the integer sums and
the sum with the bias are exact in double, so that is fl((float)I + bias) and every comparison is
bit for bit."""
import pytest
import torch

import conv_wide_cases as CW

pytestmark = pytest.mark.gpu

SHAPES, NO_BIAS = CW.SHAPES, CW.NO_BIAS         # the seven shapes the family was merged with; the table has more


def _inputs(shape, bias=True):
    N, C, H, W, Co, KH, KW, pad = shape
    g = torch.Generator().manual_seed(N * 131 + C * 7 + Co)
    vals = torch.tensor([-1.5, -0.0, 0.0, 0.25])
    x = vals[torch.randint(0, 4, (N, C, H, W), generator=g)]
    w = vals[torch.randint(0, 4, (Co, C, KH, KW), generator=g)]
    x.view(-1)[::97] = float("nan")                      # tsign(NaN) = 0
    w.view(-1)[5::89] = float("nan")
    b = torch.randn(Co, generator=g) * 3.7 if bias else None
    return x, w, b


def _reference(x, w, b, pad):
    sx, sw = (torch.nan_to_num(torch.sign(t), nan=0.0).double() for t in (x, w))
    ref = torch.nn.functional.conv2d(sx, sw, padding=pad)
    if b is not None:
        ref = ref + b.double().view(1, -1, 1, 1)
    return ref.float()


def _wide(x, w, b, shape, fill=None, short=0):
    """bnn_conv2d_fwd_wide on CUDA copies; y starts as 7.0 everywhere.  Returns (rc, y on the CPU)."""
    from bnn_amd import _lib as L
    N, C, H, W, Co, KH, KW, pad = shape
    xd, wd, bd = x.cuda(), w.cuda(), None if b is None else b.cuda()
    y = torch.full((N, Co, H + 2 * pad - KH + 1, W + 2 * pad - KW + 1), 7.0, device="cuda")
    ws = torch.empty(L.lib().bnn_conv2d_fwd_wide_workspace(N, C, H, W, Co, KH, KW, pad), dtype=torch.uint8, device="cuda")
    if fill is not None:
        ws.fill_(fill)
    rc = L.lib().bnn_conv2d_fwd_wide(xd, wd, bd, y, N, C, H, W, Co, KH, KW, 1, pad, 1, 1, ws, ws.numel() - short,
                                     L.stream())
    torch.cuda.synchronize()
    return rc, y.cpu()


@pytest.mark.parametrize("shape", CW.for_op("fwd"))
def test_wide_forward_equals_float64_reference(shape):
    from bnn_amd import _lib as L
    N, C, H, W, Co, KH, KW, pad = shape
    x, w, b = _inputs(shape, bias=shape is not NO_BIAS)
    ref = _reference(x, w, b, pad)
    assert C * KH * KW < 2 ** 24 and bool(ref.ne(0).any())           # the integer sums are exact in fp32
    rc, y = _wide(x, w, b, shape)
    assert rc == 0 and torch.equal(y, ref)
    rc, y = _wide(x, w, b, shape, fill=0xFF)             # the halo and the tail are written, not assumed
    assert rc == 0 and torch.equal(y, ref)
    if shape is SHAPES[1]:                               # and bnn_conv2d_fwd writes the same bits
        y0 = torch.empty(ref.shape, device="cuda")
        L.call("bnn_conv2d_fwd", x.cuda(), 1, w.cuda(), b.cuda(), y0, N, C, H, W, Co, KH, KW, 1, pad, 1, 1, L.stream())
        assert torch.equal(y0.cpu(), y)


def test_short_workspace_and_refused_shape_launch_nothing():
    from bnn_amd import _lib as L
    shape = SHAPES[0]
    x, w, b = _inputs(shape)
    rc, y = _wide(x, w, b, shape, short=1)
    assert rc == -1 and bool((y == 7.0).all()) and b"workspace" in L.lib().bnn_last_error()
    N, C, H, W, Co, KH, KW, pad = shape
    y = torch.full((N, Co, 3, 4), 7.0, device="cuda")    # stride 2
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    rc = L.lib().bnn_conv2d_fwd_wide(x.cuda(), w.cuda(), b.cuda(), y, N, C, H, W, Co, KH, KW, 2, pad, 1, 1, ws,
                                     ws.numel(), L.stream())
    torch.cuda.synchronize()
    assert rc == -1 and bool((y == 7.0).all())


@pytest.mark.parametrize("mode", ["det", "stoch"])
def test_module_takes_the_wide_path_with_the_same_bits(mode, monkeypatch):
    """BinarizeConv2d(64, 96, 3, padding=1), forward and backward, with CONV_WIDE on and off: the backward
    is shared and the forward exact, so everything is equal bit for bit; "stoch" binarises x in front."""
    from bnn_amd import functional as BF
    from models.binarized_modules import BinarizeConv2d
    torch.manual_seed(11)
    conv = BinarizeConv2d(64, 96, 3, padding=1).cuda().train()
    conv.quant_mode = mode
    x0 = torch.randn(2, 64, 10, 10, device="cuda")
    dy = torch.randn(2, 96, 10, 10, device="cuda")
    got = {}
    for on in (True, False):
        monkeypatch.setattr(BF, "CONV_WIDE", on)
        calls = BF.CONV_WIDE_CALLS
        torch.manual_seed(5)                             # the stochastic draw's seed
        x = x0.clone().requires_grad_(True)
        conv.zero_grad()
        y = conv(x)
        y.backward(dy)
        torch.cuda.synchronize()
        assert BF.CONV_WIDE_CALLS - calls == int(on)
        got[on] = (y.detach(), conv.weight.grad.clone(), conv.bias.grad.clone(), x.grad.clone())
    for a, b in zip(got[True], got[False]):
        assert torch.equal(a, b)


def test_empty_batch_returns_zero_and_writes_nothing():
    """N = 0 at the C ABI (functional.py never gets here: it answers an empty batch itself).  An empty tensor's
    data_ptr() is null and the entry refuses null, so the pointers are small non-empty tensors."""
    from bnn_amd import _lib as L
    N, C, H, W, Co, KH, KW, pad = CW.EMPTY
    x, w, b = (torch.ones(16, device="cuda") for _ in range(3))
    y = torch.full((64,), 7.0, device="cuda")
    ws = torch.full((L.lib().bnn_conv2d_fwd_wide_workspace(*CW.EMPTY),), 0xFF, dtype=torch.uint8, device="cuda")
    assert ws.numel() > 0
    rc = L.lib().bnn_conv2d_fwd_wide(x, w, b, y, N, C, H, W, Co, KH, KW, 1, pad, 1, 1, ws, ws.numel(), L.stream())
    torch.cuda.synchronize()
    assert rc == 0 and bool((y == 7.0).all()) and bool((ws == 0xFF).all())


def test_module_round_trip_on_a_non_square_kernel(monkeypatch):
    """BinarizeConv2d(64, 72, (5, 3), padding=1), forward and backward, with the three CONV_WIDE* switches on and
    off together (the table's shape whose filter gradient has a short last tap group): y is equal bit for bit,
    the three gradients meet the bar of tests/test_gpu_parity.py (1e-5 norm-wise) against float64 either way,
    and each wide entry is called exactly once when its switch is on."""
    import test_gpu_conv_wide_bwd as B
    import test_gpu_conv_wide_bwd_filter as BF_
    from bnn_amd import functional as BF
    from models.binarized_modules import BinarizeConv2d
    assert (2, 64, 7, 9, 72, 5, 3, 1) in CW.NEW_SHAPES
    torch.manual_seed(11)
    conv = BinarizeConv2d(64, 72, (5, 3), padding=1).cuda().train()
    x0 = torch.randn(2, 64, 7, 9, device="cuda")
    dy = torch.randn(2, 72, 5, 9, device="cuda")
    w = conv.weight.detach().cpu()
    rx = B._reference(dy.cpu(), w, 1)
    rw, rb = BF_._reference(dy.cpu(), x0.cpu(), (72, 64, 5, 3), 1)
    counters = ("CONV_WIDE_CALLS", "CONV_WIDE_BWD_CALLS", "CONV_WIDE_BWD_FILTER_CALLS")
    ys = {}
    for on in (True, False):
        for name in ("CONV_WIDE", "CONV_WIDE_BWD", "CONV_WIDE_BWD_FILTER"):
            monkeypatch.setattr(BF, name, on)
        calls = [getattr(BF, c) for c in counters]
        x = x0.clone().requires_grad_(True)
        conv.zero_grad()
        y = conv(x)
        y.backward(dy)
        torch.cuda.synchronize()
        assert [getattr(BF, c) - c0 for c, c0 in zip(counters, calls)] == [int(on)] * 3
        for name, grad, ref in (("x", x.grad, rx), ("weight", conv.weight.grad, rw), ("bias", conv.bias.grad, rb)):
            err = float((grad.cpu().double() - ref).norm() / ref.norm())
            print(f"CONV_WIDE*={on}: {name}.grad rel err {err:.3e}")
            assert err < 1e-5
        ys[on] = y.detach()
    assert torch.equal(ys[True], ys[False])
