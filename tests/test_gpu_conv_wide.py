"""The wide-channel binary conv forward (csrc/bnn_conv_wide.hip) against
F.conv2d(sign(x), sign(w)) + bias in float64 on the CPU, rounded once to fp32: the integer sums and
the sum with the bias are exact in double, so that is fl((float)I + bias) and every comparison is
bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# (N, C, H, W, Co, KH, KW, pad)
SHAPES = [
    (1, 64, 5, 7, 65, 3, 3, 1),        # Co tail, plane smaller than a tile
    (3, 128, 9, 11, 129, 3, 3, 1),     # two channel blocks, two co tiles, tiles crossing image boundaries
    (2, 64, 6, 6, 128, 1, 1, 0),       # no shift
    (2, 64, 7, 9, 72, 3, 3, 2),        # pad = K - 1
    (1, 64, 12, 13, 80, 5, 5, 0),      # 5x5 (one LDS stage), no padding
    (2, 192, 8, 8, 16, 1, 3, 0),       # non-square kernel, narrow Co, three blocks
    (5, 64, 33, 34, 130, 3, 3, 1),     # more positions than one round of tiles per image, odd Wp
]
NO_BIAS = SHAPES[3]


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


@pytest.mark.parametrize("shape", SHAPES)
def test_wide_forward_equals_float64_reference(shape):
    from bnn_amd import _lib as L
    N, C, H, W, Co, KH, KW, pad = shape
    x, w, b = _inputs(shape, bias=shape is not NO_BIAS)
    ref = _reference(x, w, b, pad)
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
