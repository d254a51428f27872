"""The stride-2 wide-channel binary conv input gradient (csrc/bnn_conv_wide_bwd_s2.hip) against
conv_transpose2d(dy, sign(w), stride=2) in float64 on the CPU, rounded once to fp32.  The inputs are chosen so
that every partial sum in any order is representable in fp32: the comparisons are bit for bit."""
import pytest
import torch

from test_conv_wide_bwd_s2_plan import GPU_CASES          # (N, C, H, W, Co, KH, KW, pad, bias)

pytestmark = pytest.mark.gpu


def _inputs(shape, kind):
    """w from {-1.5, -0, 0, 0.25} with NaNs planted.  dy "dense": integers in [-8, 8].  dy "lattice": zero except at
    oh % ceil(KH / 2) == 0 and ow % ceil(KW / 2) == 0, where one random channel holds a full-mantissa value times
    2^+-20: a dX element sees ceil(KH / 2) x ceil(KW / 2) consecutive outputs at most, so one non-zero term."""
    N, C, H, W, Co, KH, KW, pad = shape
    g = torch.Generator().manual_seed(N * 131 + C * 7 + Co)
    vals = torch.tensor([-1.5, -0.0, 0.0, 0.25])
    w = vals[torch.randint(0, 4, (Co, C, KH, KW), generator=g)]
    w.view(-1)[5::89] = float("nan")                     # tsign(NaN) = 0
    OH, OW = (H + 2 * pad - KH) // 2 + 1, (W + 2 * pad - KW) // 2 + 1
    if kind == "dense":
        return torch.randint(-8, 9, (N, Co, OH, OW), generator=g).float(), w
    sh, sw = (KH + 1) // 2, (KW + 1) // 2
    lh, lw = (OH + sh - 1) // sh, (OW + sw - 1) // sw
    v = torch.randn(N, 1, lh, lw, generator=g) * torch.exp2(torch.randint(-20, 21, (N, 1, lh, lw), generator=g).float())
    assert bool((v.view(torch.int32) & 0xFF).ne(0).any())          # the third plane is exercised
    dy = torch.zeros(N, Co, OH, OW)
    dy[:, :, ::sh, ::sw].scatter_(1, torch.randint(0, Co, (N, 1, lh, lw), generator=g), v)
    return dy, w


def _reference(dy, w, shape):
    N, C, H, W, Co, KH, KW, pad = shape
    sw = torch.nan_to_num(torch.sign(w), nan=0.0).double()
    return torch.nn.functional.conv_transpose2d(dy.double(), sw, stride=2, padding=pad,
                                                output_padding=((H + 2 * pad - KH) % 2, (W + 2 * pad - KW) % 2))


@pytest.mark.parametrize("kind", ["dense", "lattice"])
@pytest.mark.parametrize("case", GPU_CASES)
def test_input_gradient_equals_float64_reference(case, kind):
    from bnn_amd import _lib as L
    N, C, H, W, Co, KH, KW, pad = shape = case[:8]
    dy, w = _inputs(shape, kind)
    ref = _reference(dy, w, shape).float()
    assert ref.shape == (N, C, H, W) and bool(ref.ne(0).any())
    if kind == "dense":                                  # every partial sum is an integer below 2^24
        assert float(_reference(dy.abs(), w.abs(), shape).max()) < 2 ** 24
    else:                                                # at most one non-zero term per dX element
        assert int(_reference(dy.ne(0).float(), torch.ones_like(w), shape).max()) <= 1
    dyd, wd = dy.cuda(), w.cuda()
    ws = torch.empty(L.lib().bnn_conv2d_bwd_data_wide_s2_workspace(*shape), dtype=torch.uint8, device="cuda")
    dx = torch.empty(N, C, H, W, device="cuda")
    L.call("bnn_conv2d_bwd_data_wide_s2", dyd, wd, dx, N, C, H, W, Co, KH, KW, 2, pad, 1, 1, ws, ws.numel(), L.stream())
    assert torch.equal(dx.cpu(), ref)
    ws.fill_(0xFF)                                       # halo and tails are written, not assumed; dx is overwritten
    dx.fill_(7.0)
    L.call("bnn_conv2d_bwd_data_wide_s2", dyd, wd, dx, N, C, H, W, Co, KH, KW, 2, pad, 1, 1, ws, ws.numel(), L.stream())
    assert torch.equal(dx.cpu(), ref)
    if case is GPU_CASES[1] and kind == "dense":         # and bnn_conv2d_bwd_data writes the same bits
        dx0 = torch.empty_like(dx)
        L.call("bnn_conv2d_bwd_data", dyd, wd, dx0, N, C, H, W, Co, KH, KW, 2, pad, 1, 1, L.stream())
        assert torch.equal(dx0, dx)


@pytest.mark.parametrize("stride,short", [(2, 1), (1, 0)])
def test_short_workspace_and_refused_shape_launch_nothing(stride, short):
    from bnn_amd import _lib as L
    N, C, H, W, Co, KH, KW, pad = shape = GPU_CASES[0][:8]
    dy, w = _inputs(shape, "dense")
    ws = torch.empty(L.lib().bnn_conv2d_bwd_data_wide_s2_workspace(*shape), dtype=torch.uint8, device="cuda")
    dx = torch.full(shape[:4], 7.0, device="cuda")
    rc = L.lib().bnn_conv2d_bwd_data_wide_s2(dy.cuda(), w.cuda(), dx, N, C, H, W, Co, KH, KW, stride, pad, 1, 1, ws,
                                             ws.numel() - short, L.stream())
    torch.cuda.synchronize()
    assert rc == -1 and bool((dx == 7.0).all())
    assert (b"workspace" in L.lib().bnn_last_error()) == bool(short)


def test_empty_batch_returns_zero_and_writes_nothing():
    """N = 0 at the C ABI, with small non-empty tensors as the pointers (the entry refuses null)."""
    from bnn_amd import _lib as L
    N, C, H, W, Co, KH, KW, pad = shape = (0,) + GPU_CASES[0][1:8]
    dy, w = torch.ones(16, device="cuda"), torch.ones(16, device="cuda")
    dx = torch.full((64,), 7.0, device="cuda")
    ws = torch.full((L.lib().bnn_conv2d_bwd_data_wide_s2_workspace(*shape),), 0xFF, dtype=torch.uint8, device="cuda")
    assert ws.numel() > 0
    rc = L.lib().bnn_conv2d_bwd_data_wide_s2(dy, w, dx, N, C, H, W, Co, KH, KW, 2, pad, 1, 1, ws, ws.numel(), L.stream())
    torch.cuda.synchronize()
    assert rc == 0 and bool((dx == 7.0).all()) and bool((ws == 0xFF).all())


def test_module_takes_the_stride2_input_gradient(monkeypatch):
    """BinarizeConv2d(128, 136, 3, stride=2, padding=1), forward and backward, with CONV_WIDE_BWD_S2 on and off: only
    x.grad changes kernel, and both kernels meet the gradient bar of tests/test_gpu_parity.py (1e-5 norm-wise)."""
    from bnn_amd import functional as BF
    from models.binarized_modules import BinarizeConv2d
    torch.manual_seed(11)
    conv = BinarizeConv2d(128, 136, 3, stride=2, padding=1).cuda().train()
    x0 = torch.randn(2, 128, 9, 10, device="cuda")
    dy = torch.randn(2, 136, 5, 5, device="cuda")
    ref = _reference(dy.cpu(), conv.weight.detach().cpu(), (2, 128, 9, 10, 136, 3, 3, 1))
    got = {}
    for on in (True, False):
        monkeypatch.setattr(BF, "CONV_WIDE_BWD_S2", on)
        calls = BF.CONV_WIDE_BWD_S2_CALLS
        x = x0.clone().requires_grad_(True)
        conv.zero_grad()
        y = conv(x)
        y.backward(dy)
        torch.cuda.synchronize()
        assert BF.CONV_WIDE_BWD_S2_CALLS - calls == int(on)
        err = float((x.grad.cpu().double() - ref).norm() / ref.norm())
        print(f"CONV_WIDE_BWD_S2={on}: x.grad rel err {err:.3e}")
        assert err < 1e-5
        got[on] = (y.detach(), conv.weight.grad.clone(), conv.bias.grad.clone())
    for a, b in zip(got[True], got[False]):
        assert torch.equal(a, b)
