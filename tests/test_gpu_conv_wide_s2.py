"""The stride-2 wide-channel binary conv forward (csrc/bnn_conv_wide_s2.hip) against
F.conv2d(sign(x), sign(w), stride 2) + bias in float64 on the CPU, rounded once to fp32: the integer sums and
the sum with the bias are exact in double, so that is fl((float)I + bias) and every comparison is bit for bit."""
import pytest
import torch

from test_conv_wide_s2_plan import CASES

pytestmark = pytest.mark.gpu


def _inputs(case):
    N, C, H, W, Co, KH, KW, pad, bias = case
    g = torch.Generator().manual_seed(N * 131 + C * 7 + Co + W)
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(Co, C, KH, KW, generator=g)
    x.view(-1)[::7], x.view(-1)[3::11], x.view(-1)[5::97] = 0.0, -0.0, float("nan")      # tsign gives 0 for all three
    w.view(-1)[2::5] = 0.0
    return x, w, (torch.randn(Co, generator=g) * 3.7 if bias else None)


def _reference(x, w, b, pad):
    sx, sw = (torch.nan_to_num(torch.sign(t), nan=0.0).double() for t in (x, w))
    ref = torch.nn.functional.conv2d(sx, sw, None, 2, pad)
    assert float(ref.abs().max()) < 2 ** 24 and bool(ref.ne(0).any())
    return (ref if b is None else ref + b.double().view(1, -1, 1, 1)).float()


def _s2(x, w, b, case, short=0):
    """bnn_conv2d_fwd_wide_s2 on CUDA copies, the workspace prefilled with 0xFF and y with 7.0.  (rc, y on the CPU)"""
    from bnn_amd import _lib as L
    N, C, H, W, Co, KH, KW, pad, _ = case
    y = torch.full((N, Co, (H + 2 * pad - KH) // 2 + 1, (W + 2 * pad - KW) // 2 + 1), 7.0, device="cuda")
    ws = torch.full((L.lib().bnn_conv2d_fwd_wide_s2_workspace(*case[:8]),), 0xFF, dtype=torch.uint8, device="cuda")
    rc = L.lib().bnn_conv2d_fwd_wide_s2(x.cuda(), w.cuda(), None if b is None else b.cuda(), y, N, C, H, W, Co, KH, KW,
                                        2, pad, 1, 1, ws, ws.numel() - short, L.stream())
    torch.cuda.synchronize()
    return rc, y.cpu()


@pytest.mark.parametrize("case", CASES)
def test_s2_forward_equals_float64_reference(case):
    x, w, b = _inputs(case)
    rc, y = _s2(x, w, b, case)
    assert rc == 0 and torch.equal(y, _reference(x, w, b, case[7]))


def test_short_workspace_launches_nothing():
    from bnn_amd import _lib as L
    x, w, b = _inputs(CASES[0])
    rc, y = _s2(x, w, b, CASES[0], short=1)
    assert rc == -1 and bool((y == 7.0).all()) and b"workspace" in L.lib().bnn_last_error()


def test_empty_batch_returns_zero_and_writes_nothing():
    """N = 0 at the C ABI (functional.py answers an empty batch itself).  An empty tensor's data_ptr() is null
    and the entry refuses null, so the pointers are small non-empty tensors."""
    from bnn_amd import _lib as L
    x, w, b = (torch.ones(16, device="cuda") for _ in range(3))
    y = torch.full((64,), 7.0, device="cuda")
    ws = torch.full((L.lib().bnn_conv2d_fwd_wide_s2_workspace(0, 128, 8, 8, 128, 3, 3, 1),), 0xFF, dtype=torch.uint8,
                    device="cuda")
    assert ws.numel() > 0
    rc = L.lib().bnn_conv2d_fwd_wide_s2(x, w, b, y, 0, 128, 8, 8, 128, 3, 3, 2, 1, 1, 1, ws, ws.numel(), L.stream())
    torch.cuda.synchronize()
    assert rc == 0 and bool((y == 7.0).all()) and bool((ws == 0xFF).all())


def test_module_takes_the_s2_path_with_the_same_bits(monkeypatch):
    """nn.BinarizeConv2d(128, 136, 3, stride=2, padding=1), forward and backward, with CONV_WIDE_S2 on and off:
    the forward is exact and the backward shared, so the output and all three gradients are equal bit for bit."""
    from bnn_amd import functional as BF
    from bnn_amd.nn import BinarizeConv2d
    torch.manual_seed(11)
    conv = BinarizeConv2d(128, 136, 3, stride=2, padding=1).cuda().train()
    x0 = torch.randn(2, 128, 9, 10, device="cuda")
    dy = torch.randn(2, 136, 5, 5, device="cuda")
    got = {}
    for on in (True, False):
        monkeypatch.setattr(BF, "CONV_WIDE_S2", on)
        calls = BF.CONV_WIDE_S2_CALLS
        x = x0.clone().requires_grad_(True)
        conv.zero_grad()
        y = conv(x)
        y.backward(dy)
        torch.cuda.synchronize()
        assert BF.CONV_WIDE_S2_CALLS - calls == int(on)
        got[on] = (y.detach(), conv.weight.grad.clone(), conv.bias.grad.clone(), x.grad.clone())
    assert bool(got[True][0].ne(0).any())
    for a, b in zip(got[True], got[False]):
        assert torch.equal(a, b)
