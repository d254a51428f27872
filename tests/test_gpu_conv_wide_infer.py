"""The frozen wide-channel conv (csrc/bnn_conv_wide_infer.hip) against a float64 reference on
the CPU: exact integer sums from F.conv2d(sign(x), sign(w)), the bias added in double and rounded once to
fp32, then the BatchNorm expression in float64, Hardtanh, max-pool and the ternary sign.

The inputs make that comparison exact.  bias is a multiple of 0.5 and mean a multiple of 0.5 plus 0.25, so
x - mean is exact and never within 0.25 of zero: fp32 and float64 agree on every sign.  Channel 0 has
mean == bias (an integer) and beta = 0, so y == 0 exactly wherever I == 0; channel 1 has a negative gamma;
channel 2 has beta = NaN (expected 0 everywhere).  Outside channels 0 and 2 the float64 |y| of these seeds is
at least 0.0166 (beta = invstd gamma k / 2 keeps it off zero; the smallest is case 3's, the chain's is 0.0192),
five orders above fp32's rounding; over the whole of tests/conv_wide_cases.py it is at least 0.0138 (the
130-column case's), and each test asserts its own against 0.01 before it launches.  Every comparison is torch.equal over the whole buffer."""
import pytest
import torch
import torch.nn.functional as F

import conv_wide_cases as CW

pytestmark = pytest.mark.gpu

CASES = CW.INFER_CASES                         # the seven cases the layer was merged with; the table has more
GUARD = 256


def _tsign(v):
    return (v > 0).to(torch.int8) - (v < 0).to(torch.int8)


def _inputs(case):
    N, C, H, W, Co, KH, KW, pad, pool, cons = case
    g = torch.Generator().manual_seed(N * 131 + C * 7 + Co)
    vals = torch.tensor([-1.5, -0.0, 0.0, 0.25])
    x = vals[torch.randint(0, 4, (N, C, H, W), generator=g)]
    w = vals[torch.randint(0, 4, (Co, C, KH, KW), generator=g)]
    x.view(-1)[::97] = float("nan")                      # tsign(NaN) = 0
    w.view(-1)[5::89] = float("nan")
    bias = torch.randint(-8, 9, (Co,), generator=g) * 0.5
    mean = torch.randint(-8, 9, (Co,), generator=g) * 0.5 + 0.25
    invstd = torch.rand(Co, generator=g) * 0.4 + 0.1
    gamma = (torch.rand(Co, generator=g) + 0.5) * (torch.randint(0, 2, (Co,), generator=g) * 2 - 1)
    beta = torch.randint(-2, 3, (Co,), generator=g) * 0.5 * invstd * gamma     # y = invstd gamma (x - mean + k / 2)
    w[0].view(-1)[3:] = 0.0                              # few taps: I == 0 is frequent in channel 0
    bias[0], mean[0], beta[0] = 2.0, 2.0, 0.0
    gamma[1] = -gamma[1].abs()
    beta[2] = float("nan")
    return x, w, bias, mean, invstd, gamma, beta


def _reference(x, w, bias, mean, invstd, gamma, beta, pad, pool):
    """(int8 signs [N, Co, PH, PW], the float64 y before Hardtanh).  A bias, gamma or beta of None is 0, 1, 0."""
    sx, sw = (torch.nan_to_num(torch.sign(t), nan=0.0).double() for t in (x, w))
    z = F.conv2d(sx, sw, padding=pad)
    if bias is not None:
        z = (z + bias.double().view(1, -1, 1, 1)).float()
    v = lambda t, none: none if t is None else t.double().view(1, -1, 1, 1)
    y = (z.double() - v(mean, None)) * v(invstd, None) * v(gamma, 1.0) + v(beta, 0.0)
    h = F.hardtanh(y)
    return _tsign(F.max_pool2d(h, 2, 2) if pool else h), y


def _planes(s, K2, pad2, nbytes):
    """int8 signs [N, Co, PH, PW] -> the consumer's FP4 planes, uint8 [nbytes], built in torch."""
    N, Co, PH, PW = s.shape
    code = torch.where(s > 0, 2, torch.where(s < 0, 10, 0)).to(torch.uint8)
    grid = torch.zeros((Co // 64, N, PH + 2 * pad2, PW + 2 * pad2, 64), dtype=torch.uint8)
    grid[:, :, pad2:pad2 + PH, pad2:pad2 + PW] = code.view(N, Co // 64, 64, PH, PW).permute(1, 0, 3, 4, 2)
    rows = torch.zeros((Co // 64, nbytes // (Co // 64 * 32), 64), dtype=torch.uint8)
    rows[:, :grid[0].numel() // 64] = grid.view(Co // 64, -1, 64)
    return (rows[..., 0::2] | (rows[..., 1::2] << 4)).reshape(-1)


@pytest.fixture(scope="module")
def L():
    from bnn_amd import _lib
    return _lib


def _run(L, case, tensors, cons):
    """The fused entry on pack_x's planes and pack_w's weight; out pre-filled with 0xFF.  (rc, out on the CPU)."""
    N, C, H, W, Co, KH, KW, pad, pool, _ = case
    x, w, bias, mean, invstd, gamma, beta = (None if t is None else t.cuda() for t in tensors)
    lib = L.lib()
    OH, OW = H + 2 * pad - KH + 1, W + 2 * pad - KW + 1
    PH, PW = (OH // 2, OW // 2) if pool else (OH, OW)
    planes = torch.full((lib.bnn_conv2d_wide_planes_bytes(N, C, H, W, KH, KW, pad),), 0xFF, dtype=torch.uint8, device="cuda")
    wq = torch.full((lib.bnn_conv2d_wide_wq_bytes(C, Co, KH, KW),), 0xFF, dtype=torch.uint8, device="cuda")
    L.call("bnn_conv2d_wide_pack_x", x, planes, N, C, H, W, KH, KW, pad, L.stream())
    L.call("bnn_conv2d_wide_pack_w", w, wq, C, Co, KH, KW, L.stream())
    if cons is None:
        out, form, K2, pad2 = torch.full((N * Co * PH * PW + GUARD,), 0xFF, dtype=torch.uint8, device="cuda"), 1, 0, 0
    else:
        K2, pad2 = cons
        nb = max(int(lib.bnn_conv2d_wide_planes_bytes(N, Co, PH, PW, K2, K2, pad2)), 16)
        out, form = torch.full((nb,), 0xFF, dtype=torch.uint8, device="cuda"), 0
    rc = lib.bnn_conv2d_fwd_wide_bnsign(planes, wq, bias, mean, invstd, gamma, beta, out, N, C, H, W, Co, KH, KW, pad,
                                        pool, form, K2, K2, pad2, L.stream())
    torch.cuda.synchronize()
    return rc, out.cpu()


def _check(L, case, tensors):
    """The exactness pre-conditions of these inputs, then the fused entry against the reference, byte for byte."""
    N, C, H, W, Co, KH, KW, pad, pool, cons = case
    ref, y = _reference(*tensors, pad, pool)
    keep = torch.ones(Co, dtype=torch.bool)
    keep[0] = False
    keep[2] = tensors[6] is None                         # without beta channel 2 is a channel like any other
    print("min |y| outside the planted channels:", float(y[:, keep].abs().min()), "zeros:", int((ref[:, 0] == 0).sum()))
    assert float(y[:, keep].abs().min()) >= 0.01 and bool((y[:, 0] == 0).any())
    rc, out = _run(L, case, tensors, cons)
    assert rc == 0
    if cons is None:
        assert torch.equal(out[:ref.numel()].view(torch.int8).view(ref.shape), ref)
        assert bool((out[ref.numel():] == 0xFF).all())               # nothing beyond the tensor is written
    else:
        assert torch.equal(out, _planes(ref, *cons, out.numel()))    # interior, halo and tail, byte for byte


@pytest.mark.parametrize("case", CW.infer_params())
def test_fused_layer_equals_float64_reference(L, case):
    _check(L, case, _inputs(case))


@pytest.mark.parametrize("drop", ["bias", "gamma", "beta", "all"])
@pytest.mark.parametrize("case", CW.NULL_CASES, ids=CW.shape_id)
def test_null_bias_gamma_and_beta(L, case, drop):
    """A null bias, gamma or beta is 0, 1, 0.  Without the bias x is an integer and mean still a multiple of 0.5
    plus 0.25, so x - mean stays 0.25 off zero.  Without gamma, beta is drawn for gamma = 1 (k / 2 invstd), which
    keeps y = invstd (x - mean + k / 2) off zero as before."""
    x, w, bias, mean, invstd, gamma, beta = _inputs(case)
    if drop in ("gamma", "all"):
        beta = beta / gamma
        gamma = None
    if drop in ("bias", "all"):
        bias, mean[0] = None, 0.0                        # channel 0: y == 0 exactly wherever I == 0, as with the bias
    if drop in ("beta", "all"):
        beta = None
    _check(L, case, (x, w, bias, mean, invstd, gamma, beta))


def test_empty_batch_returns_zero_and_writes_nothing(L):
    """N = 0 at the C ABI for both output forms, with small non-empty tensors as the pointers (the entry refuses
    null)."""
    N, C, H, W, Co, KH, KW, pad = CW.EMPTY
    planes, wq = (torch.zeros(256, dtype=torch.uint8, device="cuda") for _ in range(2))
    params = [torch.ones(16, device="cuda") for _ in range(5)]
    for form, K2, pad2 in ((1, 0, 0), (0, 3, 1)):
        out = torch.full((1024,), 0xFF, dtype=torch.uint8, device="cuda")
        rc = L.lib().bnn_conv2d_fwd_wide_bnsign(planes, wq, *params, out, N, C, H, W, Co, KH, KW, pad, 2, form, K2, K2,
                                                pad2, L.stream())
        torch.cuda.synchronize()
        assert rc == 0 and bool((out == 0xFF).all())


def _stack(seed=3):
    import torch.nn as nn
    from bnn_amd import inference
    from bnn_amd.nn import BinarizeConv2d
    g = torch.Generator().manual_seed(seed)
    blocks = []
    for C, Co, pool in ((64, 128, True), (128, 128, False), (128, 64, True)):
        conv, bn = BinarizeConv2d(C, Co, 3, padding=1), nn.BatchNorm2d(Co)
        with torch.no_grad():
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=g))
            conv.bias.copy_(torch.randint(-8, 9, (Co,), generator=g) * 0.5)
            bn.running_mean.copy_(torch.randint(-8, 9, (Co,), generator=g) * 0.5 + 0.25)
            bn.running_var.copy_(torch.rand(Co, generator=g) * 40 + 4)
            bn.weight.copy_((torch.rand(Co, generator=g) + 0.5) * (torch.randint(0, 2, (Co,), generator=g) * 2 - 1))
            bn.bias.copy_(torch.randint(-2, 3, (Co,), generator=g) * 0.5 * inference._invstd(bn.running_var, bn.eps) * bn.weight)
        blocks.append(nn.Sequential(conv, bn, nn.Hardtanh(), *([nn.MaxPool2d(2, 2)] if pool else [])))
    return blocks, torch.randn(3, 64, 8, 8, generator=g)


def test_stack_of_three_blocks():
    from bnn_amd import inference
    blocks, x = _stack()
    s, ymin = x, float("inf")
    for seq in blocks:                                   # the float64 reference, block by block
        conv, bn = seq[0], seq[1]
        s, y = _reference(s, conv.weight.detach(), conv.bias.detach(), bn.running_mean,
                          inference._invstd(bn.running_var, bn.eps), bn.weight.detach(), bn.bias.detach(), 1, len(seq) == 4)
        ymin = min(ymin, float(y.abs().min()))
        s = s.float()
    print("min |y|:", ymin)
    assert ymin >= 0.01
    frozen = inference.freeze_conv_stack(blocks).to("cuda")
    xd = x.cuda()
    calls = inference.WIDE_FUSED_CALLS
    out = frozen(xd)
    assert inference.WIDE_FUSED_CALLS - calls == 3
    got = out.cpu()
    assert got.dtype == torch.int8 and torch.equal(got, s.to(torch.int8))
    assert frozen(xd).data_ptr() == out.data_ptr()       # the buffers of this N are kept
    frozen.two_pass = True
    calls = inference.WIDE_FUSED_CALLS
    assert torch.equal(frozen(xd).cpu(), got) and inference.WIDE_FUSED_CALLS == calls


def test_refusals(L):
    import torch.nn as nn
    from bnn_amd import inference
    from bnn_amd.nn import BinarizeConv2d
    case = CASES[1][:9] + ((3, 3),)                      # a consumer with pad2 = K2
    rc, out = _run(L, case, _inputs(case), case[9])
    assert rc == -1 and bool((out == 0xFF).all())
    with pytest.raises(ValueError):
        inference.freeze_conv_stack([nn.Sequential(BinarizeConv2d(64, 128, 3, padding=1), nn.BatchNorm2d(128))])
    with pytest.raises(ValueError):
        inference.freeze_conv_stack([nn.Sequential(BinarizeConv2d(3, 128, 3, padding=1), nn.BatchNorm2d(128), nn.Hardtanh())])
