"""The frozen wide-channel conv (csrc/bnn_conv_wide_infer.hip) against a float64 reference on
the CPU: exact integer sums from F.conv2d(sign(x), sign(w)), the bias added in double and rounded once to
fp32, then the BatchNorm expression in float64, Hardtanh, max-pool and the ternary sign.

The inputs make that comparison exact.  bias is a multiple of 0.5 and mean a multiple of 0.5 plus 0.25, so
x - mean is exact and never within 0.25 of zero: fp32 and float64 agree on every sign.  Channel 0 has
mean == bias (an integer) and beta = 0, so y == 0 exactly wherever I == 0; channel 1 has a negative gamma;
channel 2 has beta = NaN (expected 0 everywhere).  Outside channels 0 and 2 the float64 |y| of these seeds is
at least 0.0166 (beta = invstd gamma k / 2 keeps it off zero; the smallest is case 3's, the chain's is 0.0192),
five orders above fp32's rounding.  Every comparison is torch.equal over the whole buffer."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (N, C, H, W, Co, KH, KW, pad, pool, consumer (K2, pad2) or None for int8 signs NCHW)
CASES = [
    (1, 64, 6, 6, 65, 3, 3, 1, 0, None),          # Co tail, plane smaller than a tile
    (3, 128, 10, 12, 128, 3, 3, 1, 2, (3, 1)),    # two blocks; windows and tiles crossing image boundaries
    (2, 64, 8, 8, 64, 1, 1, 0, 2, (1, 0)),        # no shift; consumer without halo
    (2, 64, 6, 10, 192, 3, 3, 2, 2, (5, 2)),      # pad = K - 1; wide halo; three output blocks
    (1, 64, 12, 14, 80, 5, 5, 0, 2, None),        # one LDS stage
    (5, 64, 34, 34, 130, 3, 3, 1, 2, None),       # more windows than one round of tiles; row ends inside a wave
    (2, 192, 9, 7, 64, 3, 3, 1, 0, (3, 1)),       # odd sizes without pool
]
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
    """(int8 signs [N, Co, PH, PW], the float64 y before Hardtanh)."""
    sx, sw = (torch.nan_to_num(torch.sign(t), nan=0.0).double() for t in (x, w))
    z = (F.conv2d(sx, sw, padding=pad) + bias.double().view(1, -1, 1, 1)).float()
    v = lambda t: t.double().view(1, -1, 1, 1)
    y = (z.double() - v(mean)) * v(invstd) * v(gamma) + v(beta)
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
    x, w, bias, mean, invstd, gamma, beta = (t.cuda() for t in tensors)
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


@pytest.mark.parametrize("case", CASES)
def test_fused_layer_equals_float64_reference(L, case):
    N, C, H, W, Co, KH, KW, pad, pool, cons = case
    tensors = _inputs(case)
    ref, y = _reference(*tensors, pad, pool)
    keep = torch.ones(Co, dtype=torch.bool)
    keep[0] = keep[2] = False
    print("min |y| outside the planted channels:", float(y[:, keep].abs().min()), "zeros:", int((ref[:, 0] == 0).sum()))
    assert float(y[:, keep].abs().min()) >= 0.01 and bool((y[:, 0] == 0).any())
    rc, out = _run(L, case, tensors, cons)
    assert rc == 0
    if cons is None:
        assert torch.equal(out[:ref.numel()].view(torch.int8).view(ref.shape), ref)
        assert bool((out[ref.numel():] == 0xFF).all())               # nothing beyond the tensor is written
    else:
        assert torch.equal(out, _planes(ref, *cons, out.numel()))    # interior, halo and tail, byte for byte


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
