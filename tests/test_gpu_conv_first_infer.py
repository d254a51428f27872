"""The frozen first-layer conv (csrc/bnn_conv_first_infer.hip) against a float64 reference on the
CPU.  The bit-exact inputs make fp32 and float64 agree: x is a multiple of 1/8 in [-2, 2], bias of 1/2, mean of 1/8
plus 1/16, so every partial sum is exact and x' - mean is at least 1/16 from zero; with invstd in [0.1, 0.5], |gamma|
in [0.5, 1.5] and beta = invstd gamma k / 8, |y| = |invstd gamma (x' - mean + k / 8)| >= 3.1e-3 (each case asserts
1e-3).  Channel 0 has mean == bias, beta = 0 and three taps, so y == 0 occurs; channel 1 has beta = NaN."""
import pytest
import torch
import torch.nn.functional as F

import conv_first_infer_cases as CF

pytestmark = pytest.mark.gpu
GUARD = 256
U = 2.0 ** -23


def _tsign(v):
    return (v > 0).to(torch.int8) - (v < 0).to(torch.int8)


def _inputs(case, exact=True):
    N, C, H, W, Co, KH, KW, pad, pool, cons = case
    g = torch.Generator().manual_seed(N * 131 + C * 7 + Co)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
    w = torch.randn(Co, C, KH, KW, generator=g)
    invstd = torch.rand(Co, generator=g) * 0.4 + 0.1
    gamma = (torch.rand(Co, generator=g) + 0.5) * (ri(0, 1, Co) * 2 - 1)
    if not exact:
        return (torch.randn(N, C, H, W, generator=g), w, torch.randn(Co, generator=g), torch.randn(Co, generator=g),
                invstd, gamma, torch.randn(Co, generator=g))
    x = ri(-16, 16, N, C, H, W) / 8
    x.view(-1)[::5] = 0.0
    w.view(-1)[7::53] = 0.0
    bias, mean = ri(-8, 8, Co) / 2, ri(-16, 16, Co) / 8 + 1 / 16
    beta = ri(-2, 2, Co) / 8 * invstd * gamma
    w[0].view(-1)[3:] = 0.0                              # few taps: I == 0 is frequent in channel 0
    bias[0], mean[0], beta[0] = 1.5, 1.5, 0.0
    beta[1] = float("nan")
    return x, w, bias, mean, invstd, gamma, beta


def _reference(x, w, bias, mean, invstd, gamma, beta, pad, pool, real=True):
    """(int8 signs [N, Co, PH, PW], float64 y, the sign-flip bound tau per element).  None is 0, 1, 0."""
    v = lambda t, none: torch.full((1, 1, 1, 1), none).double() if t is None else t.double().view(1, -1, 1, 1)
    sw = torch.sign(w).double()
    xs = x.double() if real else torch.sign(x).double()
    z = (F.conv2d(xs, sw, padding=pad) + v(bias, 0.0)).float().double()
    y = (z - v(mean, 0.0)) * v(invstd, 1.0) * v(gamma, 1.0) + v(beta, 0.0)
    sabs = F.conv2d(xs.abs(), sw.abs(), padding=pad) + v(bias, 0.0).abs()
    tau = (4 * ((3 * w[0].numel() + 2) * U * sabs + 4 * U * (z.abs() + v(mean, 0.0).abs())) * (v(invstd, 1.0) * v(gamma, 1.0)).abs()
           + 4 * U * v(beta, 0.0).abs())
    h = F.hardtanh(y)
    return _tsign(F.max_pool2d(h, 2, 2) if pool else h), y, tau


def _planes(s, K2, pad2, nbytes):
    """int8 signs [N, Co, PH, PW] -> the consumer's FP4 planes, uint8 [nbytes], built in torch."""
    N, Co, PH, PW = s.shape
    code = torch.where(s > 0, 2, torch.where(s < 0, 10, 0)).to(torch.uint8)
    grid = torch.zeros((Co // 64, N, PH + 2 * pad2, PW + 2 * pad2, 64), dtype=torch.uint8)
    grid[:, :, pad2:pad2 + PH, pad2:pad2 + PW] = code.view(N, Co // 64, 64, PH, PW).permute(1, 0, 3, 4, 2)
    rows = torch.zeros((Co // 64, nbytes // (Co // 64 * 32), 64), dtype=torch.uint8)
    rows[:, :grid[0].numel() // 64] = grid.view(Co // 64, -1, 64)
    return (rows[..., 0::2] | (rows[..., 1::2] << 4)).reshape(-1)


def _unplanes(out, shape, pad2):
    """The interior of the planes back as int8 signs [N, Co, PH, PW]."""
    N, Co, PH, PW = shape
    rows = out.view(Co // 64, -1, 32)
    code = torch.stack((rows & 15, rows >> 4), dim=3).reshape(Co // 64, -1, 64)
    grid = code[:, :N * (PH + 2 * pad2) * (PW + 2 * pad2)].view(Co // 64, N, PH + 2 * pad2, PW + 2 * pad2, 64)
    code = grid[:, :, pad2:pad2 + PH, pad2:pad2 + PW].permute(1, 0, 4, 2, 3).reshape(N, Co, PH, PW)
    return (code == 2).to(torch.int8) - (code == 10).to(torch.int8)


@pytest.fixture(scope="module")
def L():
    from bnn_amd import _lib
    return _lib


def _run(L, case, tensors):
    """The entry on fp32 x and the latent weight; out pre-filled with 0xFF.  (rc, out on the CPU, (PH, PW))."""
    N, C, H, W, Co, KH, KW, pad, pool, cons = case
    dev = [None if t is None else t.cuda() for t in tensors]
    lib = L.lib()
    OH, OW = H + 2 * pad - KH + 1, W + 2 * pad - KW + 1
    PH, PW = (OH // 2, OW // 2) if pool else (OH, OW)
    K2, pad2 = cons or (0, 0)
    nb = max(int(lib.bnn_conv2d_wide_planes_bytes(N, Co, PH, PW, K2, K2, pad2)), 16) if cons else N * Co * PH * PW + GUARD
    out = torch.full((nb,), 0xFF, dtype=torch.uint8, device="cuda")
    rc = lib.bnn_conv2d_fwd_first_bnsign(*dev, out, N, C, H, W, Co, KH, KW, pad, pool, 0 if cons else 1, K2, K2, pad2,
                                         L.stream())
    torch.cuda.synchronize()
    return rc, out.cpu(), (PH, PW)


def _check_exact(L, case, tensors):
    N, C, H, W, Co, KH, KW, pad, pool, cons = case
    ref, y, _ = _reference(*tensors, pad, pool)
    print("min |y| outside the planted channels:", float(y[:, 2:].abs().min()), "zeros:", int((y[:, 0] == 0).sum()))
    assert float(y[:, 2:].abs().min()) >= 1e-3 and bool((y[:, 0] == 0).any())
    rc, out, _ = _run(L, case, tensors)
    assert rc == 0
    if cons is None:
        assert torch.equal(out[:ref.numel()].view(torch.int8).view(ref.shape), ref)
        assert bool((out[ref.numel():] == 0xFF).all())               # nothing beyond the tensor is written
    else:
        assert torch.equal(out, _planes(ref, *cons, out.numel()))    # interior, halo and tail, byte for byte


@pytest.mark.parametrize("case", CF.CASES, ids=str)
def test_fused_layer_equals_float64_reference(L, case):
    _check_exact(L, case, _inputs(case))


@pytest.mark.parametrize("case", CF.CASES, ids=str)
def test_randn_signs_outside_the_rounding_band(L, case):
    """Windows that hold an element with |y64| <= tau are left out: at most 0.5 % of a case's."""
    N, C, H, W, Co, KH, KW, pad, pool, cons = case
    tensors = _inputs(case, exact=False)
    ref, y, tau = _reference(*tensors, pad, pool)
    near = (y.abs() <= tau).float()
    skip = (F.max_pool2d(near, 2, 2) if pool else near) > 0
    print("windows left out:", int(skip.sum()), "of", skip.numel())
    assert float(skip.float().mean()) <= 0.005
    rc, out, _ = _run(L, case, tensors)
    assert rc == 0
    got = out[:ref.numel()].view(torch.int8).view(ref.shape) if cons is None else _unplanes(out, ref.shape, cons[1])
    assert torch.equal(got[~skip], ref[~skip])


def test_c_abi_nulls_empty_batch_and_refusal(L):
    case = CF.CASES[0]
    x, w, bias, mean, invstd, gamma, beta = _inputs(case)
    mean[0] = 0.0                                        # channel 0 without a bias: y == 0 wherever I == 0
    _check_exact(L, case, (x, w, None, mean, invstd, None, None))
    tensors = _inputs(case)
    rc, out, _ = _run(L, (0,) + case[1:], tensors)
    assert rc == 0 and bool((out == 0xFF).all())
    rc, out, _ = _run(L, case[:9] + ((3, 3),), tensors)  # a consumer with pad2 = K2: refused, nothing launched
    assert rc == -1 and bool((out == 0xFF).all())


def test_stack_with_a_real_first_block():
    import torch.nn as nn
    from bnn_amd import inference
    from bnn_amd.nn import BinarizeConv2d
    g = torch.Generator().manual_seed(5)
    ri = lambda lo, hi, n: torch.randint(lo, hi + 1, (n,), generator=g).float()
    blocks = []
    for C, Co, pool in ((3, 128, False), (128, 128, True), (128, 256, False)):
        conv, bn = BinarizeConv2d(C, Co, 3, padding=1), nn.BatchNorm2d(Co)
        with torch.no_grad():
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=g))
            conv.bias.copy_(ri(-8, 8, Co) / 2)
            bn.running_mean.copy_(ri(-16, 16, Co) / 8 + 1 / 16)
            bn.running_var.copy_(torch.rand(Co, generator=g) * 40 + 4)
            bn.weight.copy_((torch.rand(Co, generator=g) + 0.5) * (ri(0, 1, Co) * 2 - 1))
            bn.bias.copy_(ri(-2, 2, Co) / 8 * inference._invstd(bn.running_var, bn.eps) * bn.weight)
        blocks.append(nn.Sequential(conv, bn, nn.Hardtanh(), *([nn.MaxPool2d(2, 2)] if pool else [])))
    x = torch.randint(-16, 17, (2, 3, 16, 16), generator=g).float() / 8
    s, ymin = x, float("inf")
    for i, seq in enumerate(blocks):                     # the float64 reference, block by block
        conv, bn = seq[0], seq[1]
        s, y, _ = _reference(s, conv.weight.detach(), conv.bias.detach(), bn.running_mean,
                             inference._invstd(bn.running_var, bn.eps), bn.weight.detach(), bn.bias.detach(), 1,
                             len(seq) == 4, real=i == 0)
        ymin, s = min(ymin, float(y.abs().min())), s.float()
    assert ymin >= 1e-3
    with pytest.raises(ValueError):
        inference.freeze_conv_stack(blocks[1:], real_input=True)
    frozen = inference.freeze_conv_stack(blocks, real_input=True)
    assert torch.equal(frozen(x), s.to(torch.int8))      # the CPU path
    frozen.to("cuda")
    first, wide = inference.FIRST_FUSED_CALLS, inference.WIDE_FUSED_CALLS
    got = frozen(x.cuda()).cpu()
    assert inference.FIRST_FUSED_CALLS - first == 1 and inference.WIDE_FUSED_CALLS - wide == 2
    assert torch.equal(got, s.to(torch.int8))
    frozen.two_pass = True
    assert torch.equal(frozen(x.cuda()).cpu(), got) and inference.FIRST_FUSED_CALLS - first == 1
