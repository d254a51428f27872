"""The training hand-off between two wide conv layers (csrc/bnn_conv_wide_handoff.hip and the two consumer entries,
DESIGN.md §25) against float64 on the CPU.

The inputs make every sign decidable.  z is integer-valued, gamma is in +-[0.5, 2] and beta puts y = 0 at k + 0.5
for an integer k (from the float64 statistics), so y = (z - k - 0.5) invstd gamma and |y| >= 0.25 invstd, four
orders above fp32's rounding; each case asserts its own min |y| >= 0.01 outside the planted channels: channel
0 has gamma = beta = 0 (y == 0, code 0) and channel 1 a NaN gamma (code 0).  Without gamma and beta y has the
sign of z - mean, and the mean of n integers is an integer (exact in fp32 too) or at least 1 / n off one.  Sums of
ternary products with integer bias or small-integer dy are exact in fp32, so those results are compared with
torch.equal; planes are compared over the whole 0xFF-prefilled buffer, halo and tail included."""
import functools

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from test_conv_wide_handoff_plan import CASES

pytestmark = pytest.mark.gpu
MOM, EPS = 0.1, 1e-5


def _affine(z, g):
    """(gamma, beta) fp32 [C] for the integer-valued z [N, C, H, W] as the module docstring describes."""
    C = z.shape[1]
    mean, var = z.double().mean((0, 2, 3)), z.double().var((0, 2, 3), unbiased=False)
    gamma = (torch.rand(C, generator=g, dtype=torch.float64) * 1.5 + 0.5) * (torch.randint(0, 2, (C,), generator=g) * 2 - 1)
    k = torch.round(mean) + torch.randint(-5, 5, (C,), generator=g)
    beta = -(k + 0.5 - mean) * gamma / torch.sqrt(var + EPS)
    return gamma.float(), beta.float()


def _signs(z, gamma, beta, pool):
    """float64 reference: (int8 signs [N, C, PH, PW] by the window rule, y, mean, biased var)."""
    zd = z.double()
    mean, var = zd.mean((0, 2, 3)), zd.var((0, 2, 3), unbiased=False)
    v = lambda t, none: none if t is None else t.double().view(1, -1, 1, 1)
    y = (zd - v(mean, 0)) / torch.sqrt(v(var, 0) + EPS) * v(gamma, 1.0) + v(beta, 0.0)
    any_ = (lambda m: F.max_pool2d(m.double(), 2, 2) > 0) if pool else (lambda m: m)
    pos, zero, nan = any_(y > 0), any_(y == 0), any_(y != y)
    s = torch.where(nan, 0, torch.where(pos, 1, torch.where(zero, 0, -1))).to(torch.int8)
    return s, y, mean, var


def _planes(s, pad, nbytes):
    """int8 signs [N, C, PH, PW] -> the consumer's FP4 planes, uint8 [nbytes] (bnn.h, "planes")."""
    N, C, PH, PW = s.shape
    code = torch.where(s > 0, 2, torch.where(s < 0, 10, 0)).to(torch.uint8)
    grid = torch.zeros((C // 64, N, PH + 2 * pad, PW + 2 * pad, 64), dtype=torch.uint8)
    grid[:, :, pad:pad + PH, pad:pad + PW] = code.view(N, C // 64, 64, PH, PW).permute(1, 0, 3, 4, 2)
    rows = torch.zeros((C // 64, nbytes // (C // 64 * 32), 64), dtype=torch.uint8)
    rows[:, :grid[0].numel() // 64] = grid.view(C // 64, -1, 64)
    return (rows[..., 0::2] | (rows[..., 1::2] << 4)).reshape(-1)


@pytest.fixture(scope="module")
def L():
    from bnn_amd import _lib
    return _lib


def _apply(L, z, gamma, beta, pool, K, pad, rm, rv):
    """bnn_bn2d_fwd_train_planes on the GPU: (rc, planes prefilled with 0xFF, save_mean, save_invstd)."""
    N, C, H, W = z.shape
    lib = L.lib()
    PH, PW = (H // 2, W // 2) if pool else (H, W)
    planes = torch.full((lib.bnn_conv2d_wide_planes_bytes(N, C, PH, PW, K, K, pad),), 0xFF, dtype=torch.uint8, device="cuda")
    mean, invstd = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    ws = torch.empty(lib.bnn_bn2d_workspace(N, C), dtype=torch.uint8, device="cuda")
    rc = lib.bnn_bn2d_fwd_train_planes(z, N, C, H, W, gamma, beta, rm, rv, MOM, EPS, mean, invstd, planes, pool, K, K,
                                       pad, ws, L.stream())
    return rc, planes, mean, invstd


@functools.lru_cache(maxsize=None)
def _case(L, case):
    """Inputs, float64 reference and the planes kernel's outputs of one case, computed once for its tests."""
    N, C, H, W, pool, K, pad, Co = case
    g = torch.Generator().manual_seed(sum(case) * 31 + C)
    z = torch.randint(-8, 9, (N, C, H, W), generator=g).float()
    gamma, beta = _affine(z, g)
    gamma[0], beta[0], gamma[1] = 0.0, 0.0, float("nan")
    s, y, mean, var = _signs(z, gamma, beta, pool)
    assert y[:, 2:].abs().min() >= 0.01
    rm, rv = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    d = dict(s=s, mean=mean, var=var, rm0=rm, rv0=rv, zd=z.cuda(), ga=gamma.cuda(), be=beta.cuda(), rm=rm.cuda(), rv=rv.cuda())
    d["rc"], d["planes"], d["save_mean"], d["save_invstd"] = _apply(L, d["zd"], d["ga"], d["be"], pool, K, pad, d["rm"], d["rv"])
    d["w"] = torch.tensor([-1.5, -0.0, 0.0, 0.25, 2.0])[torch.randint(0, 5, (Co, C, K, K), generator=g)]
    return d


@pytest.mark.parametrize("case", CASES[:5])
def test_planes_and_statistics(L, case):
    N, C, H, W, pool, K, pad, Co = case
    d = _case(L, case)
    assert d["rc"] == 0
    assert torch.equal(d["planes"].cpu(), _planes(d["s"], pad, d["planes"].numel()))
    n = N * H * W
    running = lambda r0, new: (1 - MOM) * r0.double() + MOM * new
    tt = torch.testing.assert_close
    tt(d["save_mean"].cpu().double(), d["mean"], rtol=1e-5, atol=1e-6)
    tt(d["save_invstd"].cpu().double(), 1 / torch.sqrt(d["var"] + EPS), rtol=1e-5, atol=0)
    tt(d["rm"].cpu().double(), running(d["rm0"], d["mean"]), rtol=1e-5, atol=1e-6)
    tt(d["rv"].cpu().double(), running(d["rv0"], d["var"] * n / (n - 1)), rtol=1e-5, atol=1e-6)
    # no gamma, no beta, no running statistics
    rc, planes, _, _ = _apply(L, d["zd"], None, None, pool, K, pad, None, None)
    assert rc == 0 and torch.equal(planes.cpu(), _planes(_signs(d["zd"].cpu(), None, None, pool)[0], pad, planes.numel()))


@pytest.mark.parametrize("case", CASES[:5])
def test_forward_from_planes(L, case):
    N, C, H, W, pool, K, pad, Co = case
    d, lib = _case(L, case), L.lib()
    PH, PW = d["s"].shape[2:]
    bias = torch.arange(Co).float() % 7 - 3
    ref = F.conv2d(d["s"].double(), torch.sign(d["w"]).double(), bias.double(), padding=pad)
    y = torch.full(ref.shape, float("nan"), device="cuda")
    ws = torch.empty(lib.bnn_conv2d_fwd_wide_planes_workspace(N, C, PH, PW, Co, K, K, pad), dtype=torch.uint8, device="cuda")
    L.call("bnn_conv2d_fwd_wide_planes", d["planes"], d["w"].cuda(), bias.cuda(), y, N, C, PH, PW, Co, K, K, pad, ws,
           ws.numel(), L.stream())
    assert torch.equal(y.cpu().double(), ref)


@pytest.mark.parametrize("case", CASES[:5])
def test_filter_gradient_from_planes(L, case):
    N, C, H, W, pool, K, pad, Co = case
    d, lib = _case(L, case), L.lib()
    PH, PW = d["s"].shape[2:]
    OH, OW = PH + 2 * pad - K + 1, PW + 2 * pad - K + 1
    g = torch.Generator().manual_seed(Co + N)
    ws = torch.empty(lib.bnn_conv2d_bwd_filter_wide_workspace(N, C, PH, PW, Co, K, K, pad), dtype=torch.uint8, device="cuda")
    for dy, exact in ((torch.randint(-3, 4, (N, Co, OH, OW), generator=g).float(), True),
                      (torch.randn(N, Co, OH, OW, generator=g), False)):
        dw, db = torch.full((Co, C, K, K), float("nan"), device="cuda"), torch.full((Co,), float("nan"), device="cuda")
        L.call("bnn_conv2d_bwd_filter_wide_planes", dy.cuda(), d["planes"], dw, db, N, C, PH, PW, Co, K, K, 1, pad, 1, 1,
               ws, ws.numel(), L.stream())
        dw_ref = torch.nn.grad.conv2d_weight(d["s"].double(), dw.shape, dy.double(), padding=pad)
        db_ref = dy.double().sum((0, 2, 3))
        if exact:
            assert torch.equal(dw.cpu().double(), dw_ref) and torch.equal(db.cpu().double(), db_ref)
        else:
            assert rel_err(dw.cpu(), dw_ref) < 1e-5 and rel_err(db.cpu(), db_ref) < 1e-5


def test_empty_batch(L):
    """N == 0 at the C ABI: the two forward entries return 0 and write nothing, the filter gradient is zero."""
    N, C, H, W, pool, K, pad, Co = CASES[5]
    lib, shape = L.lib(), (N, C, H // 2, W // 2, Co, K, K)
    z = y = torch.zeros(4, device="cuda")         # never read or written: an empty tensor's pointer is null
    planes = torch.full((lib.bnn_conv2d_wide_planes_bytes(*shape[:4], K, K, pad),), 0xFF, dtype=torch.uint8, device="cuda")
    ws = torch.empty(max(lib.bnn_conv2d_fwd_wide_planes_workspace(*shape, pad), lib.bnn_conv2d_bwd_filter_wide_workspace(*shape, pad),
                         lib.bnn_bn2d_workspace(N, C)), dtype=torch.uint8, device="cuda")
    mean, invstd = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    L.call("bnn_bn2d_fwd_train_planes", z, N, C, H, W, None, None, None, None, MOM, EPS, mean, invstd, planes, pool, K, K,
           pad, ws, L.stream())
    w = torch.ones(Co, C, K, K, device="cuda")
    L.call("bnn_conv2d_fwd_wide_planes", planes, w, None, y, *shape, pad, ws, ws.numel(), L.stream())
    assert planes.numel() > 0 and bool((planes == 0xFF).all()) and not y.any()
    dw, db = torch.full_like(w, float("nan")), torch.full((Co,), float("nan"), device="cuda")
    L.call("bnn_conv2d_bwd_filter_wide_planes", y, planes, dw, db, *shape, 1, pad, 1, 1, ws, ws.numel(), L.stream())
    assert not dw.any() and not db.any()


@pytest.mark.parametrize("case", CASES[:2])
def test_blocks_end_to_end(L, case, monkeypatch):
    """nets.conv_blocks_forward on two blocks, forward and backward, against the same blocks in float64 torch."""
    import torch.nn as nn
    from bnn_amd import functional as BF, nets
    from bnn_amd.nn import BinarizeConv2d
    N, C, H, W, pool, K, pad, Co = case
    torch.manual_seed(sum(case))
    tail = [nn.MaxPool2d(2, 2)] if pool else []
    blocks = [nn.Sequential(BinarizeConv2d(64, C, 3, padding=1), nn.BatchNorm2d(C), nn.Hardtanh(), *tail),
              nn.Sequential(BinarizeConv2d(C, Co, K, padding=pad), nn.BatchNorm2d(Co), nn.Hardtanh())]
    x = torch.randn(N, 64, H, W)
    with torch.no_grad():
        for seq in blocks:
            nets._configure(seq, org_protocol=False, mutate_input=False)
            seq[0].bias.copy_(torch.randint(-3, 4, seq[0].bias.shape).float())
            seq[1].weight.copy_(torch.rand(seq[1].weight.shape) + 0.5)
        z1_ref = F.conv2d(torch.sign(x).double(), torch.sign(blocks[0][0].weight).double(), blocks[0][0].bias.double(), padding=1)
        gamma, beta = (2 * t for t in _affine(z1_ref, torch.Generator().manual_seed(1)))     # |y| >= 0.5 invstd
        blocks[0][1].weight.copy_(gamma), blocks[0][1].bias.copy_(beta)
    assert _signs(z1_ref, gamma, beta, pool)[1].abs().min() >= 0.01
    G = torch.randn(N, Co, *((H // 2, W // 2) if pool else (H, W)))

    # float64: sign with a straight-through gradient, on the activations and on the weights
    ste = lambda t: t + (torch.sign(t) - t).detach()
    (w1, b1, g1, e1), (w2, b2, g2, e2) = ([t.detach().double().requires_grad_() for t in
                                           (seq[0].weight, seq[0].bias, seq[1].weight, seq[1].bias)] for seq in blocks)
    z1 = F.conv2d(torch.sign(x).double(), ste(w1), b1, padding=1)
    z1.retain_grad()
    a = F.hardtanh(F.batch_norm(z1, None, None, g1, e1, True, MOM, EPS))
    z2_ref = F.conv2d(ste(F.max_pool2d(a, 2, 2) if pool else a), ste(w2), b2, padding=pad)
    z2_ref.retain_grad()
    out_ref = F.hardtanh(F.batch_norm(z2_ref, None, None, g2, e2, True, MOM, EPS))
    (out_ref * G.double()).sum().backward()

    for seq in blocks:
        seq.cuda().train()
    seen = []
    hook = blocks[0][0].register_forward_hook(lambda m, i, o: o.retain_grad() or seen.append(o))
    calls = BF.CONV_WIDE_HANDOFF_CALLS
    monkeypatch.setattr(BF, "CONV_WIDE_HANDOFF", True)     # every transition the queries accept, not only the measured classes
    out = nets.conv_blocks_forward(blocks, x.cuda())
    assert BF.CONV_WIDE_HANDOFF_CALLS == calls + 1
    (out * G.cuda()).sum().backward()
    hook.remove()
    got = [seen[0].grad, blocks[0][1].weight.grad, blocks[0][1].bias.grad, blocks[1][0].weight.grad]
    want = [z1.grad, g1.grad, e1.grad, w2.grad]
    assert rel_err(out.detach().cpu(), out_ref.detach()) < 1e-5
    for name, a_, b_ in zip(("dz", "dgamma", "dbeta", "dw"), got, want):
        assert rel_err(a_.cpu(), b_) < 1e-5, name
    # db is the sum of a BatchNorm's input gradient, zero in exact arithmetic: the 1e-5 is taken relative to the
    # terms of the sum, sum |dz2| per channel, not to the cancelled value
    db_err = (blocks[1][0].bias.grad.cpu().double() - b2.grad).norm()
    assert db_err <= 1e-5 * z2_ref.grad.abs().sum((0, 2, 3)).norm(), "db"
    # the hand-off's own output is exact: integer sums plus an integer bias
    z2 = BF.bn2d_hardtanh_pool_binary_conv2d(seen[0].detach(), blocks[0][1], blocks[1][0], pool)
    assert torch.equal(z2.detach().cpu().double(), z2_ref.detach())
    # switched off: today's chain, the same bits, and the counter stays
    calls = BF.CONV_WIDE_HANDOFF_CALLS
    monkeypatch.setattr(BF, "CONV_WIDE_HANDOFF", False)
    chain = nets.conv_blocks_forward(blocks, x.cuda())
    assert BF.CONV_WIDE_HANDOFF_CALLS == calls and torch.equal(chain, out)

