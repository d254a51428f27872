"""The wide-channel binary conv filter and bias gradient (csrc/bnn_conv_wide_bwd_filter.hip)
against torch.nn.grad.conv2d_weight(sign(x), dy) in float64 on the CPU, rounded once to fp32.  The inputs are
chosen so that every partial sum in any order is representable in fp32: the comparisons are bit for bit."""
import re

import pytest
import torch

import conv_wide_cases as CW
from test_gpu_conv_wide import SHAPES          # (N, C, H, W, Co, KH, KW, pad): the forward test's seven

pytestmark = pytest.mark.gpu
NO_DB = CW.NO_DB                               # SHAPES[3]; CW.NO_DB_NEW is the multi-pass shape run without db


def _inputs(shape, kind):
    """x as the forward test draws it.  dy "dense": integers in [-8, 8], sums below 8 * 5 * 33 * 34 < 2^24.
    dy "onehot": per output channel one random (n, oh, ow) holds a full-mantissa value, all else zero, so every
    dw element has at most one non-zero term +-v = +-(d1 + d2 + d3) and db[co] = v."""
    N, C, H, W, Co, KH, KW, pad = shape
    g = torch.Generator().manual_seed(N * 131 + C * 7 + Co)
    vals = torch.tensor([-1.5, -0.0, 0.0, 0.25])
    x = vals[torch.randint(0, 4, (N, C, H, W), generator=g)]
    x.view(-1)[::97] = float("nan")                      # tsign(NaN) = 0
    OH, OW = H + 2 * pad - KH + 1, W + 2 * pad - KW + 1
    if kind == "dense":
        return torch.randint(-8, 9, (N, Co, OH, OW), generator=g).float(), x
    v = torch.randn(Co, generator=g) * torch.exp2(torch.randint(-20, 21, (Co,), generator=g).float())
    assert bool((v.view(torch.int32) & 0xFF).ne(0).any())          # the third plane is exercised
    dy = torch.zeros(N, Co, OH * OW)
    dy[torch.randint(0, N, (Co,), generator=g), torch.arange(Co), torch.randint(0, OH * OW, (Co,), generator=g)] = v
    return dy.view(N, Co, OH, OW), x


def _reference(dy, x, wshape, pad):
    sx = torch.nan_to_num(torch.sign(x), nan=0.0).double()
    return torch.nn.grad.conv2d_weight(sx, wshape, dy.double(), padding=pad), dy.double().sum((0, 2, 3))


def _check_exactness(dy, x, wshape, pad, kind):
    """The pre-condition of the bit-for-bit comparison, from the reference itself."""
    if kind == "dense":                                  # every partial sum is an integer below 2^24
        aw, ab = _reference(dy.abs(), x.abs(), wshape, pad)
        assert float(aw.max()) < 2 ** 24 and float(ab.max()) < 2 ** 24
    else:                                                # at most one non-zero term per dw and db element
        nw, nb = _reference(dy.ne(0).float(), torch.ones_like(x), wshape, pad)
        assert int(nw.max()) <= 1 and int(nb.max()) <= 1


def _run_twice(shape, dy, x, rw, rb, with_db):
    """The entry on a fresh workspace, then on one filled with 0xFF with dw and db pre-filled: everything read is
    rewritten, not assumed; dw and db are overwritten."""
    from bnn_amd import _lib as L
    N, C, H, W, Co, KH, KW, pad = shape
    dyd, xd = dy.cuda(), x.cuda()
    ws = torch.empty(L.lib().bnn_conv2d_bwd_filter_wide_workspace(N, C, H, W, Co, KH, KW, pad), dtype=torch.uint8, device="cuda")
    dw = torch.empty(Co, C, KH, KW, device="cuda")
    db = torch.empty(Co, device="cuda") if with_db else None
    for fill in (False, True):
        if fill:
            ws.fill_(0xFF)
            dw.fill_(7.0)
            if db is not None:
                db.fill_(7.0)
        L.call("bnn_conv2d_bwd_filter_wide", dyd, xd, dw, db, N, C, H, W, Co, KH, KW, 1, pad, 1, 1, ws, ws.numel(),
               L.stream())
        assert torch.equal(dw.cpu(), rw)
        assert db is None or torch.equal(db.cpu(), rb)


@pytest.mark.parametrize("kind", ["dense", "onehot"])
@pytest.mark.parametrize("shape", CW.for_op("filt"))
def test_wide_filter_gradient_equals_float64_reference(shape, kind):
    N, C, H, W, Co, KH, KW, pad = shape
    dy, x = _inputs(shape, kind)
    rw, rb = (t.float() for t in _reference(dy, x, (Co, C, KH, KW), pad))
    assert bool(rw.ne(0).any()) and bool(rb.ne(0).any())
    _check_exactness(dy, x, (Co, C, KH, KW), pad, kind)
    _run_twice(shape, dy, x, rw, rb, with_db=shape is not NO_DB)


@pytest.mark.parametrize("kind", ["dense", "onehot"])
def test_null_db_on_a_multi_pass_shape(kind):
    """db = None on a row of three 64-column passes: pack_dy_k carries its row sum over the passes and then has
    nowhere to store it; dw is exact all the same."""
    shape = CW.NO_DB_NEW
    N, C, H, W, Co, KH, KW, pad = shape
    assert W + 2 * pad - KW + 1 > 128
    dy, x = _inputs(shape, kind)
    rw, rb = (t.float() for t in _reference(dy, x, (Co, C, KH, KW), pad))
    assert bool(rw.ne(0).any())
    _check_exactness(dy, x, (Co, C, KH, KW), pad, kind)
    _run_twice(shape, dy, x, rw, rb, with_db=False)


def test_empty_batch_writes_exact_zeros():
    """N = 0 at the C ABI, with small non-empty tensors as the input pointers (the entry refuses null): the
    reduce runs over no slices and no rows and writes zeros over all of dw and db."""
    from bnn_amd import _lib as L
    N, C, H, W, Co, KH, KW, pad = CW.EMPTY
    dy, x = torch.ones(16, device="cuda"), torch.ones(16, device="cuda")
    ws = torch.full((L.lib().bnn_conv2d_bwd_filter_wide_workspace(*CW.EMPTY),), 0xFF, dtype=torch.uint8, device="cuda")
    assert ws.numel() > 0
    dw = torch.full((Co, C, KH, KW), 7.0, device="cuda")
    db = torch.full((Co,), 7.0, device="cuda")
    rc = L.lib().bnn_conv2d_bwd_filter_wide(dy, x, dw, db, N, C, H, W, Co, KH, KW, 1, pad, 1, 1, ws, ws.numel(), L.stream())
    torch.cuda.synchronize()
    assert rc == 0 and bool((dw.view(torch.int32) == 0).all()) and bool((db.view(torch.int32) == 0).all())
    assert bool((ws == 0xFF).all())                      # nothing is packed


def test_a_shape_runs_several_k_slices_with_a_short_last_one():
    from bnn_amd import _lib as L
    N, C, H, W, Co, KH, KW, pad = SHAPES[1]
    f = {k: int(v) for k, v in re.findall(rb"(\w+)=(\d+)", L.lib().bnn_conv2d_bwd_filter_wide_kernel(N, C, H, W, Co, KH, KW, 1, pad, 1, 1))}
    assert f[b"splits"] > 1 and (f[b"splits"] - 1) * f[b"slice"] < f[b"pieces"] < f[b"splits"] * f[b"slice"]


@pytest.mark.parametrize("stride,short", [(1, 1), (2, 0)])
def test_short_workspace_and_refused_shape_launch_nothing(stride, short):
    from bnn_amd import _lib as L
    N, C, H, W, Co, KH, KW, pad = shape = SHAPES[0]
    dy, x = _inputs(shape, "dense")
    if stride == 2:
        dy = dy[:, :, ::2, ::2].contiguous()
    ws = torch.empty(L.lib().bnn_conv2d_bwd_filter_wide_workspace(N, C, H, W, Co, KH, KW, pad), dtype=torch.uint8, device="cuda")
    dw = torch.full((Co, C, KH, KW), 7.0, device="cuda")
    db = torch.full((Co,), 7.0, device="cuda")
    rc = L.lib().bnn_conv2d_bwd_filter_wide(dy.cuda(), x.cuda(), dw, db, N, C, H, W, Co, KH, KW, stride, pad, 1, 1, ws,
                                            ws.numel() - short, L.stream())
    torch.cuda.synchronize()
    assert rc == -1 and bool((dw == 7.0).all()) and bool((db == 7.0).all())
    err = L.lib().bnn_last_error()
    assert err.startswith(b"bnn_conv2d_bwd_filter_wide:") and (b"workspace" in err) == bool(short)


def test_module_takes_the_wide_filter_gradient(monkeypatch):
    """BinarizeConv2d(128, 96, 3, padding=1), forward and backward, with CONV_WIDE_BWD_FILTER on and off: only
    weight.grad and bias.grad change kernel, and both kernels meet the gradient bar of tests/test_gpu_parity.py
    (1e-5 norm-wise) against float64."""
    from bnn_amd import functional as BF
    from models.binarized_modules import BinarizeConv2d
    torch.manual_seed(11)
    conv = BinarizeConv2d(128, 96, 3, padding=1).cuda().train()
    x0 = torch.randn(2, 128, 10, 10, device="cuda")
    dy = torch.randn(2, 96, 10, 10, device="cuda")
    rw, rb = _reference(dy.cpu(), x0.cpu(), (96, 128, 3, 3), 1)
    got = {}
    for on in (True, False):
        monkeypatch.setattr(BF, "CONV_WIDE_BWD_FILTER", on)
        calls = BF.CONV_WIDE_BWD_FILTER_CALLS
        x = x0.clone().requires_grad_(True)
        conv.zero_grad()
        y = conv(x)
        y.backward(dy)
        torch.cuda.synchronize()
        assert BF.CONV_WIDE_BWD_FILTER_CALLS - calls == int(on)
        for name, grad, ref in (("weight", conv.weight.grad, rw), ("bias", conv.bias.grad, rb)):
            err = float((grad.cpu().double() - ref).norm() / ref.norm())
            print(f"CONV_WIDE_BWD_FILTER={on}: {name}.grad rel err {err:.3e}")
            assert err < 1e-5
        got[on] = (y.detach(), x.grad.clone())
    for a, b in zip(got[True], got[False]):
        assert torch.equal(a, b)
