"""Every conv kernel instance against the float64 oracle, over the case table of tests/conv_cases.py
(tests/test_conv_dispatch.py proves on the CPU that the table reaches every instance).

Three kinds of input per case:
* exact   -- every partial sum of y, dx, dw and db is exact in fp32 in any order (asserted by the
             generator), so the kernels must equal the reference element for element;
* one-hot -- for the bf16x3 and f32-MFMA backward kernels: dy with full 24-bit mantissas over 40
             binades against a one-tap weight (dx) or a one-pixel input (dw), so every output
             element is a single product and must equal the reference bit for bit -- this pins the
             second and third bf16 terms of the bf16x3 split, which a norm-wise bar cannot see;
* real    -- the parity tests' random inputs at the bars test_gpu_parity.py states: binarised
             forward bit-exact, fp32-input forward <= 1e-6 and gradients <= 1e-5 norm-wise.
"""
import numpy as np
import pytest
import torch

import conv_cases as CC
from conftest import rel_err

pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-5      # as tests/test_gpu_parity.py
FP_FWD_TOL = 1e-6

IDS = [CC.case_id(c) for c in CC.CASES]
ONEHOT_DX = [c for c in CC.CASES if CC.is_mma(c.data)]
ONEHOT_DW = [c for c in CC.CASES if CC.is_mma(c.filt)]


@pytest.fixture(scope="module")
def F():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from bnn_amd import functional
    return functional


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def run(F, c, x, w, b, dy):
    """Forward and backward through F.binary_conv2d under the case's switches, after checking that
    the dispatch takes the instances the case is in the table for.  Returns (y, dx, dw, db)."""
    from bnn_amd import _lib
    L = _lib.lib()
    popc = CC.set_switches(L, c)
    try:
        assert CC.query(L, c) == (c.fwd, c.data, c.filt)
        xt, wt = dev(x).requires_grad_(True), dev(w).requires_grad_(True)
        bt = dev(b).requires_grad_(True) if b is not None else None
        y = F.binary_conv2d(xt, wt, bt, bool(c.binarize), c.stride, c.pad, c.dil, c.groups)
        y.backward(dev(dy))
        return host(y), host(xt.grad), host(wt.grad), host(bt.grad) if bt is not None else None
    finally:
        CC.restore_switches(L, popc)


def assert_equal(what, c, got, want):
    bad = CC.first_mismatch(got, want)
    if bad:
        print(f"{CC.case_id(c)} {what}: {bad}")
    assert not bad, f"{what}: {bad}"


@pytest.mark.parametrize("c", CC.CASES, ids=IDS)
def test_exact_inputs_equal_the_reference(F, c):
    x, w, b, dy = CC.exact_inputs(c)
    y, dx, dw, db = run(F, c, x, w, b, dy)
    ry, rdx, rdw, rdb = CC.reference(c, x, w, b, dy)
    assert_equal(f"y ({c.fwd})", c, y, ry)
    assert_equal(f"dx ({c.data})", c, dx, rdx)
    assert_equal(f"dw ({c.filt})", c, dw, rdw)
    if c.bias:
        assert_equal(f"db ({c.filt})", c, db, rdb)


@pytest.mark.parametrize("c", ONEHOT_DX, ids=[CC.case_id(c) for c in ONEHOT_DX])
def test_onehot_weight_dx_is_a_shifted_copy_of_dy(F, c):
    x, w, b, dy = CC.onehot_dx_inputs(c)
    _, dx, _, _ = run(F, c, x, w, b, dy)
    rdx = CC.reference(c, x, w, b, dy)[1]
    assert np.count_nonzero(rdx) > 0
    assert_equal(f"dx ({c.data})", c, dx, rdx)


@pytest.mark.parametrize("c", ONEHOT_DW, ids=[CC.case_id(c) for c in ONEHOT_DW])
def test_onehot_input_dw_is_single_dy_elements(F, c):
    x, w, b, dy = CC.onehot_dw_inputs(c)
    _, _, dw, _ = run(F, c, x, w, b, dy)
    rdw = CC.reference(c, x, w, b, dy)[2]
    assert np.count_nonzero(rdw) > 0
    assert_equal(f"dw ({c.filt})", c, dw, rdw)


@pytest.mark.parametrize("c", CC.CASES, ids=IDS)
def test_real_inputs_meet_the_parity_bars(F, c):
    x, w, b, dy = CC.real_inputs(c)
    y, dx, dw, db = run(F, c, x, w, b, dy)
    ry, rdx, rdw, rdb = CC.reference(c, x, w, b, dy)
    if c.binarize:
        assert_equal(f"y ({c.fwd})", c, y, ry)
    else:
        err = rel_err(y, ry)
        print(f"{CC.case_id(c)} y ({c.fwd}): rel err {err:.3e}")
        assert err < FP_FWD_TOL
    errs = [(what, rel_err(got, want)) for what, got, want in
            (("dx", dx, rdx), ("dw", dw, rdw)) + ((("db", db, rdb),) if c.bias else ())]
    print(CC.case_id(c), " ".join(f"{what} {e:.3e}" for what, e in errs))
    for what, e in errs:
        assert e < GRAD_TOL, (what, e)


@pytest.mark.parametrize("binarize,C", [(True, 16), (False, 3)])
def test_empty_batch(F, binarize, C):
    """N = 0 through F.binary_conv2d: empty y and dx, zero dw and db (what torch returns)."""
    xt = torch.zeros((0, C, 9, 7), device="cuda", requires_grad=True)
    wt = torch.randn((5, C, 3, 3), device="cuda", requires_grad=True)
    bt = torch.randn((5,), device="cuda", requires_grad=True)
    y = F.binary_conv2d(xt, wt, bt, binarize, 1, 1, 1, 1)
    assert tuple(y.shape) == (0, 5, 9, 7)
    y.backward(torch.zeros_like(y))
    assert tuple(xt.grad.shape) == (0, C, 9, 7)
    assert tuple(wt.grad.shape) == (5, C, 3, 3) and not host(wt.grad).any()
    assert tuple(bt.grad.shape) == (5,) and not host(bt.grad).any()
