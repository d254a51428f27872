"""The 4-plane (dW) FP6 GEMM with its FP4 operand loaded straight into registers on a full-size tile
(csrc/bnn_gemm6.hip, gemm_fp6_k's BREG instances selected by bnn_gemm_fp6_set_wide) against the
128 x 512 tile with B staged through LDS (bnn_gemm_fp6_set_half mode 0 with the new form off, which
tests/test_gpu_fp6.py holds against the float64 product of the decoded digits).

Only the way B's bytes reach the MFMA changes -- same fragments, same MFMAs, same order -- so C must
be torch.equal.  Mode 2 of the setter forces the form at shapes far below two rounds of tiles, so the
cases are the smallest where the loop can go wrong: one k-step (the prologue alone), 2 and 3 (the
ring wraps at two and at three stages), 5 (odd, longer than the ring), a panel buffer with more
k-steps than the GEMM runs (the panel stride differs from the step count), one to three tile rows,
and one and two tile columns (a 1024-column tile spans two panels; the second starts at panel 2).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K_MAX = 320
PANEL_EXTRA = 128          # columns of the wider panel buffer beyond K_MAX
DEFAULT = "gemm_fp6_k<2, 4, 2, 4, 2>"
WIDE = "gemm_fp6_k<1, 8, 2, 4, 2, 0, 2, 0, 0, 0, 1>"     # the 64 x 1024 tile, one wave row

K_CASES = [
    (64, 64),        # one k-step
    (128, 128),      # the two-stage ring wraps
    (192, 192),      # a three-stage ring wraps
    (320, 320),      # odd step count beyond the ring depth
    (192, 448),      # panels of 7 k-steps, 3 used
    (64, 448),       # ... and 1 used
]


@pytest.fixture(scope="module")
def F():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from bnn_amd import functional
    return functional


@pytest.fixture(scope="module")
def data(F):
    """x [384, 320] fp32 with per-row magnitudes over e^+-3 and ternary w [2048, 448], made once;
    every case takes leading rows / columns of them."""
    rng = np.random.default_rng(20240808)
    x = (rng.standard_normal((384, K_MAX)) * np.exp(rng.uniform(-3, 3, (384, 1)))).astype(np.float32)
    w = rng.integers(-1, 2, (2048, K_MAX + PANEL_EXTRA)).astype(np.float32)
    return torch.as_tensor(x).cuda(), torch.as_tensor(w).cuda()


def _operands(F, x, w, M, N, K, panel_k):
    """The 4-plane row operand of x[:M, :K] and the panels of w[:N] built for panel_k >= K columns."""
    op = F.quant6_rows(x[:M, :K].contiguous())
    assert op.Kp == K
    op.res = None
    w4, _ = F.sign_pack_fp4(w[:N, :panel_k].contiguous())
    P = F.fp4_panels(w4, N, panel_k)
    ks = P.numel() // (((N + 511) // 512) * 512 * 32)
    assert ks == panel_k // 64
    return op, P, ks


def _ref_and_wide(F, op, P, ks, M, N, expect):
    """C of the 128 x 512 LDS tile (half mode 0, the new form off) and of the forced new form, whose
    reported kernel must be `expect`."""
    from bnn_amd import _lib as L
    prev_half = L.lib().bnn_gemm_fp6_set_half(-1, 0.0)
    prev_wide = L.lib().bnn_gemm_fp6_set_wide(-1)
    try:
        L.call("bnn_gemm_fp6_set_half", 0, 0.0)
        L.call("bnn_gemm_fp6_set_wide", 0)
        assert L.lib().bnn_gemm_fp6_kernel_kr(M, N, op.Kp, 0).decode() == DEFAULT
        assert L.lib().bnn_gemm_fp6_instance(M, N, op.Kp, 0, 1).decode() == DEFAULT
        ref = F.gemm_fp6(op, None, N, panels=P, panel_ks=ks)
        L.call("bnn_gemm_fp6_set_half", 1, 0.0)
        L.call("bnn_gemm_fp6_set_wide", 2)
        name = L.lib().bnn_gemm_fp6_kernel_kr(M, N, op.Kp, 0).decode()
        assert name == expect, name
        inst = L.lib().bnn_gemm_fp6_instance(M, N, op.Kp, 0, 1).decode()     # the exact instance: both are their own label
        assert inst == expect, inst
        C = F.gemm_fp6(op, None, N, panels=P, panel_ks=ks)
        torch.cuda.synchronize()
    finally:
        L.call("bnn_gemm_fp6_set_half", prev_half, 0.0)
        L.call("bnn_gemm_fp6_set_wide", prev_wide)
    return ref, C


@pytest.mark.parametrize("K,panel_k", K_CASES)
@pytest.mark.parametrize("N", [1024, 2048])
@pytest.mark.parametrize("M", [64, 128, 192])
def test_wide_tile_b_in_registers_bit_identical(F, data, M, N, K, panel_k):
    x, w = data
    op, P, ks = _operands(F, x, w, M, N, K, panel_k)
    ref, C = _ref_and_wide(F, op, P, ks, M, N, WIDE)
    assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0
    assert torch.equal(C, ref)


def test_wide_tile_not_eligible_at_1536_columns(F, data):
    """N = 1536 is no multiple of the 1024-column tile: the forced mode still runs the default
    kernel, and C is what it was."""
    x, w = data
    op, P, ks = _operands(F, x, w, 128, 1536, 320, 320)
    ref, C = _ref_and_wide(F, op, P, ks, 128, 1536, DEFAULT)
    assert torch.equal(C, ref)


def test_wide_tile_propagates_nan(F, data):
    """A NaN in one block of A: exactly the output row that sums over it is NaN (as
    test_gemm_fp6_propagates_nan asks of the default kernel), and every other element equals the
    reference."""
    x, w = data
    M, N, K = 192, 2048, 320
    xn = x[:M, :K].clone()
    xn[77, 200] = float("nan")
    op, P, ks = _operands(F, xn, w, M, N, K, K)
    ref, C = _ref_and_wide(F, op, P, ks, M, N, WIDE)
    for out in (ref, C):
        isn = torch.isnan(out)
        assert bool(isn[77].all()) and int(isn.sum()) == N
    assert torch.equal(torch.nan_to_num(C, nan=0.0), torch.nan_to_num(ref, nan=0.0))


def test_wide_tile_default_mode_keeps_small_shapes_on_the_default_kernel(F):
    """Setter at 1 (the default): a small unsplit shape is far below two rounds of tiles."""
    from bnn_amd import _lib as L
    assert L.lib().bnn_gemm_fp6_set_wide(-1) == 1
    assert L.lib().bnn_gemm_fp6_set_half(-1, 0.0) == 1
    for M, N in ((64, 1024), (192, 2048), (128, 512)):
        assert L.lib().bnn_gemm_fp6_kernel_kr(M, N, 320, 0).decode() == DEFAULT
    assert L.lib().bnn_gemm_fp6_set_wide(3) != 0          # modes 0 .. 2 only
    assert L.lib().bnn_gemm_fp6_set_wide(-1) == 1


@pytest.mark.parametrize("wide", [1, 2])
def test_wide_tile_leaves_the_half_modes_alone(F, wide):
    """bnn_gemm_fp6_set_half at 0, 2 or 4 selects the kernels it selected before the new form
    existed, whatever the new setter says: the 128 x 512 tile at 0, the half tile at 2 and 4 on a
    grid of at least four half tiles per CU, the 128 x 512 tile below that; a residual-plane launch
    never takes the new form."""
    from bnn_amd import _lib as L
    prev_half = L.lib().bnn_gemm_fp6_set_half(-1, 0.0)
    prev_wide = L.lib().bnn_gemm_fp6_set_wide(-1)
    HALF = "gemm_fp6_k<1, 4, 2, 4, 2>"
    try:
        L.call("bnn_gemm_fp6_set_wide", wide)
        for mode, big, small in ((0, DEFAULT, DEFAULT), (2, HALF, DEFAULT), (4, HALF, DEFAULT)):
            L.call("bnn_gemm_fp6_set_half", mode, 0.0)
            for res in (0, 1):
                assert L.lib().bnn_gemm_fp6_kernel_kr(8192, 4096, 1024, res).decode() == big, (mode, res)
                assert L.lib().bnn_gemm_fp6_kernel_kr(128, 2048, 320, res).decode() == small, (mode, res)
        L.call("bnn_gemm_fp6_set_half", 1, 0.0)
        assert L.lib().bnn_gemm_fp6_kernel_kr(8192, 4096, 1024, 1).decode() == HALF
        assert L.lib().bnn_gemm_fp6_kernel_kr(128, 2048, 320, 1).decode() == DEFAULT
    finally:
        L.call("bnn_gemm_fp6_set_half", prev_half, 0.0)
        L.call("bnn_gemm_fp6_set_wide", prev_wide)
