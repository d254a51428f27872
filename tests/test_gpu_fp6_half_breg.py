"""The half-tile FP6 GEMM with its FP4 operand loaded straight into registers (csrc/bnn_gemm6.hip,
gemm_fp6_k's BREG instances: bnn_gemm_fp6_set_half modes 1 / 2 on a panel operand) against the same
half tile with B staged through LDS (modes 3 / 4) and the 128 x 512 tile (mode 0, which
tests/test_gpu_fp6.py holds against the float64 product of the decoded digits).

Only the way B's bytes reach the MFMA changes -- same fragments, same MFMAs, same order -- so C must
be torch.equal across the three, with and without the residual plane.  Shapes: the half form takes
M % 64 == 0, N % 512 == 0 and >= 4 tiles per CU, so M = 8192 (and 8256: an odd number of tile rows)
by N = 4096 with a small K.  The K values are where the register path's ring and counted waits can
go wrong: one k-step (the prologue alone), 2 and 3 (the ring wraps at two and at three stages), 5
(odd, longer than the ring), and a panel buffer with more k-steps than the GEMM runs (the panel
stride differs from the step count).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 4096
K_MAX = 320
PANEL_EXTRA = 128          # columns of the wider panel buffer beyond K_MAX
# (bnn_gemm_fp6_set_half mode, residual plane) -> the exact instance bnn_gemm_fp6_instance must report:
# the labels cannot tell the three half-tile forms apart
INSTANCE = {
    (0, False): "gemm_fp6_k<2, 4, 2, 4, 2>",                              # the 128 x 512 tile
    (0, True): "gemm_fp6_k<2, 4, 2, 4, 2, 0, 2, 0, 0, 1>",
    (4, False): "gemm_fp6_k<1, 4, 2, 4, 2>",                              # the half tile, B through LDS
    (4, True): "gemm_fp6_k<1, 4, 2, 4, 2, 0, 2, 0, 0, 1>",
    (2, False): "gemm_fp6_k<1, 4, 2, 4, 2, 0, 2, 0, 0, 0, 1>",            # the half tile, B in registers
    (2, True): "gemm_fp6_k<1, 4, 2, 4, 2, 0, 2, 0, 0, 1, 1>",
}


@pytest.fixture(scope="module")
def F():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from bnn_amd import functional
    return functional


@pytest.fixture(scope="module")
def data(F):
    """x [8256, 320] fp32 with per-row magnitudes over e^+-3 and ternary w [4096, 448], made once;
    every case takes leading rows / columns of them."""
    rng = np.random.default_rng(20240607)
    x = (rng.standard_normal((8256, K_MAX)) * np.exp(rng.uniform(-3, 3, (8256, 1)))).astype(np.float32)
    w = rng.integers(-1, 2, (N, K_MAX + PANEL_EXTRA)).astype(np.float32)
    return torch.as_tensor(x).cuda(), torch.as_tensor(w).cuda()


def _operands(F, x, w, M, K, panel_k):
    """The row operand of x[:M, :K] and w's panels built for panel_k >= K columns."""
    op = F.quant6_rows(x[:M, :K].contiguous())
    assert op.Kp == K and op.res is not None
    w4, _ = F.sign_pack_fp4(w[:, :panel_k].contiguous())
    P = F.fp4_panels(w4, N, panel_k)
    ks = P.numel() // ((N // 512) * 512 * 32)
    assert ks == panel_k // 64
    return op, P, ks


def _three_modes(F, op, P, ks, M, res, stagger=0.0):
    """C of the 128 x 512 tile, the half tile with B through LDS and the half tile with B in registers."""
    from bnn_amd import _lib as L
    if not res:
        op.res = None
    prev = L.lib().bnn_gemm_fp6_set_half(-1, 0.0)
    outs = {}
    try:
        for mode in (0, 4, 2):
            L.call("bnn_gemm_fp6_set_half", mode, stagger if mode else 0.0)
            name = L.lib().bnn_gemm_fp6_kernel_kr(M, N, op.Kp, int(res)).decode()
            assert ("<1, 4, 2, 4, 2>" in name) == (mode > 0), (mode, name)
            inst = L.lib().bnn_gemm_fp6_instance(M, N, op.Kp, int(res), 1).decode()
            assert inst == INSTANCE[mode, bool(res)], (mode, inst)
            outs[mode] = F.gemm_fp6(op, None, N, panels=P, panel_ks=ks)
        torch.cuda.synchronize()
    finally:
        L.call("bnn_gemm_fp6_set_half", prev, 0.0)
    return outs


@pytest.mark.parametrize("res", [True, False])
@pytest.mark.parametrize("M,K,panel_k,stagger", [
    (8192, 64, 64, 0.0),        # one k-step
    (8192, 128, 128, 0.0),      # the two-stage ring wraps
    (8192, 192, 192, 0.0),      # the three-stage ring wraps
    (8192, 320, 320, 0.0),      # odd step count beyond the ring depth
    (8256, 320, 320, 0.0),      # 129 tile rows
    (8192, 192, 448, 0.0),      # panels of 7 k-steps, 3 used
    (8192, 64, 448, 0.0),       # ... and 1 used
    (8192, 320, 320, 60.0),     # first-round stagger
])
def test_half_tile_b_in_registers_bit_identical(F, data, M, K, panel_k, stagger, res):
    x, w = data
    op, P, ks = _operands(F, x, w, M, K, panel_k)
    outs = _three_modes(F, op, P, ks, M, res, stagger)
    assert bool(torch.isfinite(outs[0]).all()) and float(outs[0].abs().max()) > 0
    assert torch.equal(outs[4], outs[0]), "half tile, B through LDS"
    assert torch.equal(outs[2], outs[0]), "half tile, B in registers"


@pytest.mark.parametrize("res", [True, False])
def test_half_tile_b_in_registers_propagates_nan(F, data, res):
    """A NaN in one block of A: exactly the output rows that sum over it are NaN (as
    test_gemm_fp6_propagates_nan asks of the default kernel), in all three forms, and every other
    element equal across them."""
    x, w = data
    M, K = 8192, 320
    xn = x[:M, :K].clone()
    xn[4177, 200] = float("nan")
    op, P, ks = _operands(F, xn, w, M, K, K)
    outs = _three_modes(F, op, P, ks, M, res)
    for mode, C in outs.items():
        isn = torch.isnan(C)
        assert bool(isn[4177].all()) and int(isn.sum()) == N, mode
    ref = torch.nan_to_num(outs[0], nan=0.0)
    assert torch.equal(torch.nan_to_num(outs[4], nan=0.0), ref)
    assert torch.equal(torch.nan_to_num(outs[2], nan=0.0), ref)
