"""CPU checks of the stride-2 wide-channel conv forward's decision function: which shapes
bnn_conv2d_fwd_wide_s2_ok takes, that the workspace and kernel queries agree with it, and that the stride-1
query answers these tuples as before.  No GPU: nothing here launches."""
import pytest

# (N, C, H, W, Co, KH, KW, pad, bias): the shapes tests/test_gpu_conv_wide_s2.py runs, and what each pins
CASES = [
    (2, 128, 8, 8, 128, 3, 3, 1, True),        # base case: 2 blocks, <2>, 4 phases, Hp even
    (3, 64, 7, 9, 136, 3, 3, 1, False),        # one block, odd Hp and Wp, a Co tail, tiles that cross images
    (2, 256, 8, 8, 72, 3, 3, 0, True),         # four blocks, pad 0 with an unused last row / column, Co < 128
    (2, 128, 9, 8, 200, 1, 1, 0, True),        # one phase, zero shift, odd H
    (1, 128, 10, 12, 128, 5, 5, 2, True),      # <1>, shifts of two rows / columns
    (2, 128, 6, 11, 128, 3, 5, 1, False),      # non-square kernel, pad < KW - 1
    (1, 128, 4, 133, 128, 1, 3, 1, True),      # nph = 2 (KH = 1), more than two 64-column pack passes
    (5, 128, 16, 16, 128, 3, 3, 1, True),      # several position tiles per image and a last partial tile
]

# (N, C, H, W, Co, KH, KW, stride, pad, dil, groups), and bnn_conv2d_fwd_wide_ok's answer
REFUSED = [
    ((2, 128, 8, 8, 128, 3, 3, 1, 1, 1, 1), 1),         # stride 1: §19's
    ((2, 128, 8, 8, 128, 3, 3, 3, 1, 1, 1), 0),         # stride 3
    ((2, 128, 8, 8, 128, 3, 3, 2, 1, 2, 1), 0),         # dilation
    ((2, 128, 8, 8, 128, 3, 3, 2, 1, 1, 2), 0),         # groups
    ((2, 96, 8, 8, 128, 3, 3, 2, 1, 1, 1), 0),          # C % 64
    ((2, 64, 8, 8, 64, 3, 3, 2, 1, 1, 1), 0),           # C = Co = 64
    ((2, 128, 8, 8, 128, 3, 3, 2, 3, 1, 1), 0),         # pad = K
    ((1, 128, 8, 2000, 128, 3, 3, 2, 1, 1, 1), 0),      # four 1152-row phase windows are beyond the LDS
]


def full(case):
    N, C, H, W, Co, KH, KW, pad, _ = case
    return (N, C, H, W, Co, KH, KW, 2, pad, 1, 1)


@pytest.fixture(scope="module")
def L():
    from bnn_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("case", CASES)
def test_gpu_cases_are_taken_conflict_free(L, case):
    shape = full(case)
    assert L.bnn_conv2d_fwd_wide_s2_ok(*shape) == 1
    assert L.bnn_conv2d_fwd_wide_s2_workspace(*case[:8]) > 0
    name = L.bnn_conv2d_fwd_wide_s2_kernel(*shape)
    assert name.startswith(b"conv_wide_gemm_s2_k<") and b" b128=4 " in name, name
    assert L.bnn_conv2d_fwd_wide_ok(*shape) == 0 and L.bnn_conv2d_fwd_wide_kernel(*shape) == b""


@pytest.mark.parametrize("shape,wide_ok", REFUSED)
def test_refusals(L, shape, wide_ok):
    N, C, H, W, Co, KH, KW, stride, pad, dil, groups = shape
    assert L.bnn_conv2d_fwd_wide_s2_ok(*shape) == 0
    assert L.bnn_conv2d_fwd_wide_s2_kernel(*shape) == b""
    if stride == 2 and dil == groups == 1:       # the workspace query takes no such arguments
        assert L.bnn_conv2d_fwd_wide_s2_workspace(N, C, H, W, Co, KH, KW, pad) == 0
    assert L.bnn_conv2d_fwd_wide_ok(*shape) == wide_ok


def test_table_reaches_both_instances_and_every_phase_count(L):
    names = [L.bnn_conv2d_fwd_wide_s2_kernel(*full(c)).decode().split() for c in CASES]
    assert {n[0] for n in names} == {"conv_wide_gemm_s2_k<1>", "conv_wide_gemm_s2_k<2>"}
    assert {n[3] for n in names} == {"nph=1", "nph=2", "nph=4"}


def test_stage_and_workspace_bytes(L):
    # 3x3, pad 1 on 32 x 32: Wq = 17, four windows of 160 rows and 9 x 128 weight rows, twice
    assert L.bnn_conv2d_fwd_wide_s2_kernel(256, 128, 32, 32, 256, 3, 3, 2, 1, 1, 1) == \
        b"conv_wide_gemm_s2_k<2> lds=114688 b128=4 nph=4"
    assert L.bnn_conv2d_fwd_wide_s2_kernel(256, 128, 32, 32, 256, 5, 5, 2, 2, 1, 1).startswith(
        b"conv_wide_gemm_s2_k<1> lds=126976 ")
    assert L.bnn_conv2d_fwd_wide_s2_kernel(256, 128, 32, 32, 256, 1, 1, 2, 0, 1, 1).startswith(
        b"conv_wide_gemm_s2_k<2> lds=16384 ")
    # 2 blocks x 4 phases x (2*5*5 = 50 -> 128 positions - 128 + the 160-row window) x 32 B, then 2 x 9 x 128 rows
    assert L.bnn_conv2d_fwd_wide_s2_workspace(2, 128, 8, 8, 96, 3, 3, 1) == 2 * 4 * 160 * 32 + 2 * 9 * 128 * 32
