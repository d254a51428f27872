"""CPU checks of the stride-2 wide-channel conv input gradient's decision function: which shapes
bnn_conv2d_bwd_data_wide_s2_ok takes, that the workspace and kernel queries agree with it, and that the stride-1
query goes on refusing these tuples.  No GPU: nothing here launches."""
import pytest

from test_conv_wide_s2_plan import CASES, REFUSED, full

# three windows of round_up(128 + 2 * 99 + 2, 32) = 352 rows and 25 x 64 weight rows: 84992 B, twice is beyond 160 KiB
ONE_STAGE = (1, 128, 5, 190, 80, 5, 5, 2, False)
GPU_CASES = CASES + [ONE_STAGE]


@pytest.fixture(scope="module")
def L():
    from bnn_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("case", GPU_CASES)
def test_gpu_cases_are_taken_conflict_free(L, case):
    shape = full(case)
    assert L.bnn_conv2d_bwd_data_wide_s2_ok(*shape) == 1
    assert L.bnn_conv2d_bwd_data_wide_s2_workspace(*case[:8]) > 0
    name = L.bnn_conv2d_bwd_data_wide_s2_kernel(*shape)
    assert name.startswith(b"conv_wide_bwd_data_s2_k<") and name.endswith(b" b128=4"), name
    assert L.bnn_conv2d_bwd_data_wide_ok(*shape) == 0 and L.bnn_conv2d_bwd_data_wide_kernel(*shape) == b""


@pytest.mark.parametrize("shape,_wide_ok", REFUSED)
def test_refusals(L, shape, _wide_ok):
    N, C, H, W, Co, KH, KW, stride, pad, dil, groups = shape
    assert L.bnn_conv2d_bwd_data_wide_s2_ok(*shape) == 0
    assert L.bnn_conv2d_bwd_data_wide_s2_kernel(*shape) == b""
    if stride == 2 and dil == groups == 1:       # the workspace query takes no such arguments
        assert L.bnn_conv2d_bwd_data_wide_s2_workspace(N, C, H, W, Co, KH, KW, pad) == 0


def test_table_reaches_both_instances(L):
    names = {L.bnn_conv2d_bwd_data_wide_s2_kernel(*full(c)).split()[0] for c in GPU_CASES}
    assert names == {b"conv_wide_bwd_data_s2_k<1>", b"conv_wide_bwd_data_s2_k<2>"}
    assert L.bnn_conv2d_bwd_data_wide_s2_kernel(*full(ONE_STAGE)) == b"conv_wide_bwd_data_s2_k<1> lds=84992 b128=4"


def test_stage_and_workspace_bytes(L):
    # 3x3, pad 1 on 32 x 32: Hp = 34, Hq = Wq = 17, mh = mw = 1, so Gh = Gw = 18 and a window is round_up(128 + 18 + 1,
    # 32) = 160 rows; a stage is 3 x 160 + 9 x 64 = 1056 rows of 32 B = 33792 B, and two of them are staged
    assert L.bnn_conv2d_bwd_data_wide_s2_kernel(256, 128, 32, 32, 256, 3, 3, 2, 1, 1, 1) == \
        b"conv_wide_bwd_data_s2_k<2> lds=67584 b128=4"
    # 1x1: no halo, one 128-row window per plane and 64 weight rows
    assert L.bnn_conv2d_bwd_data_wide_s2_kernel(256, 128, 32, 32, 256, 1, 1, 2, 0, 1, 1) == \
        b"conv_wide_bwd_data_s2_k<2> lds=28672 b128=4"
    # 8 x 8, pad 1: 2 x 6 x 6 = 72 positions -> one tile of 160 rows; 6 blocks x 3 planes of it, then 6 x 9 x 128 rows
    assert L.bnn_conv2d_bwd_data_wide_s2_workspace(2, 128, 8, 8, 96, 3, 3, 1) == 6 * 3 * 160 * 32 + 6 * 9 * 128 * 32
