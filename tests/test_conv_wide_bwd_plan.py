"""CPU checks of the wide-channel conv input gradient's decision function, over the
forward plan test's shapes: the three queries agree, the set lies inside the forward's, the fragment
reads are conflict-free, and the dispatch of bnn_conv2d_bwd_data is untouched.  Nothing here launches."""
import pytest

from test_conv_wide_plan import SHAPES


@pytest.fixture(scope="module")
def L():
    from bnn_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("shape,ok", SHAPES)
def test_ok_workspace_and_kernel_agree(L, shape, ok):
    N, C, H, W, Co, KH, KW, stride, pad, dil, groups = shape
    assert L.bnn_conv2d_bwd_data_wide_ok(*shape) == ok      # every listed forward shape fits the backward stage
    assert L.bnn_conv2d_fwd_wide_ok(*shape) >= L.bnn_conv2d_bwd_data_wide_ok(*shape)
    name = L.bnn_conv2d_bwd_data_wide_kernel(*shape)
    assert (name != b"") == bool(ok)
    if stride == dil == groups == 1:      # the workspace query takes no such arguments
        assert (L.bnn_conv2d_bwd_data_wide_workspace(N, C, H, W, Co, KH, KW, pad) > 0) == bool(ok)
    if ok:
        assert name.startswith(b"conv_wide_bwd_data_k<") and name.endswith(b" b128=4"), name


def test_three_windows_take_less_than_the_forward(L):
    shape = (1, 128, 8, 700, 128, 3, 3, 1, 1, 1, 1)         # (3 * 1536 + 1152) * 32 B = 180 KiB
    assert L.bnn_conv2d_fwd_wide_ok(*shape) == 1 and L.bnn_conv2d_bwd_data_wide_ok(*shape) == 0
    assert L.bnn_conv2d_bwd_data_wide_kernel(*shape) == b""
    assert L.bnn_conv2d_bwd_data_wide_workspace(1, 128, 8, 700, 128, 3, 3, 1) == 0


def test_double_buffer_where_it_fits(L):
    assert L.bnn_conv2d_bwd_data_wide_kernel(256, 128, 32, 32, 128, 3, 3, 1, 1, 1, 1) == \
        b"conv_wide_bwd_data_k<2> lds=116736 b128=4"
    assert L.bnn_conv2d_bwd_data_wide_kernel(256, 512, 8, 8, 512, 5, 5, 1, 2, 1, 1) == \
        b"conv_wide_bwd_data_k<1> lds=120832 b128=4"


def test_workspace_holds_the_planes_and_the_weight(L):
    # 6 blocks of 16 channels x 3 planes x (2*10*10 -> 256 positions - 128 + the 160-row window) x 32 B,
    # then 6 blocks x 9 shifts x 128 channel rows x 32 B
    assert L.bnn_conv2d_bwd_data_wide_workspace(2, 128, 8, 8, 96, 3, 3, 1) == 6 * 3 * 288 * 32 + 6 * 9 * 128 * 32


def test_old_dispatch_is_untouched(L):
    assert L.bnn_conv_kernel(1, 0, 2, 128, 8, 8, 128, 3, 3, 1, 1, 1, 1) == b"conv_bwd_data_k"
    assert L.bnn_conv_kernel(1, 0, 2, 65, 8, 8, 128, 3, 3, 1, 1, 1, 1) == b"conv_bwd_data_k"
    assert L.bnn_conv2d_bwd_data_wide_ok(2, 65, 8, 8, 128, 3, 3, 1, 1, 1, 1) == 0
