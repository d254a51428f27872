"""CPU checks of the wide-channel conv forward's decision function: which shapes
bnn_conv2d_fwd_wide_ok takes, that the workspace and kernel-name queries agree with it, and that the
dispatch of bnn_conv2d_fwd is untouched.  No GPU: nothing here launches."""
import pytest

# (N, C, H, W, Co, KH, KW, stride, pad, dil, groups), taken?
SHAPES = [
    ((1, 64, 5, 7, 65, 3, 3, 1, 1, 1, 1), 1),
    ((256, 128, 32, 32, 128, 3, 3, 1, 1, 1, 1), 1),
    ((2, 64, 6, 6, 128, 1, 1, 1, 0, 1, 1), 1),
    ((256, 512, 8, 8, 512, 5, 5, 1, 2, 1, 1), 1),
    ((2, 192, 8, 8, 16, 1, 3, 1, 0, 1, 1), 1),
    ((0, 128, 8, 8, 128, 3, 3, 1, 1, 1, 1), 1),         # an empty batch is a shape like any other
    ((2, 80, 8, 8, 128, 3, 3, 1, 1, 1, 1), 0),          # C % 64
    ((2, 64, 8, 8, 64, 3, 3, 1, 1, 1, 1), 0),           # the fast paths of bnn_conv2d_fwd take it
    ((2, 128, 8, 8, 128, 3, 3, 2, 1, 1, 1), 0),         # stride
    ((2, 128, 8, 8, 128, 3, 3, 1, 1, 2, 1), 0),         # dilation
    ((2, 128, 8, 8, 128, 3, 3, 1, 1, 1, 2), 0),         # groups
    ((2, 128, 8, 8, 128, 3, 3, 1, 3, 1, 1), 0),         # pad = K
    ((2, 128, 3, 3, 128, 3, 3, 1, 0, 2, 1), 0),         # dilated kernel larger than the padded input
    ((2, 128, 2, 8, 128, 3, 3, 1, 0, 1, 1), 0),         # kernel larger than the input
    ((1, 128, 8, 2000, 128, 3, 3, 1, 1, 1, 1), 0),      # the shifted window of one block is beyond the LDS
]


@pytest.fixture(scope="module")
def L():
    from bnn_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("shape,ok", SHAPES)
def test_ok_workspace_and_kernel_agree(L, shape, ok):
    N, C, H, W, Co, KH, KW, stride, pad, dil, groups = shape
    assert L.bnn_conv2d_fwd_wide_ok(*shape) == ok
    name = L.bnn_conv2d_fwd_wide_kernel(*shape)
    assert (name != b"") == bool(ok)
    if stride == dil == groups == 1:      # the workspace query takes no such arguments
        assert (L.bnn_conv2d_fwd_wide_workspace(N, C, H, W, Co, KH, KW, pad) > 0) == bool(ok)
    if ok:
        assert name.startswith(b"conv_wide_gemm_k<") and name.endswith(b" b128=4"), name   # conflict-free reads


def test_double_buffer_where_it_fits(L):
    assert L.bnn_conv2d_fwd_wide_kernel(256, 128, 32, 32, 128, 3, 3, 1, 1, 1, 1).startswith(b"conv_wide_gemm_k<2> ")
    assert L.bnn_conv2d_fwd_wide_kernel(256, 512, 8, 8, 512, 5, 5, 1, 2, 1, 1).startswith(b"conv_wide_gemm_k<1> ")


def test_workspace_holds_both_packed_operands(L):
    # 2 blocks x (2*10*10 -> 256 positions - 128 + the 160-row window) x 32 B, then 2 x 9 x 128 rows x 32 B
    assert L.bnn_conv2d_fwd_wide_workspace(2, 128, 8, 8, 96, 3, 3, 1) == 2 * 288 * 32 + 2 * 9 * 128 * 32


def test_old_dispatch_is_untouched(L):
    assert L.bnn_conv_kernel(0, 1, 2, 128, 8, 8, 128, 3, 3, 1, 1, 1, 1) == b"conv_fwd_k"
    assert L.bnn_conv_kernel(0, 1, 2, 64, 8, 8, 65, 3, 3, 1, 1, 1, 1) == b"conv_fwd_k"
