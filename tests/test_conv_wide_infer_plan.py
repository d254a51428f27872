"""CPU checks of the frozen wide-channel conv's decision function: which geometries
bnn_conv2d_fwd_wide_bnsign_ok takes, that the kernel-name query agrees with it, that the two operand sizes
are the two parts of bnn_conv2d_fwd_wide's workspace, and that the existing queries answer as before.
No GPU: nothing here launches."""
import pytest

# (N, C, H, W, Co, KH, KW, stride, pad, dil, groups, pool, out_form, KH2, KW2, pad2), taken?
SHAPES = [
    ((256, 128, 32, 32, 128, 3, 3, 1, 1, 1, 1, 2, 0, 3, 3, 1), 1),
    ((256, 512, 8, 8, 512, 3, 3, 1, 1, 1, 1, 0, 0, 3, 3, 1), 1),
    ((1, 64, 6, 6, 65, 3, 3, 1, 1, 1, 1, 0, 1, 0, 0, 0), 1),
    ((2, 64, 8, 8, 64, 1, 1, 1, 0, 1, 1, 2, 0, 1, 1, 0), 1),       # 64 -> 64 is taken here
    ((2, 64, 6, 10, 192, 3, 3, 1, 2, 1, 1, 2, 0, 5, 5, 2), 1),
    ((0, 128, 8, 8, 128, 3, 3, 1, 1, 1, 1, 2, 1, 0, 0, 0), 1),     # an empty batch is a shape like any other
    ((2, 128, 8, 8, 128, 3, 3, 1, 1, 1, 1, 1, 1, 0, 0, 0), 0),     # pool 1
    ((2, 128, 8, 8, 128, 3, 3, 1, 1, 1, 1, 3, 1, 0, 0, 0), 0),     # pool 3
    ((2, 128, 9, 8, 128, 3, 3, 1, 1, 1, 1, 2, 1, 0, 0, 0), 0),     # odd OH with pool 2
    ((2, 128, 9, 8, 128, 3, 3, 1, 1, 1, 1, 0, 1, 0, 0, 0), 1),     # ... which pool 0 takes
    ((2, 128, 8, 8, 96, 3, 3, 1, 1, 1, 1, 2, 0, 3, 3, 1), 0),      # planes of 96 channels
    ((2, 128, 8, 8, 96, 3, 3, 1, 1, 1, 1, 2, 1, 3, 3, 1), 1),      # ... int8 signs of 96 channels
    ((2, 128, 8, 8, 128, 3, 3, 1, 1, 1, 1, 2, 0, 3, 3, 3), 0),     # a consumer with pad2 = K2
    ((2, 128, 8, 8, 128, 3, 3, 2, 1, 1, 1, 0, 1, 0, 0, 0), 0),     # stride 2
    ((2, 80, 8, 8, 128, 3, 3, 1, 1, 1, 1, 0, 1, 0, 0, 0), 0),      # C % 64
    ((1, 128, 8, 2000, 128, 3, 3, 1, 1, 1, 1, 0, 1, 0, 0, 0), 0),  # the window beyond the LDS
    ((1, 128, 8, 1500, 128, 3, 3, 1, 1, 1, 1, 0, 1, 0, 0, 0), 1),  # a window pool 0 still holds
    ((1, 128, 8, 1500, 128, 3, 3, 1, 1, 1, 1, 2, 1, 0, 0, 0), 0),  # ... and the pooled mapping's does not fit
]


@pytest.fixture(scope="module")
def L():
    from bnn_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("shape,ok", SHAPES)
def test_ok_and_kernel_agree(L, shape, ok):
    assert L.bnn_conv2d_fwd_wide_bnsign_ok(*shape) == ok
    name = L.bnn_conv2d_fwd_wide_bnsign_kernel(*shape)
    assert (name != b"") == bool(ok)
    if ok:
        pool, form = shape[11], shape[12]
        assert name.startswith(b"conv_wide_bnsign_k<") and b",%d,%d> lds=" % (pool, form) in name and b" b128=" in name


def test_operand_sizes_are_the_parts_of_the_training_workspace(L):
    # 2 blocks x (2*10*10 -> 256 positions - 128 + the 160-row window) x 32 B, then 2 x 9 x 128 rows x 32 B
    assert L.bnn_conv2d_wide_planes_bytes(2, 128, 8, 8, 3, 3, 1) == 2 * 288 * 32
    assert L.bnn_conv2d_wide_wq_bytes(128, 96, 3, 3) == 2 * 9 * 128 * 32
    assert (L.bnn_conv2d_fwd_wide_workspace(2, 128, 8, 8, 96, 3, 3, 1)
            == L.bnn_conv2d_wide_planes_bytes(2, 128, 8, 8, 3, 3, 1) + L.bnn_conv2d_wide_wq_bytes(128, 96, 3, 3))
    assert L.bnn_conv2d_wide_planes_bytes(2, 80, 8, 8, 3, 3, 1) == 0 == L.bnn_conv2d_wide_wq_bytes(80, 96, 3, 3)


def test_existing_queries_answer_as_before(L):
    assert L.bnn_conv2d_fwd_wide_kernel(256, 128, 32, 32, 128, 3, 3, 1, 1, 1, 1) == b"conv_wide_gemm_k<2> lds=88064 b128=4"
    assert L.bnn_conv2d_fwd_wide_ok(2, 64, 8, 8, 64, 3, 3, 1, 1, 1, 1) == 0
    assert L.bnn_conv_kernel(0, 1, 2, 128, 8, 8, 128, 3, 3, 1, 1, 1, 1) == b"conv_fwd_k"
