"""CPU checks of the wide-channel conv filter gradient's decision function, over the
forward plan test's shapes: the three queries agree, the set lies inside the forward's, the fragment
reads are conflict-free, and the dispatch of bnn_conv2d_bwd_filter is untouched.  Nothing here launches."""
import re

import pytest

from test_conv_wide_plan import SHAPES


@pytest.fixture(scope="module")
def L():
    from bnn_amd import _lib
    return _lib.lib()


def fields(name):
    """{"lds": ..., "splits": ..., "slice": ..., "pieces": ..., ...} of a kernel string."""
    return {k: int(v) for k, v in re.findall(rb"(\w+)=(\d+)", name)} | {b"inst": name.split(b" lds=")[0]}


@pytest.mark.parametrize("shape,ok", SHAPES)
def test_ok_workspace_and_kernel_agree(L, shape, ok):
    N, C, H, W, Co, KH, KW, stride, pad, dil, groups = shape
    assert L.bnn_conv2d_bwd_filter_wide_ok(*shape) == ok      # every listed forward shape fits the filter stage
    assert L.bnn_conv2d_fwd_wide_ok(*shape) >= L.bnn_conv2d_bwd_filter_wide_ok(*shape)
    name = L.bnn_conv2d_bwd_filter_wide_kernel(*shape)
    assert (name != b"") == bool(ok)
    if stride == dil == groups == 1:      # the workspace query takes no such arguments
        assert (L.bnn_conv2d_bwd_filter_wide_workspace(N, C, H, W, Co, KH, KW, pad) > 0) == bool(ok)
    if ok:
        assert name.startswith(b"conv_wide_bwd_filter_k<") and name.endswith(b" b128=4"), name
        assert fields(name)[b"lds"] <= 160 * 1024


@pytest.mark.parametrize("shape", [
    (2, 128, 12, 12, 128, 1, 10, 1, 0, 1, 1),      # KW = 10
    (1, 128, 8, 700, 128, 3, 3, 1, 1, 1, 1),       # the ring's halo alone, 3 x 2 x 88 pieces, is beyond the LDS
])
def test_refused_inside_the_forwards_set(L, shape):
    N, C, H, W, Co, KH, KW, stride, pad, dil, groups = shape
    assert L.bnn_conv2d_fwd_wide_ok(*shape) == 1 and L.bnn_conv2d_bwd_filter_wide_ok(*shape) == 0
    assert L.bnn_conv2d_bwd_filter_wide_kernel(*shape) == b""
    assert L.bnn_conv2d_bwd_filter_wide_workspace(N, C, H, W, Co, KH, KW, pad) == 0


def test_instances_tap_groups_and_k_split(L):
    binarynet = [(256, 128, 32, 32, 128, 3, 3, 1, 1, 1, 1), (256, 512, 8, 8, 512, 3, 3, 1, 1, 1, 1)]
    for shape in binarynet:
        f = fields(L.bnn_conv2d_bwd_filter_wide_kernel(*shape))
        assert f[b"inst"] == b"conv_wide_bwd_filter_k<9, 2>" and f[b"groups"] == 1 and f[b"splits"] > 1
        assert (f[b"splits"] - 1) * f[b"slice"] < f[b"pieces"] <= f[b"splits"] * f[b"slice"]
    # 34816 pieces in chunks of 10 over 2 x 2 tiles: 128 slices wanted, 28 chunks each, which 125 slices cover
    assert fields(L.bnn_conv2d_bwd_filter_wide_kernel(*binarynet[0])) | {b"inst": 0} == {
        b"inst": 0, b"lds": (2 * 3 * 10 + 3 * (2 * 10 + 8)) * 1024, b"groups": 1, b"chunk": 10, b"splits": 125,
        b"slice": 280, b"pieces": 256 * 34 * 4, b"b128": 4}
    f = fields(L.bnn_conv2d_bwd_filter_wide_kernel(256, 512, 8, 8, 512, 5, 5, 1, 2, 1, 1))
    assert f[b"inst"] == b"conv_wide_bwd_filter_k<5, 2>" and f[b"groups"] == 5
    assert fields(L.bnn_conv2d_bwd_filter_wide_kernel(2, 64, 6, 6, 128, 1, 1, 1, 0, 1, 1))[b"inst"] == \
        b"conv_wide_bwd_filter_k<1, 2>"
    # a wide row: the halo leaves room for one stage of two pieces
    assert fields(L.bnn_conv2d_bwd_filter_wide_kernel(1, 128, 8, 190, 128, 3, 3, 1, 1, 1, 1))[b"inst"] == \
        b"conv_wide_bwd_filter_k<9, 1>"


def test_workspace_holds_planes_copies_partials_and_row_sums(L):
    # 2 x 10 rows x 1 piece = 20 pieces in chunks of 12: 2 slices of 12, + 2 halo pieces = 26 per plane / copy;
    # 3 planes x 2 blocks + 3 copies x 2 blocks of them, 2 x 9 x 128 x 128 partials, 2 x 8 x 96 row sums
    assert L.bnn_conv2d_bwd_filter_wide_workspace(2, 128, 8, 8, 96, 3, 3, 1) == \
        12 * 26 * 1024 + 2 * 9 * 128 * 128 * 4 + 2 * 8 * 96 * 4


def test_old_dispatch_is_untouched(L):
    assert L.bnn_conv_kernel(2, 1, 2, 128, 8, 8, 128, 3, 3, 1, 1, 1, 1) == b"conv_bwd_filter_k"
    assert L.bnn_conv_kernel(2, 1, 256, 128, 32, 32, 128, 3, 3, 1, 1, 1, 1) == b"conv_bwd_filter_k"
