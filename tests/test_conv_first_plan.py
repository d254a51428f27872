"""CPU checks of the first-layer conv's decision function.  Nothing here launches."""
import re

import pytest

FLAGSHIP = (256, 3, 32, 32, 128, 3, 3, 1, 1, 1, 1)       # N, C, H, W, Co, KH, KW, stride, pad, dil, groups
SHAPES = [
    (FLAGSHIP, 1),
    ((2, 3, 9, 11, 129, 5, 5, 1, 2, 1, 1), 1),            # Kt = 75
    ((1, 1, 8, 8, 65, 3, 3, 1, 1, 1, 1), 1),
    ((1, 4, 8, 9, 65, 2, 4, 1, 1, 1, 1), 1),              # Kt = 32
    ((0, 3, 8, 8, 65, 3, 3, 1, 1, 1, 1), 1),              # the empty batch
    ((1, 3, 8, 1972, 65, 3, 3, 1, 1, 1, 1), 1),           # the widest 3x3 RGB row whose window fits the LDS
    ((1, 3, 8, 1973, 65, 3, 3, 1, 1, 1, 1), 0),
    ((2, 5, 8, 8, 128, 3, 3, 1, 1, 1, 1), 0),             # C = 5
    ((2, 3, 8, 8, 64, 3, 3, 1, 1, 1, 1), 0),              # Co = 64: the tiled kernels' shape
    ((2, 3, 8, 8, 128, 3, 3, 2, 1, 1, 1), 0),             # stride 2
    ((2, 3, 8, 8, 128, 3, 3, 1, 3, 1, 1), 0),             # pad = K
    ((2, 1, 12, 12, 128, 9, 9, 1, 0, 1, 1), 0),           # Kt = 81
    ((2, 4, 8, 8, 128, 3, 3, 1, 1, 1, 2), 0),             # groups 2
]


@pytest.fixture(scope="module")
def L():
    from bnn_amd import _lib
    return _lib.lib()


def fields(name):
    return {k: int(v) for k, v in re.findall(rb"(\w+)=(\d+)", name)} | {b"inst": name.split(b" lds=")[0]}


@pytest.mark.parametrize("shape,ok", SHAPES)
def test_ok_workspace_and_kernels_agree(L, shape, ok):
    N, C, H, W, Co, KH, KW, stride, pad, dil, groups = shape
    assert L.bnn_conv2d_fwd_first_ok(*shape) == ok and L.bnn_conv2d_bwd_filter_first_ok(*shape) == ok
    fwd, flt = L.bnn_conv2d_fwd_first_kernel(*shape), L.bnn_conv2d_bwd_filter_first_kernel(*shape)
    assert (fwd != b"") == bool(ok) and (flt != b"") == bool(ok)
    if stride == dil == groups == 1:      # the workspace query takes no such arguments
        assert (L.bnn_conv2d_bwd_filter_first_workspace(N, C, H, W, Co, KH, KW, pad) > 0) == bool(ok and N > 0)
    if ok:
        assert fwd.startswith(b"conv_first_fwd_k<") and flt.startswith(b"conv_first_bwd_filter_k<")
        assert max(fields(fwd)[b"lds"], fields(flt)[b"lds"]) <= 160 * 1024
        assert fields(fwd)[b"b128"] == 4                  # the weight fragment read is conflict-free


def test_workspace_is_the_partial_layout(L):
    # 256 x 32 rows over one channel tile: 512 slices of 16 rows, [512][128][round_up(27 + 1, 32)] floats
    assert L.bnn_conv2d_bwd_filter_first_workspace(256, 3, 32, 32, 128, 3, 3, 1) == 512 * 128 * 32 * 4
    f = fields(L.bnn_conv2d_bwd_filter_first_kernel(*FLAGSHIP))
    assert (f[b"rows"], f[b"slice"], f[b"splits"], f[b"Kp"]) == (8192, 16, 512, 32)
    # 3 x 9 = 27 rows, fewer than two rounds of workgroups: a slice per row; Co = 129 -> 256 rows, Kt + 1 = 76 -> 96
    assert L.bnn_conv2d_bwd_filter_first_workspace(3, 3, 9, 11, 129, 5, 5, 2) == 27 * 256 * 96 * 4
    # Kt = 32: the ones column of db needs a second block
    assert L.bnn_conv2d_bwd_filter_first_workspace(1, 4, 8, 9, 65, 2, 4, 1) == 9 * 128 * 64 * 4


def test_kernel_strings_tell_the_instances_apart(L):
    def insts(C, W, K, pad):
        s = (2, C, 8, W, 128, K, K, 1, pad, 1, 1)
        return fields(L.bnn_conv2d_fwd_first_kernel(*s))[b"inst"], fields(L.bnn_conv2d_bwd_filter_first_kernel(*s))[b"inst"]
    assert insts(3, 8, 3, 1) == (b"conv_first_fwd_k<2>", b"conv_first_bwd_filter_k<1, 1>")
    assert insts(3, 9, 3, 1) == (b"conv_first_fwd_k<2>", b"conv_first_bwd_filter_k<1, 0>")     # OW % 4 != 0
    assert insts(1, 8, 3, 1) == (b"conv_first_fwd_k<1>", b"conv_first_bwd_filter_k<1, 1>")
    assert insts(3, 8, 5, 2) == (b"conv_first_fwd_k<5>", b"conv_first_bwd_filter_k<3, 1>")
    assert insts(4, 8, 3, 1) == (b"conv_first_fwd_k<3>", b"conv_first_bwd_filter_k<2, 1>")
    assert insts(4, 8, 4, 1)[0] == b"conv_first_fwd_k<4>"
    assert b"chunk=1x64 " in L.bnn_conv2d_bwd_filter_first_kernel(1, 3, 8, 300, 128, 3, 3, 1, 1, 1, 1)   # a long row
    assert b"chunk=2x32 " in L.bnn_conv2d_bwd_filter_first_kernel(*FLAGSHIP)
