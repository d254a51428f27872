"""CPU checks of the frozen first-layer conv's decision function: which geometries
bnn_conv2d_fwd_first_bnsign_ok takes, that the kernel-name query agrees with it, and that the GPU test's case
table reaches every kernel instance the entry can launch.  No GPU: nothing here launches."""
import re

import pytest

import conv_first_infer_cases as CF

# (N, C, H, W, Co, KH, KW, stride, pad, dil, groups, pool, out_form, KH2, KW2, pad2), taken?
SHAPES = [
    ((256, 3, 32, 32, 128, 3, 3, 1, 1, 1, 1, 0, 0, 3, 3, 1), 1),
    ((0, 3, 32, 32, 128, 3, 3, 1, 1, 1, 1, 2, 1, 0, 0, 0), 1),     # an empty batch is a shape like any other
    ((2, 3, 8, 8, 64, 3, 3, 1, 1, 1, 1, 0, 1, 0, 0, 0), 0),        # Co <= 64
    ((2, 5, 8, 8, 128, 3, 3, 1, 1, 1, 1, 0, 1, 0, 0, 0), 0),       # C = 5
    ((2, 3, 8, 8, 128, 3, 3, 2, 1, 1, 1, 0, 1, 0, 0, 0), 0),       # stride 2
    ((2, 3, 9, 8, 128, 3, 3, 1, 1, 1, 1, 2, 1, 0, 0, 0), 0),       # odd OH with pool 2
    ((2, 3, 8, 8, 130, 3, 3, 1, 1, 1, 1, 2, 0, 3, 3, 1), 0),       # planes of 130 channels
    ((2, 3, 8, 8, 130, 3, 3, 1, 1, 1, 1, 2, 1, 3, 3, 1), 1),       # ... int8 signs of 130 channels
    ((2, 3, 8, 8, 128, 3, 3, 1, 1, 1, 1, 2, 0, 3, 3, 3), 0),       # a consumer with pad2 = K2
    ((1, 3, 8, 1800, 128, 3, 3, 1, 1, 1, 1, 0, 1, 0, 0, 0), 1),    # a window pool 0 holds
    ((1, 3, 8, 1800, 128, 3, 3, 1, 1, 1, 1, 2, 1, 0, 0, 0), 0),    # ... and the pooled mapping's does not fit
]
INSTANCES = {f"conv_first_bnsign_k<{ks},{pool}>" for ks in (1, 2, 3, 4, 5) for pool in (0, 2)}


@pytest.fixture(scope="module")
def L():
    from bnn_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("shape,ok", SHAPES)
def test_ok_and_kernel_agree(L, shape, ok):
    assert L.bnn_conv2d_fwd_first_bnsign_ok(*shape) == ok
    name = L.bnn_conv2d_fwd_first_bnsign_kernel(*shape).decode()
    assert (name != "") == bool(ok)
    if ok:
        assert re.fullmatch(r"conv_first_bnsign_k<[1-5],%d> form=%d lds=\d+ rows=\d+ Kp=\d+ pitch=\d+ b128=\d+"
                            % (shape[11], shape[12]), name)


def test_case_table_reaches_every_instance(L):
    names = [L.bnn_conv2d_fwd_first_bnsign_kernel(*CF.abi_shape(c)).decode() for c in CF.CASES]
    assert all(names)
    assert {n.split(" ")[0] for n in names} == INSTANCES
    assert {n.split(" ")[1] for n in names} == {"form=0", "form=1"}
