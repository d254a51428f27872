"""CPU checks of the wide-conv training hand-off's decision functions: which shapes
bnn_bn2d_fwd_train_planes_ok takes, and that the workspace queries of the two consumer entries are positive
exactly where their shape queries accept.  No GPU: nothing here launches."""
import pytest

# (N, C, H, W, pool | consumer KH = KW, pad, Co): the smallest shapes at which each mechanism can go wrong
CASES = [
    (2, 64, 4, 6, 2, 3, 1, 65),      # one channel block, pooled, Co tail
    (3, 128, 5, 8, 0, 3, 1, 64),     # two blocks, odd H, no pool
    (1, 64, 2, 132, 2, 3, 1, 128),   # 66 output columns: a second 64-column pass
    (2, 128, 4, 4, 0, 1, 0, 128),    # no halo
    (2, 64, 6, 6, 2, 5, 4, 128),     # pad = K - 1, a single-LDS-stage consumer
    (0, 64, 4, 4, 2, 3, 1, 128),     # the empty batch
]
REFUSED = [
    (2, 96, 4, 6, 2, 3, 1, 128),     # C % 64
    (2, 64, 5, 6, 2, 3, 1, 128),     # odd H with pool 2
    (2, 64, 3, 6, 0, 3, 1, 128),     # H W % 4
    (2, 64, 4, 6, 1, 3, 1, 128),     # pool 1
    (2, 64, 4, 6, 2, 3, 3, 128),     # a consumer with pad = K: planes_bytes == 0
]


@pytest.fixture(scope="module")
def L():
    from bnn_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("case,ok", [(c, 1) for c in CASES] + [(c, 0) for c in REFUSED])
def test_ok_and_workspaces(L, case, ok):
    N, C, H, W, pool, K, pad, Co = case
    assert L.bnn_bn2d_fwd_train_planes_ok(N, C, H, W, pool, K, K, pad) == ok
    PH, PW = (H // 2, W // 2) if pool else (H, W)
    assert (L.bnn_conv2d_wide_planes_bytes(N, C, PH, PW, K, K, pad) > 0) >= bool(ok)
    shape = (N, C, PH, PW, Co, K, K)
    for query, accepts in ((L.bnn_conv2d_fwd_wide_planes_workspace, L.bnn_conv2d_fwd_wide_ok),
                           (L.bnn_conv2d_bwd_filter_wide_workspace, L.bnn_conv2d_bwd_filter_wide_ok)):
        assert (query(*shape, pad) > 0) == bool(accepts(*shape, 1, pad, 1, 1))
        assert ok == 0 or accepts(*shape, 1, pad, 1, 1) == 1     # every case of the table runs all three entries
    if ok:
        assert L.bnn_conv2d_fwd_wide_planes_workspace(*shape, pad) == L.bnn_conv2d_wide_wq_bytes(C, Co, K, K)
