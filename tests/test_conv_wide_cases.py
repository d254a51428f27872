"""CPU proof that tests/conv_wide_cases.py reaches what it says: the four host-only kernel queries (the
decision functions the launching entries consume) give every case's recorded instance, the table's
union covers every instance of the four kernels but the filter gradient's documented unreachable one,
and each feature a case was added for is present, computed here from the shapes.  A change to a plan
function that moves a case off its instance fails here, and so does the table with any one new case
taken out.  No GPU: nothing here launches."""
import pytest

import conv_wide_cases as CW


@pytest.fixture(scope="module")
def L():
    from bnn_amd import _lib
    return _lib.lib()


def test_table_is_well_formed():
    shapes = [t.shape for t in CW.TRAIN]
    cases = [c.case for c in CW.INFER]
    assert shapes == CW.SHAPES + CW.NEW_SHAPES and len(CW.SHAPES) == 7
    assert cases == CW.INFER_CASES + CW.NEW_INFER_CASES and len(CW.INFER_CASES) == 7
    assert len(set(shapes)) == len(shapes) and len(set(cases)) == len(cases)
    assert len({CW.shape_id(s) for s in shapes + cases}) == len(shapes) + len(cases)
    assert CW.NO_BIAS is CW.SHAPES[3] and CW.NO_DB is CW.SHAPES[3] and CW.NO_DB_NEW in CW.NEW_SHAPES
    for s in shapes + cases:                        # test size: far below the workload's
        assert s[0] * s[1] * s[2] * s[3] <= 5 * 64 * 34 * 34 and s[4] <= 192, s
    for s in CW.NEW_SHAPES + CW.NEW_INFER_CASES:    # and no new case is larger than 64 x 3 x 640
        assert s[0] * s[1] * s[2] * s[3] <= 64 * 3 * 640, s
    assert all(t.fwd for t in CW.TRAIN) and all(c.inst for c in CW.INFER)
    assert CW.NULL_CASES[0][8] == 2 and CW.NULL_CASES[0][9] is not None and CW.NULL_CASES[1][9] is None
    assert all(c in CW.NEW_INFER_CASES for c in CW.NULL_CASES)


@pytest.mark.parametrize("t", CW.TRAIN, ids=lambda t: CW.shape_id(t.shape))
def test_training_queries_give_the_recorded_instances(L, t):
    names = CW.query_train(L, t.shape)
    assert tuple(CW.instance(n) for n in names) == (t.fwd, t.data, t.filt)
    a = CW.train_args(t.shape)
    for name, ok, ws in ((t.fwd, L.bnn_conv2d_fwd_wide_ok(*a), L.bnn_conv2d_fwd_wide_workspace(*t.shape)),
                         (t.data, L.bnn_conv2d_bwd_data_wide_ok(*a), L.bnn_conv2d_bwd_data_wide_workspace(*t.shape)),
                         (t.filt, L.bnn_conv2d_bwd_filter_wide_ok(*a), L.bnn_conv2d_bwd_filter_wide_workspace(*t.shape))):
        assert ok == int(bool(name)) and (ws > 0) == bool(name)      # a refused op is refused by all three queries
    for n in names:
        if n:
            f = CW.fields(n)
            assert f["lds"] <= 160 * 1024 and f["b128"] == 4, n       # conflict-free fragment reads


@pytest.mark.parametrize("c", CW.INFER, ids=lambda c: CW.shape_id(c.case))
def test_infer_query_gives_the_recorded_instance(L, c):
    n = CW.query_infer(L, c.case)
    assert CW.instance(n) == c.inst
    assert L.bnn_conv2d_fwd_wide_bnsign_ok(*CW.infer_args(c.case)) == 1
    assert CW.fields(n)["lds"] <= 160 * 1024


def gaps(L, train, infer):
    """What a table of these cases would leave unrun: instances, then the named features, each computed
    from the shapes (and the filter query's fields).  Empty for the table as it stands."""
    out = []

    def need(what, ok):
        if not ok:
            out.append(what)
    shapes = [t.shape for t in train]
    filt = [t.shape for t in train if t.filt]
    data = [t.shape for t in train if t.data]
    cases = [c.case for c in infer]
    wp = lambda s: s[3] + 2 * s[7]
    ow = lambda s: wp(s) - s[6] + 1
    ff = {s: CW.fields(L.bnn_conv2d_bwd_filter_wide_kernel(*CW.train_args(s))) for s in filt}
    # 1. instances
    need("gemm", {t.fwd for t in train} == {"conv_wide_gemm_k<1>", "conv_wide_gemm_k<2>"})
    need("bwd_data", {t.data for t in train} - {""} == {"conv_wide_bwd_data_k<1>", "conv_wide_bwd_data_k<2>"})
    need("bnsign", {c.inst for c in infer} == {f"conv_wide_bnsign_k<{nb},{pool},{form}>"
                                               for nb in (1, 2) for pool in (0, 2) for form in (0, 1)})
    need("bwd_filter", {t.filt for t in train} - {""} == CW.FILTER_INSTANCES - CW.FILTER_UNREACHABLE)
    # 2. a single-stage 3x3 in the forward and in the data gradient (the 5x5 was the only single-stage shape),
    #    and a forward the two gradients refuse
    need("gemm<1> 3x3", any(t.fwd.endswith("<1>") and t.shape[5:7] == (3, 3) for t in train))
    need("bwd_data<1> 3x3", any(t.data.endswith("<1>") and t.shape[5:7] == (3, 3) for t in train))
    need("forward only", any(not t.data and not t.filt for t in train))
    # 3. a row of more than two 64-column passes through every pack kernel: the forward's pack_x (W) and the
    #    infer pack_x, the data gradient's pack_dy (OW), the filter's pack_dy (OW) and pack_x (OWq)
    need("Wp > 128", any(wp(s) > 128 for s in shapes))
    need("passes fwd", any(s[3] > 128 for s in shapes))
    need("passes infer", any(c[3] > 128 for c in cases))
    need("passes data", any(ow(s) > 128 for s in data))
    need("passes filt", any(ow(s) > 128 for s in filt))
    need("passes filt without db", ow(CW.NO_DB_NEW) > 128 and CW.NO_DB_NEW in filt)
    # 4. the pooled mapping with Wpe != Wp (only even kernel widths reach it): to planes without and with
    #    padding of its own, and to int8
    odd = [c for c in cases if c[8] == 2 and wp(c) % 2 == 1]
    need("odd Wp planes pad 0", any(c[9] is not None and c[7] == 0 for c in odd))
    need("odd Wp planes pad > 0", any(c[9] is not None and c[7] > 0 for c in odd))
    need("odd Wp int8", any(c[9] is None for c in odd))
    # 5. a last tap group with fewer kh rows than grows: with a halo of its own (2 of 3) and without (1 of 3)
    short = {(s[5] % CW.tap_groups(s)[0], CW.tap_groups(s)[0]) for s in filt}
    need("last group 2 of 3", (2, 3) in short and all(ff[s]["groups"] == 2 for s in filt if s[5:7] == (5, 3)))
    need("last group 1 of 3", (1, 3) in short and all(ff[s]["groups"] == 2 for s in filt if s[5:7] == (4, 3)))
    # 6. the partial-group path: fewer taps than the instance's accumulator sets in the only group
    cnt = {CW.tap_groups(s)[2] for s in filt}
    need("grows KW not in {1, 3, 5, 9}", bool(cnt - {1, 3, 5, 9}))
    need("4 taps of 5", 4 in cnt)
    need("8 taps of 9", 8 in cnt)
    need("filter LDS of 160 KiB with KW = 4", any(s[6] == 4 and ff[s]["lds"] == 160 * 1024 for s in filt))
    # 7. four channel blocks: the stage parity goes past block 2
    need("C // 64 >= 4", any(s[1] // 64 >= 4 for s in shapes))
    need("C // 64 >= 4 infer", any(c[1] // 64 >= 4 for c in cases))
    # 8. several K slices with a short last one
    need("short last K slice", any(f["splits"] > 1 and (f["splits"] - 1) * f["slice"] < f["pieces"] < f["splits"] * f["slice"]
                                   for f in ff.values()))
    return out


def test_table_covers_every_instance_and_named_feature(L):
    assert CW.FILTER_UNREACHABLE == {"conv_wide_bwd_filter_k<1, 1>"}
    assert gaps(L, CW.TRAIN, CW.INFER) == []


def test_no_new_case_can_be_deleted(L):
    for t in CW.TRAIN[7:]:
        assert gaps(L, [u for u in CW.TRAIN if u is not t], CW.INFER), f"nothing is lost without {t.shape}"
    for c in CW.INFER[7:]:
        assert gaps(L, CW.TRAIN, [u for u in CW.INFER if u is not c]), f"nothing is lost without {c.case}"


def test_the_forward_only_case_is_refused_by_both_gradients(L):
    fwd_only = [t for t in CW.TRAIN if not t.data or not t.filt]
    assert [t.shape for t in fwd_only] == [(1, 64, 3, 640, 65, 3, 3, 1)]
    a = CW.train_args(fwd_only[0].shape)
    assert L.bnn_conv2d_fwd_wide_ok(*a) == 1
    assert L.bnn_conv2d_bwd_data_wide_ok(*a) == 0 and L.bnn_conv2d_bwd_filter_wide_ok(*a) == 0


def test_a_one_tap_filter_never_runs_single_stage(L):
    """What the table's docstring says of <1, 1>: a 1 x 1 kernel has no halo, so the widest and the
    tallest planes the forward still takes run two stages."""
    for shape in ((1, 64, 1, 4000, 65, 1, 1, 0), (1, 64, 3, 1200, 65, 1, 1, 0), (1, 128, 1 << 20, 1, 128, 1, 1, 0)):
        assert L.bnn_conv2d_fwd_wide_ok(*CW.train_args(shape)) == 1
        assert CW.instance(L.bnn_conv2d_bwd_filter_wide_kernel(*CW.train_args(shape))) == "conv_wide_bwd_filter_k<1, 2>"


def test_empty_batch_is_a_shape_like_any_other(L):
    a = CW.train_args(CW.EMPTY)
    assert CW.EMPTY[0] == 0
    assert L.bnn_conv2d_fwd_wide_ok(*a) == L.bnn_conv2d_bwd_data_wide_ok(*a) == L.bnn_conv2d_bwd_filter_wide_ok(*a) == 1
    assert L.bnn_conv2d_fwd_wide_bnsign_ok(*a, 2, 0, 3, 3, 1) == L.bnn_conv2d_fwd_wide_bnsign_ok(*a, 2, 1, 0, 0, 0) == 1
    assert min(L.bnn_conv2d_fwd_wide_workspace(*CW.EMPTY), L.bnn_conv2d_bwd_data_wide_workspace(*CW.EMPTY),
               L.bnn_conv2d_bwd_filter_wide_workspace(*CW.EMPTY)) > 0
