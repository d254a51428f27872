"""CPU proof that tests/conv_cases.py covers the conv dispatch: the host-only bnn_conv_kernel query
(the same decision functions the launching entries consume) gives every case's recorded instance
names, and the table reaches every instance bnn_conv_kernel_at lists, both schedules of the bf16x3
data kernel and every wave split of the two MFMA filter kernels.  Also the make_shape guard: a
dilated kernel larger than the padded input is refused by the library and by functional.conv_out_hw.
No GPU: nothing here launches."""
import pytest

import conv_cases as CC

# Instances the table may leave out, with the reason.  Nothing is listed: the only thing a case
# of N <= 17 cannot reach is the ipb=16 schedule of the bf16x3 kernels (N >= 4096), which is a
# run-time schedule of instances the table does reach, and
# test_gpu_parity.py::test_conv_backward_full_batch_vs_float64 runs it.
NEEDS_N_4096 = {}


@pytest.fixture(scope="module")
def L():
    from bnn_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def answers(L):
    """The query's answers for every case, each under its own switches (restored after)."""
    out = []
    popc = L.bnn_conv_set_popc(-1)
    try:
        for c in CC.CASES:
            CC.set_switches(L, c)
            out.append(CC.query(L, c))
    finally:
        CC.restore_switches(L, popc)
    return out


def test_table_is_well_formed():
    assert len(set(c[:15] for c in CC.CASES)) == len(CC.CASES), "duplicate case"
    assert len(set(CC.case_id(c) for c in CC.CASES)) == len(CC.CASES), "duplicate case id"
    for c in CC.CASES:
        assert c.binarize == (c.C != 3), c          # the oracle's input rule
        assert c.N <= 17 and c.H * c.W <= 1100, c
        oh, ow = CC.out_hw(c)
        assert oh > 0 and ow > 0, c


def test_query_gives_the_recorded_instances(answers):
    bad = [(CC.case_id(c), got, (c.fwd, c.data, c.filt))
           for c, got in zip(CC.CASES, answers) if got != (c.fwd, c.data, c.filt)]
    assert not bad, bad


@pytest.mark.parametrize("op", [0, 1, 2])
def test_table_reaches_every_instance(L, answers, op):
    listed = CC.instances(L, op)
    assert len(listed) == len(set(listed)) and len(listed) >= 20
    reached = {CC.base(a[op]) for a in answers}
    assert reached <= set(listed), sorted(reached - set(listed))
    lost = [n for n in listed if n not in reached and n not in NEEDS_N_4096]
    assert not lost, f"no case reaches {lost}"


def test_instance_lists_are_the_documented_families(L):
    fwd, data, filt = (CC.instances(L, op) for op in range(3))
    assert len(fwd) == 20 and len(data) == 26 and len(filt) == 29
    assert CC.instances(L, 3) == [] and L.bnn_conv_kernel_at(0, -1) == b""
    for names, generic in ((fwd, "conv_fwd_k"), (data, "conv_bwd_data_k"), (filt, "conv_bwd_filter_k")):
        assert names[-1] == generic


def test_schedules_are_reached(answers):
    rowt = {CC.schedule(a[1])["rowt"] for a in answers if "_bf3_k<" in a[1]}
    assert rowt == {0, 1}
    wt_b3 = {CC.schedule(a[2])["WT"] for a in answers if "_bf3_k<" in a[2]}
    assert wt_b3 == {1, 2, 4, 8}
    wt_mf = {CC.schedule(a[2])["WT"] for a in answers if "_mfma_k<" in a[2]}
    assert wt_mf == {1, 2, 4}
    for a in answers:                     # WT * KS = the workgroup's waves
        if "_bf3_k<" in a[2]:
            s = CC.schedule(a[2])
            assert s["WT"] * s["KS"] == 8 and s["ipb"] == 8
        if "_mfma_k<" in a[2]:
            s = CC.schedule(a[2])
            assert s["WT"] * s["KS"] == 4


def test_main_block_reaches_every_instance_schedule_pair():
    """Every (instance, schedule) pair the dispatch can produce at the table's sizes, so that deleting
    any case of the main block loses a pair named here.  Filter kernels: a wave split WT holds
    WT .. 2 WT - 1 tiles per tile row below the largest split, so MT = 1 pairs with every WT, MT = 2
    with WT >= 2 and MT >= 4 only with the largest.  bf16x3 data kernel: both schedules wherever a
    plane wider than 16 pixels with that many pixel tiles still fits the LDS (not MT = 16, nor
    MT = 8 with two channel tiles)."""
    want = {}
    for nt in (1, 2):
        for mt in (1, 2, 4, 8, 16):
            want[f"conv_bwd_data_bf3_k<{nt},{mt}>"] = {1} if mt == 16 or (nt, mt) == (2, 8) else {0, 1}
    for na in (1, 2, 3, 4):
        for mt in (1, 2, 4, 8):
            want[f"conv_bwd_filter_bf3_k<{na},{mt}>"] = {1: {1, 2, 4, 8}, 2: {2, 4, 8}}.get(mt, {8})
    for mt in (1, 2, 4, 8, 13, 16):
        want[f"conv_bwd_filter_mfma_k<{mt}>"] = {1: {1, 2, 4}, 2: {2, 4}}.get(mt, {4})
    got = {}
    for c in CC.MAIN:
        if "_bf3_k<" in c.data:
            got.setdefault(CC.base(c.data), set()).add(CC.schedule(c.data)["rowt"])
        if CC.is_mma(c.filt):
            got.setdefault(CC.base(c.filt), set()).add(CC.schedule(c.filt)["WT"])
    assert got == want, {k: (got.get(k), want[k]) for k in want if got.get(k) != want[k]}
    # and no case is there twice over: each reaches a pair or an instance no other main case does
    def keys(c):
        return {(op, " ".join(t for t in c[15 + op].split(" ") if t[:3] not in ("ipb", "KS=")))
                for op in range(3)}
    for c in CC.MAIN:
        others = set().union(*(keys(d) for d in CC.MAIN if d is not c))
        assert not keys(c) <= others, f"redundant case {CC.case_id(c)}"


def test_geometry_block_takes_the_generic_kernels():
    alone = {"stride2": 0, "stride3": 0, "dil2": 0, "groups2": 0, "depthwise": 0, "bigpad": 0, "bigC": 0, "bigCo": 0}
    for c in CC.GEOMETRY:
        props = {"stride2": c.stride == 2, "stride3": c.stride == 3, "dil2": c.dil == 2,
                 "groups2": c.groups == 2, "depthwise": c.groups == c.C == c.Co and c.C > 1,
                 "bigpad": c.pad > min(c.KH, c.KW) - 1, "bigC": c.C > 64, "bigCo": c.Co > 64}
        on = [k for k, v in props.items() if v]
        if len(on) == 1:
            alone[on[0]] += 1
        if c.stride > 1 or c.dil > 1 or c.groups > 1:
            assert (c.fwd, c.data, c.filt) == CC.GEN, c
        else:
            assert c.fwd == "conv_fwd_k", c
    assert all(alone.values()), alone
    assert sum(1 for c in CC.GEOMETRY if (c.stride > 1) + (c.dil > 1) + (c.groups > 1) >= 2) >= 2
    assert any(not c.binarize and c.fwd == "conv_fwd_k" for c in CC.GEOMETRY)   # the generic forward, fp32 input


def test_nonsquare_block_takes_tiled_mfma_and_generic_kernels():
    for k in ((1, 5), (5, 1), (3, 5)):
        cs = [c for c in CC.NONSQUARE if (c.KH, c.KW) == k]
        for op, mma in ((0, ("_i8mfma_k<",)), (1, ("_bf3_k<", "_mfma_k<")), (2, ("_bf3_k<", "_mfma_k<"))):
            names = [c[15 + op] for c in cs]
            assert any("_tile_k<" in n for n in names), (k, op)
            assert any(CC.base(n) == CC.GEN[op] for n in names), (k, op)
            for m in mma:
                assert any(m in n for n in names), (k, op, m)


# ------------------------------------------------------------------------------- the shape guard
BAD = [  # (H, KH, stride, pad, dil): C's truncating division gave these one output row
    (2, 3, 2, 0, 1),
    (5, 3, 3, 0, 3),
]


@pytest.mark.parametrize("h,k,stride,pad,dil", BAD)
@pytest.mark.parametrize("in_w", [False, True])
def test_library_refuses_a_kernel_larger_than_the_padded_input(L, h, k, stride, pad, dil, in_w):
    H, W, KH, KW = (9, h, 1, k) if in_w else (h, 9, k, 1)
    for op in range(3):
        assert L.bnn_conv_kernel(op, 1, 1, 1, H, W, 1, KH, KW, stride, pad, dil, 1) == b""
    assert L.bnn_conv2d_fwd_q_ok(2, 1, 1, H, W, 1, KH, KW, stride, pad, dil, 1) == 0
    # the same plane with enough padding is accepted
    assert L.bnn_conv_kernel(0, 1, 1, 1, H, W, 1, KH, KW, stride, pad + dil, dil, 1) != b""


def test_issue_shape_is_refused(L):
    assert L.bnn_conv_kernel(0, 1, 1, 1, 2, 2, 1, 3, 3, 2, 0, 1, 1) == b""
    from bnn_amd import functional as F
    with pytest.raises(ValueError):
        F.conv_out_hw(2, 2, 3, 3, 2, 0, 1)


@pytest.mark.parametrize("h,k,stride,pad,dil", BAD)
def test_out_size_helper_raises(h, k, stride, pad, dil):
    from bnn_amd import functional as F
    with pytest.raises(ValueError):
        F.conv_out_hw(h, 9, k, 1, stride, pad, dil)
    with pytest.raises(ValueError):
        F.conv_out_hw(9, h, 1, k, stride, pad, dil)


def test_out_size_helper_matches_the_case_table():
    from bnn_amd import functional as F
    for c in CC.CASES:
        assert F.conv_out_hw(c.H, c.W, c.KH, c.KW, c.stride, c.pad, c.dil) == CC.out_hw(c)
    assert F.conv_out_hw(2, 2, 3, 3, 2, 1, 1) == (1, 1)
    assert F.conv_out_hw(5, 7, 3, 3, 3, 1, 3) == (1, 1)     # extent 7 == padded height 7


def test_query_answers_for_empty_and_bad_arguments(L):
    assert L.bnn_conv_kernel(0, 1, 0, 1, 8, 8, 4, 3, 3, 1, 1, 1, 1) == b"none"
    assert L.bnn_conv_kernel(1, 1, 0, 1, 8, 8, 4, 3, 3, 1, 1, 1, 1) == b"none"
    assert L.bnn_conv_kernel(2, 1, 0, 1, 8, 8, 4, 3, 3, 1, 1, 1, 1) == b"none"
    assert L.bnn_conv_kernel(3, 1, 1, 1, 8, 8, 4, 3, 3, 1, 1, 1, 1) == b""
    assert L.bnn_conv_kernel(-1, 1, 1, 1, 8, 8, 4, 3, 3, 1, 1, 1, 1) == b""
    assert L.bnn_conv_kernel(0, 1, 1, 4, 8, 8, 4, 3, 3, 1, 1, 1, 3) == b""      # C % groups != 0


def test_switches_change_the_answer_and_are_restored(L):
    """The BinCNN's layers under the three switches: what the default launches, and what the
    cross-check modes launch instead."""
    conv2 = (4096, 16, 14, 14, 32, 5, 5, 1, 2, 1, 1)
    conv1 = (4096, 1, 28, 28, 16, 5, 5, 1, 2, 1, 1)
    popc = L.bnn_conv_set_popc(-1)
    try:
        L.bnn_conv_set_popc(0)
        assert L.bnn_conv_kernel(0, 1, *conv2) == b"conv_fwd_i8mfma_k<2>"
        assert L.bnn_conv_kernel(1, 1, *conv2) == b"conv_bwd_data_bf3_k<1,2> rowt=1 ipb=16"
        assert L.bnn_conv_kernel(2, 1, *conv2) == b"conv_bwd_filter_bf3_k<2,4> WT=8 KS=1 ipb=16"
        assert L.bnn_conv_kernel(0, 1, *conv1) == b"conv_fwd_bin_c1_k<16,2>"
        assert L.bnn_conv_kernel(2, 1, *conv1) == b"conv_bwd_filter_c1_k<5,5>"
        L.bnn_conv_set_c1_filter(0)
        assert L.bnn_conv_kernel(2, 1, *conv1).startswith(b"conv_bwd_filter_bf3_k<1,")
        L.bnn_conv_set_mfma(2)
        assert L.bnn_conv_kernel(1, 1, *conv2) == b"conv_bwd_data_mfma_k<1,4>"      # 13 pixel tiles on 4 waves
        assert L.bnn_conv_kernel(2, 1, *conv2) == b"conv_bwd_filter_mfma_k<13> WT=4 KS=1"
        L.bnn_conv_set_mfma(0)
        assert L.bnn_conv_kernel(0, 1, *conv2) == b"conv_fwd_bin_tile_k<32>"
        assert L.bnn_conv_kernel(1, 1, *conv2) == b"conv_bwd_data_tile_k<16>"
        assert L.bnn_conv_kernel(2, 1, *conv2) == b"conv_bwd_filter_tile_k<32>"
        L.bnn_conv_set_popc(1)
        assert L.bnn_conv_kernel(0, 1, *conv2) == b"popc"
    finally:
        CC.restore_switches(L, popc)
    assert L.bnn_conv_set_popc(-1) == popc
