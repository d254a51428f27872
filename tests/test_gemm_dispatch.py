"""CPU proof that the int8 / FP4 GEMM's dispatch table chooses what the five free-standing choices
chose: the label query, the two statistics-chunk queries and bnn_gemm_i8_bnstats_ok give every case of
tests/gemm_cases.py its recorded answer (tests/golden/gemm_dispatch.json); the exact instance of
every case and form (the host-only bnn_gemm_instance query, the same decision function the launching
entries consume) keeps the label a prefix key of it wherever label and launch are meant to agree,
and is the documented other row where they are not; and the cases reach every row
bnn_gemm_instance_at lists.

Where the row pitch passes the 32-bit tile offsets (K * 256 >= 2^31) every entry but the plain int8
one refuses, so its instance is ""; the label and chunk queries never looked at the pitch of those
forms and still answer, so the label / chunk assertions are made at the K the entries take.
No GPU: nothing here launches."""
import pytest

import gemm_cases as GC

PLAIN, I16, STATS, S20, BNSIGN = range(5)
FORMS = (PLAIN, I16, STATS, S20, BNSIGN)
# the forms each family's entries have
HAS = {"11": {PLAIN, STATS, S20, BNSIGN}, "31": {PLAIN}, "33": {PLAIN}, "fp4": {PLAIN, I16, STATS, BNSIGN}}

I8_BST = {128: "gemm_i8_v2_k<1, 1, 2, 2, 2, 2, 3, 64, 0, 0, 0, 1>", 256: "gemm_i8_v2_k<1, 1, 2, 4, 4, 2, 3, 64, 0, 0, 0, 1>"}
FP4_BST = {128: "gemm_fp4_k<2, 2, 2, 2, 3, 64, 0, 0, 1>", 256: "gemm_fp4_k<2, 4, 4, 2, 2, 128, 2, 1, 1>"}
I8_BNS = {128: "gemm_i8_bnsign_k<2, 2, 2, 2, 3, 64>", 256: "gemm_i8_bnsign_k<2, 4, 4, 2, 3, 64>"}
FP4_BNS = {128: "gemm_fp4_bnsign_k<2, 2, 2, 2, 3, 64, 0, 0>", 256: "gemm_fp4_bnsign_k<2, 4, 4, 2, 2, 128, 2, 1>"}
# rows per statistics partial = one wave row of the tile: 32 WM (the instance's WM argument)
CHUNK_OF = {I8_BST[128]: 64, I8_BST[256]: 128, FP4_BST[128]: 64, FP4_BST[256]: 128, "": 0}

# Rows no case may reach, with the reason.
NOT_REACHED = set()

# the first row past the variant ids of each family (an unknown or foreign forced id answers with it)
BASE1 = {"11": ("gemm_i8_v2_k<1, 1, 2, 2, 2, 2, 3, 64, 0, 0, 0>", "gemm_i8_v2_k<1, 1, 2, 2, 2, 2, 3, 64, 0, 0, 0, 0>"),
         "33": ("gemm_i8_v2_k<3, 3, 2, 2, 2, 1, 2, 64, 0, 0, 0>", "gemm_i8_v2_k<3, 3, 2, 2, 2, 1, 2, 64, 0, 0, 0, 0>"),
         "fp4": ("gemm_fp4_k<2, 2, 2, 2, 3, 64, 0, 0>", "gemm_fp4_k<2, 2, 2, 2, 3, 64, 0, 0>")}


def big(c):
    """At least 512 tiles of 256 x 256: the grid threshold of the (1,1) and FP4 families."""
    return ((c.M + 255) // 256) * ((c.N + 255) // 256) >= 512


def fits(c):
    """The row pitch stays inside the 32-bit tile offsets."""
    return c.K * 256 < 2 ** 31


def is_key_of(label, inst):
    """bench.py's matching rule: the label without its closing '>' starts the name, up to ',' or '>'."""
    p = label.rstrip(">")
    return inst.startswith(p) and inst[len(p):len(p) + 1] in (",", ">")


def args_of(inst):
    return inst[inst.find("<") + 1:-1].split(", ")


@pytest.fixture(scope="module")
def L():
    from bnn_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def recorded():
    return GC.recorded()


@pytest.fixture(scope="module")
def answers(L):
    return GC.answers(L)


@pytest.fixture(scope="module")
def instances(L):
    """The instance of every form, for every case: of the case's family, and (i8) of the (1,1) family,
    whose statistics forms bnn_gemm_i8_bnstats_chunk describes whatever the case's family."""
    def what(L, c):
        a, b = GC.FAMILIES[c.family]
        return ([L.bnn_gemm_instance(f, a, b, c.M, c.N, c.K).decode() for f in FORMS],
                [L.bnn_gemm_instance(f, 1, 1, c.M, c.N, c.K).decode() for f in (STATS, S20)])
    return GC.answers(L, what)


def listed(L):
    out = []
    while L.bnn_gemm_instance_at(len(out)):
        out.append(L.bnn_gemm_instance_at(len(out)).decode())
    return out


def test_table_is_well_formed(recorded):
    assert len(GC.CASES) == 4410 and len(set(GC.CASES)) == len(GC.CASES)
    assert set(recorded) == set(GC.CASES)
    # both sides of each grid threshold, of K % 128 and of the offset limit
    assert {big(c) for c in GC.CASES} == {True, False}
    assert {c.K % 128 == 0 for c in GC.CASES} == {True, False} and {fits(c) for c in GC.CASES} == {True, False}
    assert {((M + 127) // 128) * ((N + 255) // 256) for M, N in GC.SHAPES} >= {256, 224}
    assert {((M + 255) // 256) * ((N + 255) // 256) for M, N in GC.SHAPES} >= {512, 480}
    # no forced variant of the table reaches another family's row
    owner = {i: f for f, ids in (("11", list(range(10)) + [77, 78]), ("31", list(range(10, 20)) + [97, 98]),
                                 ("33", [20, 21, 22]), ("fp4", range(30, 40))) for i in ids}
    for f, vs in GC.VARIANTS.items():
        assert all(owner.get(GC.BASE[f] + v, f) == f for v in vs if v >= 0), f
        assert {GC.BASE[f] + v for v in vs if v >= 0} >= {i for i, g in owner.items() if g == f}, f
    assert len({a.kernel for a in recorded.values()}) == 37          # every row below 100 answers somewhere


def test_queries_give_the_recorded_answers(answers, recorded):
    bad = [(c, got, recorded[c]) for c, got in zip(GC.CASES, answers) if got != recorded[c]]
    assert not bad, (len(bad), bad[:5])


def test_switches_are_restored(L, answers, instances):
    assert GC.switches(L) == (-1, 0)


def test_label_is_a_prefix_key_of_the_instance(L, instances, recorded):
    """Forms 0 and 1 launch what the label names.  The FP4 statistics form follows the plan, so
    wherever it exists the label keys it.  The (1,1) statistics and s20 forms ignore the variant and
    obey bnstats_tile: the label keys them under the default switches on a small grid or with
    K % 128 != 0, and otherwise the instance is the BST row of the tile the switch selects, whatever
    the label says."""
    names = set(listed(L))
    bad = []
    for c, (inst, _) in zip(GC.CASES, instances):
        lab = recorded[c].kernel
        for f in FORMS:
            i = inst[f]
            if f not in HAS[c.family] or (not fits(c) and not (f == PLAIN and c.family != "fp4")) \
                    or (f == I16 and 2 * c.K > 32767):
                ok = i == ""                                            # no such entry, or it refuses
            elif f in (PLAIN, I16):
                ok = i in names and (lab.startswith("diag: ") or is_key_of(lab, i))
            elif f in (STATS, S20) and c.family == "11":
                tile = {0: 256 if big(c) else 128, 1: 128, 2: 256}[c.tile]
                ok = i == I8_BST[tile]
                if c.variant < 0 and c.tile == 0 and (c.K % 128 != 0 or not big(c)):
                    ok = ok and is_key_of(lab, i)
                elif c.variant < 0 and c.tile == 0:
                    ok = ok and not is_key_of(lab, i)               # the label is variant 9's, the launch row 2's BST
            elif f == STATS:                                            # FP4
                ok = i == "" or (i in FP4_BST.values() and is_key_of(lab, i))
            else:
                continue                                                # BN-sign: the test below
            if not ok:
                bad.append((c, f, i, lab))
    assert not bad, (len(bad), bad[:5])


def test_bnsign_instance_is_the_default_tiles(instances, recorded):
    """The BN-sign forms ignore both switches: the 256 x 256 tile on big grids (FP4: where K % 128
    == 0 too), else 128 x 128.  A *_bnsign_k instance carries its own kernel name, so the label keys
    it only through the name of the plain kernel of the same tile: under the default switches, the
    label's template arguments begin with the instance's (FP4: are the instance's) wherever the plain
    launch takes the same tile."""
    for c, (inst, _) in zip(GC.CASES, instances):
        i = inst[BNSIGN]
        if c.family not in ("11", "fp4") or not fits(c):
            assert i == "", (c, i)
            continue
        if c.family == "fp4":
            assert i == FP4_BNS[256 if big(c) and c.K % 128 == 0 else 128], (c, i)
            plain, agree = i.replace("gemm_fp4_bnsign_k<", "gemm_fp4_k<"), not (big(c) and c.K % 128 != 0)
        else:
            assert i == I8_BNS[256 if big(c) else 128], (c, i)
            plain, agree = i.replace("gemm_i8_bnsign_k<", "gemm_i8_v2_k<1, 1, "), not (big(c) and c.K % 128 == 0)
        if c.variant < 0:
            assert is_key_of(plain, recorded[c].kernel) == agree, (c, i, recorded[c].kernel)


def test_chunk_is_the_statistics_rows_chunk(instances, recorded):
    """bnn_gemm_i8_bnstats_chunk / bnn_gemm_fp4_bnstats_chunk give the chunk of the row the statistics
    and s20 launches run (32 WM rows), and the FP4 chunk is 0 exactly where there is no such row."""
    for inst in list(I8_BST.values()):
        assert CHUNK_OF[inst] == 32 * int(args_of(inst)[4])
    for inst in list(FP4_BST.values()):
        assert CHUNK_OF[inst] == 32 * int(args_of(inst)[2])
    for c, (inst, pix) in zip(GC.CASES, instances):
        if not fits(c):
            assert pix == ["", ""] and inst[STATS] == "", (c, pix, inst)
            continue
        assert recorded[c].i8_ok == 1
        assert CHUNK_OF[pix[0]] == CHUNK_OF[pix[1]] == recorded[c].i8_chunk, (c, pix)
        if c.family == "fp4":
            assert CHUNK_OF[inst[STATS]] == recorded[c].fp4_chunk, (c, inst[STATS])
            assert (inst[STATS] == "") == (recorded[c].fp4_chunk == 0)


def test_epilogue_shows_in_the_instance(instances):
    """What the labels cannot say: BST (the last template argument) is 1 on every statistics and s20
    instance; the plain and int16 forms never run a BST or BN-sign instance; the BN-sign form always
    runs a *_bnsign_k one."""
    for c, (inst, pix) in zip(GC.CASES, instances):
        for i in [inst[STATS], inst[S20]] + pix:
            if i:
                full = 12 if i.startswith("gemm_i8_v2_k<") else 9
                assert len(args_of(i)) == full and args_of(i)[-1] == "1", (c, i)
        for i in (inst[PLAIN], inst[I16]):
            assert "_bnsign_k<" not in i and i not in CHUNK_OF or i == "", (c, i)
            if i.startswith("gemm_i8_v2_k<"):
                assert args_of(i)[-1] == "0", (c, i)
        assert inst[BNSIGN] == "" or "_bnsign_k<" in inst[BNSIGN], (c, inst[BNSIGN])


def test_cases_reach_every_listed_instance(L, instances):
    names = listed(L)
    assert len(names) == len(set(names)) == 45
    assert L.bnn_gemm_instance_at(len(names)) == b"" and L.bnn_gemm_instance_at(-1) == b""
    assert NOT_REACHED <= set(names)
    reached = {i for inst, pix in instances for i in inst + pix if i}
    assert reached <= set(names), sorted(reached - set(names))
    assert not reached & NOT_REACHED
    lost = [n for n in names if n not in reached and n not in NOT_REACHED]
    assert not lost, f"no case reaches {lost}"


@pytest.mark.parametrize("family,variant", [("11", 10), ("11", 30), ("fp4", 47), ("33", 5)])
def test_a_variant_of_another_family_is_an_unknown_id(L, family, variant):
    """A forced id whose row belongs to another family (or to none) is answered by the family's row
    base + 1, in the label and in the instance alike."""
    a, b = GC.FAMILIES[family]
    prev = GC.switches(L)
    try:
        GC.set_switches(L, variant, 0)
        for M, N, K in ((64, 64, 64), (8192, 4096, 1024)):
            assert L.bnn_gemm_i8_kernel(a, b, M, N, K).decode() == BASE1[family][0]
            assert L.bnn_gemm_instance(PLAIN, a, b, M, N, K).decode() == BASE1[family][1]
    finally:
        GC.set_switches(L, *prev)


def test_instance_query_answers_for_bad_arguments(L):
    assert L.bnn_gemm_instance(0, 1, 1, 0, 4096, 1024) == b""
    assert L.bnn_gemm_instance(0, 1, 1, 8192, 0, 1024) == b""
    assert L.bnn_gemm_instance(0, 1, 1, 8192, 4096, 1000) == b""       # K % 64 != 0
    assert L.bnn_gemm_instance(5, 1, 1, 8192, 4096, 1024) == b"" and L.bnn_gemm_instance(-1, 1, 1, 8192, 4096, 1024) == b""
    for a, b in ((1, 3), (2, 1), (3, 2), (4, 4), (-1, 1)):
        assert L.bnn_gemm_instance(0, a, b, 8192, 4096, 1024) == b"", (a, b)
    assert L.bnn_gemm_instance(0, 1, 1, 8192, 4096, 1024) == b"gemm_i8_v2_k<1, 1, 2, 4, 4, 2, 2, 128, 2, 0, 1, 0>"
    assert L.bnn_gemm_instance(2, 1, 1, 8192, 4096, 1024) == I8_BST[256].encode()     # where the label says variant 9
    assert L.bnn_gemm_instance(0, 0, 0, 8192, 4096, 1024) == b"gemm_fp4_k<2, 4, 4, 2, 2, 128, 2, 1>"
