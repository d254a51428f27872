"""CPU proof that the FP6 GEMM's dispatch table chooses what the free-standing predicates chose:
the three label queries and bnn_gemm_fp6_workspace give every case of tests/fp6_cases.py its
recorded answer (tests/golden/fp6_dispatch.json), the exact instance of every case (the host-only
bnn_gemm_fp6_instance query, the same decision function the launching entries consume) maps to the
recorded label, and the cases reach every row bnn_gemm_fp6_instance_at lists.
No GPU: nothing here launches."""
import pytest

import fp6_cases as FC

DEFAULT = "gemm_fp6_k<2, 4, 2, 4, 2>"
HALF = "gemm_fp6_k<1, 4, 2, 4, 2>"
WIDE = "gemm_fp6_k<1, 8, 2, 4, 2, 0, 2, 0, 0, 0, 1>"
PERS = "gemm_fp6_pers_k<2, 4, 2, 4, 2>"

# Rows no case may reach, with the reason.
NOT_REACHED = {
    # the BatchNorm-statistics epilogue: only bnn_gemm_fp6_bnstats launches these, and the instance
    # query describes bnn_gemm_fp6_ws / bnn_gemm_fp6_panel_ws
    "gemm_fp6_k<2, 4, 2, 4, 2, 0, 2, 0, 1>",
    "gemm_fp6_k<2, 4, 2, 4, 2, 0, 2, 0, 1, 1>",
}

# exact instance -> label, for the instances whose label is not their own string: the residual-plane,
# B-in-registers and persistent instances report the tile they run on
LABEL_OF = {
    "gemm_fp6_k<2, 4, 2, 4, 2, 0, 2, 0, 0, 1>": DEFAULT,
    "gemm_fp6_k<1, 4, 2, 4, 2, 0, 2, 0, 0, 1>": HALF,
    "gemm_fp6_k<1, 4, 2, 4, 2, 0, 2, 0, 0, 0, 1>": HALF,
    "gemm_fp6_k<1, 4, 2, 4, 2, 0, 2, 0, 0, 1, 1>": HALF,
    "gemm_fp6_pers_k<0>": PERS,
    "gemm_fp6_pers_k<1>": PERS,
    "gemm_fp6_k<2, 4, 2, 4, 3, 1>": "diag: v5 without global->LDS staging",
    "gemm_fp6_k<2, 4, 2, 4, 3, 2>": "diag: v5 without LDS fragment reads",
    "gemm_fp6_k<2, 4, 2, 4, 2, 3>": "diag: v7 MFMA stream + barrier",
    "gemm_fp6_k<2, 4, 2, 4, 2, 4>": "diag: v7 MFMA stream only",
    "gemm_fp6_k<2, 4, 2, 4, 2, 1>": "diag: v7 without global->LDS staging",
    "gemm_fp6_k<2, 4, 2, 4, 2, 2>": "diag: v7 without LDS fragment reads",
    "gemm_fp6_k<2, 4, 2, 4, 2, 5>": "diag: v7 with B staged from contiguous panels",
    "gemm_fp6_k<2, 4, 2, 4, 2, 6>": "diag: v7 with B and A hi staged from contiguous panels",
}
BREG = {WIDE, "gemm_fp6_k<1, 4, 2, 4, 2, 0, 2, 0, 0, 0, 1>", "gemm_fp6_k<1, 4, 2, 4, 2, 0, 2, 0, 0, 1, 1>"}


def base(name):
    """An instance or label without its " split-K S" suffix."""
    return name.split(" split-K ")[0]


@pytest.fixture(scope="module")
def L():
    from bnn_amd import _lib
    lib = _lib.lib()
    try:
        import torch
        if torch.cuda.is_available() and torch.cuda.get_device_properties(0).multi_processor_count != FC.CUS:
            pytest.skip(f"the table is recorded for {FC.CUS} compute units")
    except ImportError:
        pass
    return lib


@pytest.fixture(scope="module")
def recorded():
    return FC.recorded()


@pytest.fixture(scope="module")
def answers(L):
    return FC.answers(L)


@pytest.fixture(scope="module")
def instances(L):
    """(instance with panels, instance with a row-major B) of every case."""
    return FC.answers(L, lambda L, c: (L.bnn_gemm_fp6_instance(c.M, c.N, c.K, c.res, 1).decode(),
                                       L.bnn_gemm_fp6_instance(c.M, c.N, c.K, c.res, 0).decode()))


def listed(L):
    out = []
    while L.bnn_gemm_fp6_instance_at(len(out)):
        out.append(L.bnn_gemm_fp6_instance_at(len(out)).decode())
    return out


def test_table_is_well_formed(recorded):
    assert len(FC.GRID) == 1800 and len(set(FC.CASES)) == len(FC.CASES)
    assert set(recorded) == set(FC.CASES)
    kr = {base(a.kernel_kr) for c, a in recorded.items() if c in set(FC.GRID)}
    assert {DEFAULT, HALF, WIDE, PERS, "gemm_fp6_k<2, 4, 2, 4, 3>"} <= kr            # default, half, wide,
    assert any(" split-K " in a.kernel_kr for a in recorded.values())                # persistent, forced, split-K
    # the forced wide mode keeps a split-K shape it divides unsplit
    assert recorded[FC.Case(768, 2048, 4096, 0, -1, 0, 1, 1)].workspace == 8 * 768 * 2048 * 4
    assert recorded[FC.Case(768, 2048, 4096, 0, -1, 0, 1, 2)].workspace == 0


def test_queries_give_the_recorded_answers(answers, recorded):
    bad = [(c, got, recorded[c]) for c, got in zip(FC.CASES, answers) if got != recorded[c]]
    assert not bad, (len(bad), bad[:5])


def test_switches_are_restored(L, answers):
    assert FC.switches(L) == (-1, 0, 1, 1)


def test_exact_instance_maps_to_the_recorded_label(L, instances, recorded):
    """The instance of a panel launch carries the label bnn_gemm_fp6_kernel_kr recorded for the case
    and the same split; a residual plane with a forced variant other than 7 is refused."""
    names = set(listed(L))
    bad = []
    for c, (inst, _) in zip(FC.CASES, instances):
        want = recorded[c].kernel_kr
        if c.res and c.variant >= 0 and c.variant != 7:
            ok = inst == ""
        else:
            ok = (base(inst) in names and LABEL_OF.get(base(inst), base(inst)) == base(want)
                  and inst[len(base(inst)):] == want[len(base(want)):])
        if not ok:
            bad.append((c, inst, want))
    assert not bad, (len(bad), bad[:5])


def test_residual_plane_and_form_show_in_the_instance(L, instances):
    """What the labels cannot say: RES (the 10th template argument) follows `res` on every form that
    carries the plane, and the half tile's BREG instance follows the mode."""
    for c, (inst, _) in zip(FC.CASES, instances):
        args = base(inst)[base(inst).find("<") + 1:-1].split(", ")
        if inst.startswith("gemm_fp6_pers_k"):
            assert args == [str(c.res)], (c, inst)
        elif inst and c.variant < 0:
            assert (len(args) >= 10 and args[9] == "1") == bool(c.res), (c, inst)
        if LABEL_OF.get(base(inst)) == HALF or base(inst) == HALF:
            if c.variant < 0:
                assert (base(inst) in BREG) == (c.half <= 2), (c, inst)


def test_row_major_b_never_takes_a_b_in_registers_or_wide_instance(instances):
    for c, (with_panels, row_major) in zip(FC.CASES, instances):
        assert base(row_major) not in BREG, (c, row_major)
        assert not row_major.startswith("gemm_fp6_pers_k"), (c, row_major)          # persistent needs panels too
        if base(with_panels) not in BREG and not with_panels.startswith("gemm_fp6_pers_k"):
            assert row_major == with_panels, (c, with_panels, row_major)


def test_cases_reach_every_listed_instance(L, instances):
    names = listed(L)
    assert len(names) == len(set(names)) == 35
    assert L.bnn_gemm_fp6_instance_at(len(names)) == b"" and L.bnn_gemm_fp6_instance_at(-1) == b""
    assert NOT_REACHED <= set(names)
    reached = {base(i) for pair in instances for i in pair if i}
    assert reached <= set(names), sorted(reached - set(names))
    assert not reached & NOT_REACHED
    lost = [n for n in names if n not in reached and n not in NOT_REACHED]
    assert not lost, f"no case reaches {lost}"


def test_instance_query_answers_for_bad_arguments(L):
    assert L.bnn_gemm_fp6_instance(0, 4096, 1024, 0, 1) == b""
    assert L.bnn_gemm_fp6_instance(8192, 0, 1024, 0, 1) == b""
    assert L.bnn_gemm_fp6_instance(8192, 4096, 1000, 0, 1) == b""       # K % 64 != 0
    assert L.bnn_gemm_fp6_instance(8192, 4096, 1024, 1, 1) == b"gemm_fp6_k<1, 4, 2, 4, 2, 0, 2, 0, 0, 1, 1>"
    assert L.bnn_gemm_fp6_instance(768, 1536, 4096, 1, 1) == b"gemm_fp6_k<2, 4, 2, 4, 2, 0, 2, 0, 0, 1> split-K 8"
    assert L.bnn_gemm_fp6_instance(768, 1538, 4096, 0, 1) == DEFAULT.encode()   # N % 4 != 0: the sum kernel cannot fold it
