"""CPU proof that tests/bn_cases.py covers the BatchNorm schedules: the host-only bnn_bn_plan and
bnn_bn2d_plan queries (the decision functions the launching entries consume) give every case's
recorded plan, the 1d table reaches every class named in bn_cases.CLASSES_1D, the 2d table under each
of bnn_bn2d_set_rows 0, 1 and 2 reaches every value of every field bnn_bn2d_plan reports, and no case
can be deleted without losing a class (the failure names it).  No GPU: nothing here launches."""
import pytest

import bn_cases as BC


@pytest.fixture(scope="module")
def L():
    from bnn_amd import _lib
    return _lib.lib()


@pytest.fixture()
def rows_restored(L):
    prev = BC.rows_setting(L)
    yield
    L.bnn_bn2d_set_rows(prev)


def test_1d_query_gives_the_recorded_plans(L):
    bad = [(BC.id_1d(c), BC.plan_1d(L, c.M, c.C), tuple(c[2:])) for c in BC.CASES_1D
           if BC.plan_1d(L, c.M, c.C) != tuple(c[2:])]
    assert not bad, bad


def test_1d_plan_is_consistent_with_the_shape(L):
    for c in BC.CASES_1D:
        assert c.R == -(-c.M // c.chunk) and c.gy == -(-c.M // c.apply_rows) and c.gx == -(-(c.C // 4) // 256), c
        assert c.kb == (1 if c.chunk % 8 == 0 else 0), c
        assert c.C % 4 == 0 and c.M * c.C <= (17 << 20) or c == BC.LARGE_1D, c
    assert BC.LARGE_1D in BC.CASES_1D and len(BC.SMALL_1D) == len(BC.CASES_1D) - 1
    assert {c.chunk for c in BC.DROPOUT_1D} == {16, 32}


def test_1d_table_reaches_every_class():
    lost = sorted(set(BC.CLASSES_1D) - BC.classes_1d(BC.CASES_1D))
    assert not lost, f"no 1d case reaches {lost}"


@pytest.mark.parametrize("case", BC.CASES_1D, ids=BC.id_1d)
def test_1d_case_cannot_be_deleted(case):
    """Each case is the only provider of at least one class; this names what its deletion loses."""
    rest = [c for c in BC.CASES_1D if c != case]
    lost = sorted(BC.classes_1d(BC.CASES_1D) - BC.classes_1d(rest))
    assert lost, f"{BC.id_1d(case)} is redundant: every class it reaches another case reaches too"


def test_1d_deleting_a_case_is_noticed_by_name():
    """The coverage test's own message for a deleted case (here: the 8-row chunk case)."""
    rest = [c for c in BC.CASES_1D if c.chunk != 8]
    assert sorted(set(BC.CLASSES_1D) - BC.classes_1d(rest)) == ["chunk rows 8"]


def test_1d_query_refuses_what_the_entries_refuse(L):
    for M, C in ((0, 4), (-1, 4), (4, 0), (4, 6), (4, 3), (65536 * 64, 4)):
        assert BC.plan_1d(L, M, C) is None, (M, C)
    assert L.bnn_bn_plan(4, 4, None) == -1
    assert BC.plan_1d(L, 65536, 8192) == (256, 256, 64, 8, 1024, 1)      # the bench's workload


def test_2d_query_gives_the_recorded_plans(L, rows_restored):
    bad = []
    for rows in (0, 1, 2):
        L.bnn_bn2d_set_rows(rows)
        assert BC.rows_setting(L) == rows
        for c in BC.CASES_2D:
            for pool in (0, 2):
                got = BC.plan_2d(L, c.N, c.C, c.H, c.W, pool)
                if got != c.plans[(rows, pool)]:
                    bad.append((BC.id_2d(c), rows, pool, got, c.plans[(rows, pool)]))
    assert not bad, bad


def test_2d_table_reaches_every_field_value_and_class():
    for c in BC.CASES_2D:
        assert c.N <= 9 and set(c.plans) == {(r, p) for r in (0, 1, 2) for p in (0, 2)}, c
    lost = sorted(set(BC.CLASSES_2D) - BC.classes_2d(BC.CASES_2D))
    assert not lost, f"no 2d case reaches {lost}"
    # every value of every field the query reports, per bnn_bn2d_set_rows setting that can give it
    for f, want in (("fwd_stats", {0, 1}), ("fwd_apply", {0, 7, 14}), ("bwd_stats", {0, 7, 14}),
                    ("bwd_apply", {0, 7, 14})):
        i = BC.FIELDS_2D.index(f)
        assert {p[i] for c in BC.CASES_2D for p in c.plans.values()} == want, f
    for rows, want in ((0, (0, 0, 0, 0)), (1, (1, 14, 14, 0)), (2, (1, 14, 14, 14))):
        assert any(c.plans[(rows, 2)][2:] == want for c in BC.CASES_2D), rows
        assert any(c.plans[(rows, 2)][2:] == tuple(7 if v == 14 else v for v in want) for c in BC.CASES_2D), rows


@pytest.mark.parametrize("case", BC.CASES_2D, ids=BC.id_2d)
def test_2d_case_cannot_be_deleted(case):
    rest = [c for c in BC.CASES_2D if c != case]
    lost = sorted(BC.classes_2d(BC.CASES_2D) - BC.classes_2d(rest))
    assert lost, f"{BC.id_2d(case)} is redundant: every class it reaches another case reaches too"


def test_2d_query_refuses_what_the_entries_refuse(L):
    for shape in ((0, 4, 4, 4, 0), (1, 0, 4, 4, 0), (1, 4, 3, 3, 0), (1, 4, 2, 6, 1), (1, 4, 6, 6, 3),
                  (1, 4, 4, 3, 2), (1, 65536, 2, 2, 0)):
        assert BC.plan_2d(L, *shape) is None, shape
    assert BC.plan_2d(L, 1, 4, 2, 6, 0) is not None and BC.plan_2d(L, 1, 4, 2, 6, 2) is not None


def test_2d_switch_is_restored(L, rows_restored):
    L.bnn_bn2d_set_rows(2)
    assert BC.rows_setting(L) == 2
    L.bnn_bn2d_set_rows(7)                  # out of range: the default
    assert BC.rows_setting(L) == 1
