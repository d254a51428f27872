"""Case tables of the element-wise BatchNorm tests (tests/test_gpu_bn_elementwise.py), found with the
host-only bnn_bn_plan / bnn_bn2d_plan queries, each case with the plan the query must give.
tests/test_bn_plan.py (CPU) proves the recorded plans are the query's answers and that the tables
cover every schedule class named below; deleting a case loses a class that test names.

BatchNorm1d plan (bnn_bn_plan): rows per reduction chunk, chunk count R, rows per apply workgroup, the
apply grid (x, y), keep_bits_fused.  bn_reduce_k walks a chunk in 16-row fp32 folds of 8-row load
batches; the merges (bn_fwd_final_k, bn_bwd_final_body) take rounds of 128 chunks, 16 columns per
workgroup; the apply passes take 1024 columns x `apply rows` rows per workgroup."""
import ctypes
from collections import namedtuple

Case1 = namedtuple("Case1", "M C chunk R apply_rows gx gy kb")

CASES_1D = [
    #      M     C  chunk     R  rows gx    gy kb
    Case1(1,     4,   1,      1,  4,  1,    1, 0),
    Case1(3,    20,   1,      3,  4,  1,    1, 0),
    Case1(7,    12,   1,      7,  4,  1,    2, 0),
    Case1(300,  64,   1,    300,  4,  1,   75, 0),
    Case1(131, 1028,  1,    131,  4,  2,   33, 0),
    Case1(2053, 256,  2,   1027,  4,  1,  514, 0),
    Case1(2059, 512,  4,    515,  4,  1,  515, 0),
    Case1(1021, 2048, 8,    128,  4,  2,  256, 1),
    Case1(4117, 1024, 16,   258,  4,  1, 1030, 1),
    Case1(4117, 2048, 32,   129,  4,  2, 1030, 1),
    Case1(4131, 4096, 64,    65,  8,  4,  517, 1),
    Case1(8205, 8192, 256,   33, 32,  8,  257, 1),
]
LARGE_1D = Case1(8205, 8192, 256, 33, 32, 8, 257, 1)     # 67 M elements: run once per pass
SMALL_1D = [c for c in CASES_1D if c != LARGE_1D]          # at most 17 M elements each
DROPOUT_1D = [c for c in CASES_1D if c.chunk in (16, 32)]


def last_rows(c):
    return c.M - (c.R - 1) * c.chunk


# name -> predicate.  Every name must be reached; the first block is what the issue lists, the second
# makes each case the only one of its kind (so that none can be deleted unnoticed).
CLASSES_1D = {
    "chunk rows 1": lambda c: c.chunk == 1,
    "chunk rows 2": lambda c: c.chunk == 2,
    "chunk rows 4": lambda c: c.chunk == 4,
    "chunk rows 8": lambda c: c.chunk == 8,
    "chunk rows 16": lambda c: c.chunk == 16,
    "chunk rows 32": lambda c: c.chunk == 32,
    "chunk rows 64": lambda c: c.chunk == 64,
    "chunk rows 256": lambda c: c.chunk == 256,
    "last chunk shorter than the others": lambda c: c.R > 1 and last_rows(c) < c.chunk,
    "last chunk: a full 8-row batch plus a partial one": lambda c: 8 < last_rows(c) % 16 < 16,
    "last chunk: a partial 8-row batch alone": lambda c: c.chunk >= 8 and 0 < last_rows(c) % 16 < 8,
    "last chunk: a whole 16-row fold plus a remainder": lambda c: last_rows(c) > 16 and last_rows(c) % 16 != 0,
    "R = 1": lambda c: c.R == 1,
    "R in 2..16": lambda c: 2 <= c.R <= 16,
    "R in 17..128": lambda c: 17 <= c.R <= 128,
    "R > 128, R % 16 != 0": lambda c: c.R > 128 and c.R % 16 != 0,
    "C % 16 != 0": lambda c: c.C % 16 != 0,
    "C > 1024, ragged last column block": lambda c: c.C > 1024 and (c.C // 4) % 256 != 0,
    "M % apply rows != 0, several row blocks": lambda c: c.M % c.apply_rows != 0 and c.gy > 1,
    "apply rows 4": lambda c: c.apply_rows == 4,
    "apply rows 8": lambda c: c.apply_rows == 8,
    "apply rows 32": lambda c: c.apply_rows == 32,
    "keep bits by their own kernel": lambda c: c.kb == 0,
    "keep bits by the statistics pass": lambda c: c.kb == 1,
    # the single-provider classes of the chunk-rows-1 cases
    "M = 1": lambda c: c.M == 1,
    "R in 2..16, dead merge lanes beside a full 16-column block": lambda c: 2 <= c.R <= 16 and c.C > 16 and c.C % 16 != 0,
    "R in 2..16, apply row tail": lambda c: 2 <= c.R <= 16 and c.gy > 1 and c.M % c.apply_rows != 0,
    "chunk rows 1, R > 128, one column block": lambda c: c.chunk == 1 and c.R > 128 and c.gx == 1,
}


def classes_1d(cases):
    return {name for name, pred in CLASSES_1D.items() if any(pred(c) for c in cases)}


def plan_1d(L, M, C):
    out = (ctypes.c_int64 * 6)()
    return None if L.bnn_bn_plan(M, C, out) != 0 else tuple(out)


def id_1d(c):
    return f"{c.M}x{c.C}"


# ------------------------------------------------------------------------------------- BatchNorm2d
# bnn_bn2d_plan: images per chunk CR, chunk count R, forward statistics (1 flat / 0 window), forward
# apply, backward statistics, backward apply (14 / 7 row kernels, 0 window kernels).  `plans` maps
# (bnn_bn2d_set_rows value, pool) -> that tuple.  bn2d_fwd_stats_flat_k takes rounds of 1024
# four-element groups per chunk; bn2d_reduce_k<0> spreads images over the workgroup when a plane has
# fewer than 256 groups; the row kernels take 256 (plane, pooled row) pairs per workgroup.
Case2 = namedtuple("Case2", "N C H W plans")


def _plans(CR, R, pw):
    """The dispatch for a plane whose pooled width the row kernels take (pw = 14 / 7) or not (0)."""
    return {(rows, pool): (CR, R, 1 if rows else 0, pw if (rows and pool) else 0, pw if (rows and pool) else 0,
                           pw if (rows == 2 and pool) else 0)
            for rows in (0, 1, 2) for pool in (0, 2)}


CASES_2D = [
    Case2(5, 16, 28, 28, _plans(1, 5, 14)),      # HW/4 = 196; 5*16*14 = 1120 row pairs: 4 workgroups + 96
    Case2(9, 32, 14, 14, _plans(1, 9, 7)),       # HW/4 = 49; 2016 row pairs: 7 workgroups + 224
    Case2(3, 8, 6, 10, _plans(1, 3, 0)),         # HW/4 = 15, another width
    Case2(2, 4, 32, 32, _plans(1, 2, 0)),        # HW/4 = 256: one group per thread; flat total 256 < 1024
    Case2(5, 1024, 4, 4, _plans(3, 2, 0)),       # CR = 3, last chunk 2 images
    Case2(2, 4, 64, 64, _plans(1, 2, 0)),        # flat total = 1024: exactly one round
    Case2(2, 4, 72, 64, _plans(1, 2, 0)),        # flat total = 1152: one round and a partial one
]

FIELDS_2D = ("CR", "R", "fwd_stats", "fwd_apply", "bwd_stats", "bwd_apply")
CLASSES_2D = {
    "CR = 1": lambda c, p: p[0] == 1,
    "CR > 1, short last chunk": lambda c, p: p[0] > 1 and c.N % p[0] != 0,
    "forward statistics: window": lambda c, p: p[2] == 0,
    "forward statistics: flat": lambda c, p: p[2] == 1,
    "forward apply: window": lambda c, p: p[3] == 0,
    "forward apply: rows<7>": lambda c, p: p[3] == 7,
    "forward apply: rows<14>": lambda c, p: p[3] == 14,
    "backward statistics: window": lambda c, p: p[4] == 0,
    "backward statistics: rows<7>": lambda c, p: p[4] == 7,
    "backward statistics: rows<14>": lambda c, p: p[4] == 14,
    "backward apply: window": lambda c, p: p[5] == 0,
    "backward apply: rows<7>": lambda c, p: p[5] == 7,
    "backward apply: rows<14>": lambda c, p: p[5] == 14,
    "HW/4 >= 256": lambda c, p: c.H * c.W // 4 >= 256,
    "HW/4 = 196": lambda c, p: c.H * c.W // 4 == 196,
    "HW/4 = 49": lambda c, p: c.H * c.W // 4 == 49,
    "HW/4 = 15": lambda c, p: c.H * c.W // 4 == 15,
    "flat total < 1024": lambda c, p: p[2] == 1 and p[0] * (c.H * c.W // 4) < 1024,
    "flat total = 1024": lambda c, p: p[2] == 1 and p[0] * (c.H * c.W // 4) == 1024,
    "flat total > 1024, partial last round": lambda c, p: p[2] == 1 and p[0] * (c.H * c.W // 4) > 1024
    and p[0] * (c.H * c.W // 4) % 1024 != 0,
    "flat total < 1024, images of 256 groups": lambda c, p: p[2] == 1 and c.H * c.W // 4 == 256,
    "row kernels: N C H/2 % 256 != 0": lambda c, p: p[3] != 0 and (c.N * c.C * (c.H // 2)) % 256 != 0,
    "width 28": lambda c, p: c.W == 28,
    "width 14": lambda c, p: c.W == 14,
    "another width": lambda c, p: c.W not in (14, 28),
}


def classes_2d(cases):
    return {name for name, pred in CLASSES_2D.items()
            if any(pred(c, p) for c in cases for p in c.plans.values())}


def plan_2d(L, N, C, H, W, pool):
    """(CR, R, fwd_stats, fwd_apply, bwd_stats, bwd_apply) under the current bnn_bn2d_set_rows."""
    out = (ctypes.c_int64 * 7)()
    return None if L.bnn_bn2d_plan(N, C, H, W, pool, out) != 0 else tuple(out)[:6]


def rows_setting(L):
    out = (ctypes.c_int64 * 7)()
    assert L.bnn_bn2d_plan(1, 1, 2, 2, 0, out) == 0
    return int(out[6])


def id_2d(c):
    return f"{c.N}x{c.C}x{c.H}x{c.W}"
