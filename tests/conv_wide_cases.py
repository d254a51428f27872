"""The wide-channel conv family's case table: every shape the four bit-exact GPU
tests run, with the kernel template instance each op must reach for it.

A training case is a shape (N, C, H, W, Co, KH, KW, pad) plus the leading `name<...>` of
bnn_conv2d_fwd_wide_kernel, bnn_conv2d_bwd_data_wide_kernel and bnn_conv2d_bwd_filter_wide_kernel; an
infer case is (N, C, H, W, Co, KH, KW, pad, pool, consumer (K2, pad2) or None for int8 signs NCHW) plus
that of bnn_conv2d_fwd_wide_bnsign_kernel.  An empty string means the op refuses the shape: the GPU
tests skip an op by this string, never by a run-time _ok call, so a new refusal is a failure.

SHAPES and INFER_CASES are the seven shapes and seven cases the family was merged with, unchanged (the
generators seed from N, C and Co, so their inputs are unchanged too).  NEW_SHAPES and NEW_INFER_CASES
were found by reading the plan functions against those and querying the CPU build for what had never
been launched; the comment of each names what it adds.

Instances of conv_wide_bwd_filter_k<NT, NBUF> no shape reaches, at any size: <1, 1>.  NT = 1 is a 1 x 1
kernel, whose tap group has no halo, so its two-stage ring of 2 x 4 x 16 pieces always fits the LDS
and the plan never falls back to one stage.  <3, 1> and <5, 1> need a KW = 1 kernel on a row of more
than 512 / 256 columns (the halo of KH - 1 rows must crowd the second stage out); the table has both.

Shared by test_conv_wide_cases.py (CPU: the table reaches what it says) and the four test_gpu_conv_wide*
files (the kernels compute what float64 computes).
"""
import collections
import re

Train = collections.namedtuple("Train", "shape fwd data filt what")
Infer = collections.namedtuple("Infer", "case inst what")

G1, G2 = "conv_wide_gemm_k<1>", "conv_wide_gemm_k<2>"
D1, D2 = "conv_wide_bwd_data_k<1>", "conv_wide_bwd_data_k<2>"


def _f(nt, nbuf):
    return f"conv_wide_bwd_filter_k<{nt}, {nbuf}>"


def _b(nbuf, pool, form):
    return f"conv_wide_bnsign_k<{nbuf},{pool},{form}>"


# (N, C, H, W, Co, KH, KW, pad)
SHAPES = [
    (1, 64, 5, 7, 65, 3, 3, 1),        # Co tail, plane smaller than a tile
    (3, 128, 9, 11, 129, 3, 3, 1),     # two channel blocks, two co tiles, tiles crossing image boundaries
    (2, 64, 6, 6, 128, 1, 1, 0),       # no shift
    (2, 64, 7, 9, 72, 3, 3, 2),        # pad = K - 1
    (1, 64, 12, 13, 80, 5, 5, 0),      # 5x5 (one LDS stage), no padding
    (2, 192, 8, 8, 16, 1, 3, 0),       # non-square kernel, narrow Co, three blocks
    (5, 64, 33, 34, 130, 3, 3, 1),     # more positions than one round of tiles per image, odd Wp
]
NO_BIAS = NO_DB = SHAPES[3]

NEW_SHAPES = [
    (1, 64, 3, 170, 65, 3, 3, 1),      # three 64-column passes in every pack; single-stage 3x3; 28 K slices
    (2, 64, 5, 6, 65, 2, 2, 1),        # even kernel; 4 taps in a 5-set instance (the partial path)
    (2, 64, 7, 9, 72, 5, 3, 1),        # two tap groups, the last 2 kh rows of 3; non-square
    (2, 64, 7, 9, 72, 4, 3, 1),        # two tap groups, the last one row (no halo, in a ring sized for one)
    (1, 64, 4, 150, 65, 2, 4, 1),      # KW = 4; 8 taps of 9; W > 128; the filter's LDS exactly 160 KiB
    (1, 256, 4, 4, 65, 3, 3, 1),       # four channel blocks
    (1, 64, 3, 640, 65, 3, 3, 1),      # single-stage 3x3 forward; ten pack passes.  Forward only
    (1, 64, 3, 520, 65, 3, 1, 0),      # KW = 1 on a 520-column row: the filter's <3, 1>; nine pack passes
    (1, 64, 5, 260, 65, 5, 1, 0),      # KW = 1, KH = 5 on a 260-column row: the filter's <5, 1>
]
NO_DB_NEW = NEW_SHAPES[0]              # the filter gradient without db on a multi-pass shape

TRAIN = [Train(s, *v) for s, v in zip(SHAPES + NEW_SHAPES, [
    (G2, D2, _f(9, 2), "Co tail"),
    (G2, D2, _f(9, 2), "two blocks, short last K slice"),
    (G2, D2, _f(1, 2), "1x1"),
    (G2, D2, _f(9, 2), "pad = K - 1"),
    (G1, D1, _f(5, 2), "5x5, five tap groups"),
    (G2, D2, _f(3, 2), "1x3, three blocks"),
    (G2, D2, _f(9, 2), "many tiles"),
    (G2, D1, _f(9, 1), "three pack passes, single-stage 3x3 backward"),
    (G2, D2, _f(5, 2), "even kernel, partial tap group"),
    (G2, D2, _f(9, 2), "last tap group of 2 rows"),
    (G2, D2, _f(9, 2), "last tap group of 1 row"),
    (G2, D2, _f(9, 2), "KW = 4, 8 taps of 9"),
    (G2, D2, _f(9, 2), "four channel blocks"),
    (G1, "", "", "single-stage 3x3 forward, ten pack passes"),
    (G2, D1, _f(3, 1), "single-stage three-tap filter"),
    (G2, D1, _f(5, 1), "single-stage five-tap filter"),
])]

# (N, C, H, W, Co, KH, KW, pad, pool, consumer (K2, pad2) or None for int8 signs NCHW)
INFER_CASES = [
    (1, 64, 6, 6, 65, 3, 3, 1, 0, None),          # Co tail, plane smaller than a tile
    (3, 128, 10, 12, 128, 3, 3, 1, 2, (3, 1)),    # two blocks; windows and tiles crossing image boundaries
    (2, 64, 8, 8, 64, 1, 1, 0, 2, (1, 0)),        # no shift; consumer without halo
    (2, 64, 6, 10, 192, 3, 3, 2, 2, (5, 2)),      # pad = K - 1; wide halo; three output blocks
    (1, 64, 12, 14, 80, 5, 5, 0, 2, None),        # one LDS stage
    (5, 64, 34, 34, 130, 3, 3, 1, 2, None),       # more windows than one round of tiles; row ends inside a wave
    (2, 192, 9, 7, 64, 3, 3, 1, 0, (3, 1)),       # odd sizes without pool
]

NEW_INFER_CASES = [
    (2, 64, 7, 7, 64, 2, 2, 0, 2, (3, 1)),        # Wp = 7 odd, Wpe = 8: the padded column and the pairing across it
    (3, 64, 5, 7, 64, 2, 2, 1, 2, (1, 0)),        # Wp = 9 odd, pad = K - 1, windows crossing images
    (2, 64, 7, 9, 128, 4, 2, 1, 2, None),         # Wp = 11 odd, non-square
    (1, 64, 12, 14, 128, 5, 5, 0, 2, (3, 1)),     # one stage, pooled, planes
    (1, 64, 12, 14, 128, 5, 5, 0, 0, (3, 1)),     # one stage, planes
    (1, 64, 12, 14, 80, 5, 5, 0, 0, None),        # one stage, int8
    (1, 64, 4, 130, 65, 3, 3, 1, 2, None),        # pack_x over three passes; long window rows
    (1, 256, 6, 6, 64, 3, 3, 1, 2, (3, 1)),       # four channel blocks
]
NULL_CASES = [NEW_INFER_CASES[0], NEW_INFER_CASES[5]]     # null bias / gamma / beta: pooled planes, int8

INFER = [Infer(c, *v) for c, v in zip(INFER_CASES + NEW_INFER_CASES, [
    (_b(2, 0, 1), "Co tail"),
    (_b(2, 2, 0), "two blocks"),
    (_b(2, 2, 0), "1x1"),
    (_b(2, 2, 0), "pad = K - 1"),
    (_b(1, 2, 1), "one stage, pooled, int8"),
    (_b(2, 2, 1), "many tiles"),
    (_b(2, 0, 0), "three blocks, no pool"),
    (_b(2, 2, 0), "odd Wp = 7"),
    (_b(2, 2, 0), "odd Wp = 9, pad = K - 1"),
    (_b(2, 2, 1), "odd Wp = 11, int8"),
    (_b(1, 2, 0), "one stage, pooled, planes"),
    (_b(1, 0, 0), "one stage, planes"),
    (_b(1, 0, 1), "one stage, int8"),
    (_b(2, 2, 1), "three pack passes"),
    (_b(2, 2, 0), "four channel blocks"),
])]

FILTER_UNREACHABLE = {_f(1, 1)}
FILTER_INSTANCES = {_f(nt, nbuf) for nt in (1, 3, 5, 9) for nbuf in (1, 2)}

EMPTY = (0, 128, 8, 8, 128, 3, 3, 1)              # the empty batch at the C ABI


def shape_id(s):
    N, C, H, W, Co, KH, KW, pad = s[:8]
    tail = "" if len(s) == 8 else f"-pool{s[8]}-" + ("i8" if s[9] is None else "k%dp%d" % s[9])
    return f"n{N}c{C}h{H}w{W}o{Co}k{KH}x{KW}p{pad}{tail}"


def for_op(op):
    """The shapes `op` ("fwd", "data" or "filt") takes, as pytest params in table order.  The first seven keep
    the ids they had as a plain list (shape0 .. shape6); the rest are named by their shape."""
    import pytest
    return [pytest.param(t.shape, id=f"shape{i}" if i < len(SHAPES) else shape_id(t.shape))
            for i, t in enumerate(TRAIN) if getattr(t, op)]


def infer_params():
    """Every infer case as a pytest param: case0 .. case6 as before, the rest named by their shape."""
    import pytest
    return [pytest.param(c.case, id=f"case{i}" if i < len(INFER_CASES) else shape_id(c.case))
            for i, c in enumerate(INFER)]


def instance(name):
    """The leading `name<...>` of a kernel query's answer (bytes or str); "" for a refusal."""
    name = name.decode() if isinstance(name, bytes) else name
    return name.split(" lds=")[0]


def fields(name):
    """{"lds": ..., "groups": ..., "splits": ..., "slice": ..., "pieces": ...} of a kernel query's answer."""
    name = name.decode() if isinstance(name, bytes) else name
    return {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", name)}


def train_args(s):
    """A training shape as the queries' (N, C, H, W, Co, KH, KW, stride, pad, dil, groups)."""
    N, C, H, W, Co, KH, KW, pad = s
    return (N, C, H, W, Co, KH, KW, 1, pad, 1, 1)


def infer_args(c):
    """An infer case as the bnsign queries' sixteen arguments."""
    N, C, H, W, Co, KH, KW, pad, pool, cons = c
    form, K2, pad2 = (1, 0, 0) if cons is None else (0,) + tuple(cons)
    return (N, C, H, W, Co, KH, KW, 1, pad, 1, 1, pool, form, K2, K2, pad2)


def query_train(lib, s):
    """The three training queries' full answers for a shape, as str."""
    a = train_args(s)
    return tuple(f(*a).decode() for f in (lib.bnn_conv2d_fwd_wide_kernel, lib.bnn_conv2d_bwd_data_wide_kernel,
                                          lib.bnn_conv2d_bwd_filter_wide_kernel))


def query_infer(lib, c):
    return lib.bnn_conv2d_fwd_wide_bnsign_kernel(*infer_args(c)).decode()


def tap_groups(s):
    """(grows, ngroup, taps of a full group) of the filter gradient's plan, from the shape alone."""
    KH, KW = s[5], s[6]
    grows = min(KH, max(1, 9 // KW))
    return grows, (KH + grows - 1) // grows, grows * KW
