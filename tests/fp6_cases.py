"""The FP6 GEMM dispatch case table.

bnn_gemm_fp6_ws / bnn_gemm_fp6_panel_ws choose among the gemm_fp6_k / gemm_fp6_pers_k instances by
shape, residual plane and four process-global switches (bnn_gemm_fp6_set_variant, _set_persistent,
_set_half, _set_wide).  A case is a shape, `res` and one setting of the switches; its recorded answers
are the three label queries (bnn_gemm_fp6_kernel, _kernel_k, _kernel_kr) and bnn_gemm_fp6_workspace.

GRID is the full product of the shapes below, res and the switch values: 10 shapes x 2 x 90 settings
= 1800 cases.  The shapes: the wide step's dX and dW, two rounds and four rounds of tiles per CU, an
odd number of 64-row tile rows, an N that 1024 does not divide, split-K shapes, and the small shapes
of tests/test_gpu_fp6_wide_breg.py, where only the forced wide mode changes the answer.  VARIANTS adds
every variant id bnn_gemm_fp6_set_variant accepts (the timing-only diagnostic rows 91-98 and two
unknown ids included) at two shapes under the default switches, so every row of the instance table is
reached.  SPLIT_WIDE is one more shape over the same product: a split-K shape that the 64 x 1024
tile divides, which the forced wide mode runs unsplit (workspace 0) while bnn_gemm_fp6_set_half is 1.

tests/golden/fp6_dispatch.json holds the answers of the last commit whose FP6 host code chose its
kernel with free-standing predicates and hand-typed names; the dispatch table that replaced them must
give the same ones (tests/test_fp6_dispatch.py).  `python tests/fp6_cases.py OUT.json` records the
answers of the library it loads: re-record only when a default or a label changes on purpose.

The answers depend on the device's compute-unit count (256 on the MI355X, and the library's fallback
where no device is present).
"""
import collections
import itertools
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fp6_dispatch.json")
CUS = 256

SHAPES = [  # (M, N, K)
    (8192, 4096, 1024),
    (16384, 4096, 1024),
    (8256, 4096, 512),
    (8192, 4608, 1024),
    (32768, 8192, 8192),
    (8192, 8192, 32768),
    (768, 1536, 4096),
    (128, 2048, 320),
    (128, 1536, 320),
    (64, 1024, 64),
]
RES = (0, 1)
VARIANT = (-1, 5, 14)
PERS = (0, 1)
HALF = (0, 1, 2, 3, 4)
WIDE = (0, 1, 2)

# every id of the variant list, and two it does not hold (the first entry answers for those)
VARIANT_IDS = tuple(range(0, 9)) + tuple(range(10, 19)) + tuple(range(91, 99)) + (9, 99)
VARIANT_SHAPES = (SHAPES[0], SHAPES[6])

Case = collections.namedtuple("Case", "M N K res variant pers half wide")
Answer = collections.namedtuple("Answer", "kernel kernel_k kernel_kr workspace")

GRID = [Case(M, N, K, res, v, p, h, w)
        for (M, N, K), res, v, p, h, w in itertools.product(SHAPES, RES, VARIANT, PERS, HALF, WIDE)]
VARIANTS = [Case(M, N, K, res, v, 0, 1, 1)
            for v, (M, N, K), res in itertools.product(VARIANT_IDS, VARIANT_SHAPES, RES) if v not in VARIANT]
SPLIT_WIDE = [Case(768, 2048, 4096, res, v, p, h, w)
              for res, v, p, h, w in itertools.product(RES, VARIANT, PERS, HALF, WIDE)]
CASES = GRID + VARIANTS + SPLIT_WIDE


def switches(L):
    """The four switches' current values (the variant has no query: -1, its default)."""
    return (-1, L.bnn_gemm_fp6_set_persistent(-1), L.bnn_gemm_fp6_set_half(-1, 0.0), L.bnn_gemm_fp6_set_wide(-1))


def set_switches(L, variant, pers, half, wide):
    assert L.bnn_gemm_fp6_set_variant(variant) == 0
    assert L.bnn_gemm_fp6_set_persistent(pers) == 0
    assert L.bnn_gemm_fp6_set_half(half, 0.0) == 0
    assert L.bnn_gemm_fp6_set_wide(wide) == 0


def query(L, c):
    """The three labels and the workspace bytes of a case, under the switches now set."""
    return Answer(L.bnn_gemm_fp6_kernel(c.M, c.N).decode(), L.bnn_gemm_fp6_kernel_k(c.M, c.N, c.K).decode(),
                  L.bnn_gemm_fp6_kernel_kr(c.M, c.N, c.K, c.res).decode(), L.bnn_gemm_fp6_workspace(c.M, c.N, c.K))


def answers(L, what=query):
    """what(L, case) for every case, each under its own switches (restored after)."""
    prev = switches(L)
    out = []
    try:
        for c in CASES:
            set_switches(L, c.variant, c.pers, c.half, c.wide)
            out.append(what(L, c))
    finally:
        set_switches(L, *prev)
    return out


def recorded():
    """case -> Answer of the golden file."""
    with open(GOLDEN) as f:
        g = json.load(f)
    assert g["cus"] == CUS
    labels = g["labels"]
    return {Case(*r[:8]): Answer(labels[r[8]], labels[r[9]], labels[r[10]], r[11]) for r in g["rows"]}


def record(L, path):
    got = answers(L)
    labels = sorted({s for a in got for s in a[:3]})
    at = {s: i for i, s in enumerate(labels)}
    rows = [list(c) + [at[a.kernel], at[a.kernel_k], at[a.kernel_kr], a.workspace] for c, a in zip(CASES, got)]
    with open(path, "w") as f:
        f.write('{"cus": %d,\n "columns": "M N K res variant pers half wide kernel kernel_k kernel_kr workspace",\n'
                ' "labels": %s,\n "rows": [\n' % (CUS, json.dumps(labels, indent=1)))
        f.write(",\n".join(json.dumps(r, separators=(",", ":")) for r in rows))
        f.write("\n]}\n")


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(GOLDEN), "..", "..", "distributed-mnist-bnns_amd"))
    from bnn_amd import _lib
    record(_lib.lib(), sys.argv[1])
