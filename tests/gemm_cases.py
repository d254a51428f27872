"""The int8 / FP4 GEMM dispatch case table.

The forward GEMM entries of bnn_gemm.hip choose among the gemm_i8_k / gemm_i8_v2_k / gemm_fp4_k /
gemm_fp4_h_k instances by digit family, shape and two process-global switches
(bnn_gemm_set_variant, bnn_gemm_i8_bnstats_set_tile).  A case is a family, a shape and one setting
of the switches; its recorded answers are the label query (bnn_gemm_i8_kernel), the two statistics
chunk queries (bnn_gemm_i8_bnstats_chunk, bnn_gemm_fp4_bnstats_chunk) and bnn_gemm_i8_bnstats_ok.

CASES is the full product, per family, of the shapes, the K values, the family's variants and the
tile values: 6 x 5 x (15 + 15 + 6 + 13) x 3 = 4410 cases.  The (M, N) put each grid threshold on
both sides: 512 and 480 tiles of 256 x 256 (the (1,1) and FP4 threshold is 512), 256 and 224 tiles
of 128 x 256 (the (3,1) threshold is 256), a ragged and a one-tile shape.  The K put K % 128 on
both sides, and the last one makes a row pitch of K bytes reach the 32-bit tile-offset limit
(K * 256 = 2^31: the int8 forms fall back to rows 0 / 10 / 20).  The variants are -1, every value
that reaches a row of the family (`family base + v`), and two that reach none: 50, and 92, which
lands on the ids from 100 on for (3,1) -- rows that only the decision function may choose.
A variant that reaches another family's row is not in the table: its answer changed on purpose
when the dispatch table replaced the free-standing choices (tests/test_gemm_dispatch.py has it).

tests/golden/gemm_dispatch.json holds the answers of the last commit whose int8 / FP4 host code
chose its kernel in five places with hand-typed names; the dispatch table that replaced them must
give the same ones (tests/test_gemm_dispatch.py).  `python tests/gemm_cases.py OUT.json` records
the answers of the library it loads: re-record only when a default or a label changes on purpose.
"""
import collections
import itertools
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_dispatch.json")

# family -> (a_digits, b_digits) of bnn_gemm_i8_kernel (0, 0: the FP4 form) and the id of its first row
FAMILIES = {"11": (1, 1), "31": (3, 1), "33": (3, 3), "fp4": (0, 0)}
BASE = {"11": 0, "31": 10, "33": 20, "fp4": 30}

SHAPES = [  # (M, N)
    (8192, 4096),
    (8192, 3840),
    (4096, 2048),
    (4096, 1792),
    (300, 200),
    (64, 64),
]
KS = (64, 128, 832, 1024, 1 << 23)
UNKNOWN = (50, 92)
VARIANTS = {
    "11": (-1,) + tuple(range(10)) + (77, 78) + UNKNOWN,
    "31": (-1,) + tuple(range(10)) + (87, 88) + UNKNOWN,
    "33": (-1, 0, 1, 2) + UNKNOWN,
    "fp4": (-1,) + tuple(range(10)) + UNKNOWN,
}
TILES = (0, 1, 2)

Case = collections.namedtuple("Case", "family M N K variant tile")
Answer = collections.namedtuple("Answer", "kernel i8_chunk fp4_chunk i8_ok")

CASES = [Case(f, M, N, K, v, t)
         for f in FAMILIES for (M, N), K, v, t in itertools.product(SHAPES, KS, VARIANTS[f], TILES)]


def switches(L):
    """The two switches' current values (the variant has no query: -1, its default)."""
    return (-1, L.bnn_gemm_i8_bnstats_set_tile(-1))


def set_switches(L, variant, tile):
    assert L.bnn_gemm_set_variant(variant) == 0
    assert L.bnn_gemm_i8_bnstats_set_tile(tile) == 0


def query(L, c):
    """The label, the two chunks and the statistics form's shape verdict of a case, under the
    switches now set."""
    a, b = FAMILIES[c.family]
    return Answer(L.bnn_gemm_i8_kernel(a, b, c.M, c.N, c.K).decode(), L.bnn_gemm_i8_bnstats_chunk(c.M, c.N),
                  L.bnn_gemm_fp4_bnstats_chunk(c.M, c.N, c.K), L.bnn_gemm_i8_bnstats_ok(c.M, c.N, c.K, c.K, c.K))


def answers(L, what=query):
    """what(L, case) for every case, each under its own switches (restored after)."""
    prev = switches(L)
    out = []
    try:
        for c in CASES:
            set_switches(L, c.variant, c.tile)
            out.append(what(L, c))
    finally:
        set_switches(L, *prev)
    return out


def recorded():
    """case -> Answer of the golden file."""
    with open(GOLDEN) as f:
        g = json.load(f)
    labels, families = g["labels"], g["families"]
    return {Case(families[r[0]], *r[1:6]): Answer(labels[r[6]], r[7], r[8], r[9]) for r in g["rows"]}


def record(L, path):
    got = answers(L)
    labels = sorted({a.kernel for a in got})
    at = {s: i for i, s in enumerate(labels)}
    families = list(FAMILIES)
    rows = [[families.index(c.family)] + list(c[1:]) + [at[a.kernel], a.i8_chunk, a.fp4_chunk, a.i8_ok]
            for c, a in zip(CASES, got)]
    with open(path, "w") as f:
        f.write('{"columns": "family M N K variant tile kernel i8_chunk fp4_chunk i8_ok",\n'
                ' "families": %s,\n "labels": %s,\n "rows": [\n' % (json.dumps(families), json.dumps(labels, indent=1)))
        f.write(",\n".join(json.dumps(r, separators=(",", ":")) for r in rows))
        f.write("\n]}\n")


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(GOLDEN), "..", "..", "distributed-mnist-bnns_amd"))
    from bnn_amd import _lib
    record(_lib.lib(), sys.argv[1])
