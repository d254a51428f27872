"""Cases of the frozen first-layer conv's tests: (N, C, H, W, Co, KH, KW, pad, pool, consumer (K2, pad2) or None)."""
CASES = [
    (2, 3, 8, 8, 128, 3, 3, 1, 0, (3, 1)),       # the flagship in miniature; a position tile larger than the image
    (1, 3, 12, 11, 192, 3, 3, 1, 0, (3, 1)),     # odd OW; two position tiles with a tail; a half-full second channel tile
    (2, 3, 8, 8, 130, 3, 3, 1, 2, None),         # Co tail; int8 output; pooled
    (1, 3, 12, 12, 128, 5, 5, 2, 2, (3, 1)),     # 5x5 on RGB, Kt = 75; pooled to planes
    (3, 1, 10, 6, 256, 3, 3, 0, 2, (5, 2)),      # C = 1; pad 0; 4x2 pooled maps; two channel tiles; a 5x5 consumer
    (1, 4, 9, 9, 65, 3, 3, 2, 0, None),          # C = 4; pad = K - 1; the smallest Co
    (1, 3, 4, 150, 128, 3, 3, 1, 0, (3, 1)),     # a row longer than a position tile
    (1, 2, 6, 140, 128, 5, 5, 2, 2, (1, 0)),     # a long pooled row; Kt = 50; a 1x1 consumer
    # the instances <k-steps, pool> the eight above do not reach
    (1, 1, 7, 9, 96, 3, 3, 1, 0, None),          # <1,0>
    (2, 4, 6, 6, 128, 3, 3, 1, 2, (3, 1)),       # <3,2>
    (1, 2, 7, 6, 128, 5, 5, 2, 0, (3, 1)),       # <4,0>
    (1, 3, 6, 7, 66, 5, 5, 1, 0, None),          # <5,0>
]


def abi_shape(case):
    """The 16 arguments of the _ok / _kernel queries."""
    N, C, H, W, Co, KH, KW, pad, pool, cons = case
    K2, pad2 = cons or (0, 0)
    return (N, C, H, W, Co, KH, KW, 1, pad, 1, 1, pool, 0 if cons else 1, K2, K2, pad2)
