"""The evaluation metrics restated directly from the rule in include/bnn.h, in numpy float64 -- the
reference of tests/test_metrics.py and tests/test_gpu_metrics.py (independent of bnn_amd.metrics.ranking).

Order of values: a ranks above b when a > b; a NaN ranks above every non-NaN; equal values, and two NaNs,
rank by the lower column index first.  Every pair of columns of every row is compared, so the rule is
applied as it reads: column a ranks above column b iff above(a, b), or neither is above the other and
a < b.  The prediction is the column nothing ranks above, the rank of a label the number of columns that
rank above its column.
"""
import numpy as np


def n_above(z):
    """int64 [M, C]: per row and column b, the number of columns that rank above b."""
    z = np.asarray(z)
    M, C = z.shape
    a, b = z[:, :, None], z[:, None, :]                   # [i, a, b]
    nan_a, nan_b = np.isnan(a), np.isnan(b)
    with np.errstate(invalid="ignore"):
        above = (a > b) | (nan_a & ~nan_b)                # value a ranks above value b
        below = (b > a) | (nan_b & ~nan_a)
    lower = np.arange(C)[:, None] < np.arange(C)[None, :]  # a < b
    return (above | (~below & lower)).sum(axis=1).astype(np.int64)


def row_terms(z, y):
    """float64 [M]: lse(z_i) - z_i[y_i] in double (NaN where the label is outside [0, C) or the row holds a
    NaN)."""
    z = np.asarray(z, np.float64)
    y = np.asarray(y, np.int64)
    M, C = z.shape
    mx = z.max(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        lse = mx + np.log(np.exp(z - mx[:, None]).sum(axis=1))
    ok = (y >= 0) & (y < C)
    return np.where(ok, lse - z[np.arange(M), np.clip(y, 0, C - 1)], np.nan)


def metrics_ref(z, y, k, ignore_index=-100):
    """What one bnn_eval_metrics call adds to zeroed accumulators: {"counts" int64 [3 + C*C], "pred" int64
    [M], "terms" float64 [M] (every row's, counted or not), "counted" bool [M], "loss_sum" float64}."""
    z = np.asarray(z)
    y = np.asarray(y, np.int64)
    M, C = z.shape
    na = n_above(z)
    assert ((na == 0).sum(axis=1) == 1).all()              # the order is total: one top column per row
    pred = (na == 0).argmax(axis=1).astype(np.int64)
    counted = y != ignore_index
    ok = counted & (y >= 0) & (y < C)
    rank = na[np.arange(M), np.clip(y, 0, C - 1)]
    counts = np.zeros(3 + C * C, np.int64)
    counts[0] = counted.sum()
    counts[1] = (ok & (rank == 0)).sum()
    counts[2] = (ok & (rank < k)).sum()
    counts[3:] = np.bincount(y[ok] * C + pred[ok], minlength=C * C)
    terms = row_terms(z, y)
    return {"counts": counts, "pred": pred, "terms": terms, "counted": counted,
            "loss_sum": float(terms[counted].sum())}
