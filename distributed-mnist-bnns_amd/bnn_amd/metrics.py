"""Evaluation metrics: the reference's ``utils.accuracy`` (utils.py:142-155) and the running meter of a
test loop -- held-out loss, precision@1 / @k and the confusion matrix -- computed on the device.

CUDA fp32 outputs with a class count libbnn has go through ``functional.eval_metrics`` (bnn_eval_metrics:
one small launch per batch into device accumulators, no host synchronisation, capturable).  Everything
else -- CPU tensors above all -- runs ``ranking``, a plain-torch restatement of the same rule, which is
also what the tests check the kernel against:

    a ranks above b when a > b; a NaN ranks above every non-NaN; equal values, and two NaNs, rank by the
    lower column index first.  rank = the number of columns that rank above the label's column;
    the prediction is the top-ranked column.

This is torch's argmax / topk treatment of NaN with the tie rule made explicit (torch.topk leaves the
order of equal values open).
"""
import torch

from . import functional as BF

__all__ = ["accuracy", "Meter", "ranking"]


def ranking(z, y, ignore_index=-100):
    """The rule above on z [M, C] and int64 labels y [M], in plain torch: a dict of ``pred`` (int64 [M], the
    top-ranked column), ``rank`` (int64 [M], columns ranking above the label's; C where the label is outside
    [0, C)), ``counted`` (bool [M], y != ignore_index), ``in_range`` (bool [M]) and ``term`` (float64 [M],
    lse(z_i) - z_i[y_i] in double; NaN where the label is out of range)."""
    M, C = z.shape
    cols = torch.arange(C, device=z.device).view(1, C)
    nan = torch.isnan(z)
    # the top-ranked column: the first NaN of a row that has one, else the first maximum
    best = torch.where(nan.any(dim=1, keepdim=True), nan, z == z.masked_fill(nan, float("-inf")).amax(dim=1, keepdim=True))
    pred = torch.where(best, cols, C).amin(dim=1) if C > 0 else torch.zeros((M,), dtype=torch.int64, device=z.device)
    in_range = (y >= 0) & (y < C)
    yc = y.clamp(0, C - 1).view(M, 1)
    vy = z.gather(1, yc)
    vy_nan = torch.isnan(vy)
    col_above = (z > vy) | (nan & ~vy_nan)            # column j ranks above the label's by value
    lab_above = (vy > z) | (vy_nan & ~nan)            # the label's column ranks above column j by value
    rank = torch.where(cols < yc, ~lab_above, col_above).sum(dim=1)
    rank = torch.where(in_range, rank, torch.full_like(rank, C))
    zd = z.double()
    term = torch.logsumexp(zd, dim=1) - zd.gather(1, yc).squeeze(1)
    term = torch.where(in_range, term, torch.full_like(term, float("nan")))
    return {"pred": pred, "rank": rank, "counted": y != ignore_index, "in_range": in_range, "term": term}


def _accumulate_torch(acc, z, y, k, ignore_index=-100):
    """functional.eval_metrics restated on ``ranking`` (any device, any float dtype, any C); returns the
    ranking."""
    C = acc.C
    r = ranking(z, y, ignore_index)
    counted = r["counted"]
    hit = counted & r["in_range"]
    acc.loss_sum += r["term"][counted].sum()
    acc.counts[0] += counted.sum()
    acc.counts[1] += (hit & (r["rank"] == 0)).sum()
    acc.counts[2] += (hit & (r["rank"] < k)).sum()
    cells = (y[hit] * C + r["pred"][hit]).to(torch.int64)
    acc.counts[3:] += torch.bincount(cells, minlength=C * C)
    return r


def _on_libbnn(z, y):
    return torch.is_tensor(z) and z.is_cuda and BF.eval_metrics_ok(z, y)


def accuracy(output, target, topk=(1,)):
    """Computes the precision@k for the specified values of k: utils.accuracy's signature and return, a list
    of 0-dim fp32 tensors ``hits_k * (100.0 / batch)`` on output's device (no host synchronisation).  CUDA
    fp32 [M, C] outputs with a class count libbnn has take one bnn_eval_metrics launch for the pair {1, k}
    and one more per further distinct k; everything else runs the plain-torch ``ranking``.  Equal values
    rank by the lower column first (see the module doc); labels outside [0, C) are never hits."""
    topk = tuple(int(k) for k in topk)
    batch = target.size(0)
    C = output.shape[1]
    if not topk or min(topk) < 1 or max(topk) > C:
        raise ValueError(f"accuracy: topk {topk} must lie in 1..{C} (the class count)")
    target = target.reshape(-1)
    hits = {}
    if _on_libbnn(output, target):
        ks = sorted(set(topk) - {1}) or [1]
        accs = [BF.eval_metrics(output, target, k, BF.MetricAccumulators(C, output.device))
                for k in ks]
        hits[1] = accs[0].counts[1]
        for k, a in zip(ks, accs):
            hits[k] = a.counts[2]
    else:
        z = output.float()
        r = ranking(z, target.to(torch.int64))
        for k in set(topk):
            hits[k] = (r["in_range"] & (r["rank"] < k)).sum()
    return [hits[k].to(torch.float32).mul_(100.0 / batch) for k in topk]


class Meter:
    """A test loop's running metrics over batches: ``update(z, y)`` adds a batch of outputs z [M, C] (logits
    or log-probabilities) and int64 labels to accumulators on ``device`` without a host synchronisation --
    one bnn_eval_metrics launch for CUDA tensors (capturable; ``reset`` zeroes in place, so a captured
    update keeps counting into the same memory), the plain-torch ``ranking`` for CPU tensors -- and
    ``result()`` reads them once.  ``k`` is clipped to C."""

    def __init__(self, C, k=5, device="cuda", ignore_index=-100):
        self.C = int(C)
        self.k = max(1, min(int(k), self.C))
        self.ignore_index = int(ignore_index)
        self.acc = BF.MetricAccumulators(self.C, device)

    @property
    def device(self):
        return self.acc.buf.device

    def reset(self):
        self.acc.zero_()
        return self

    def update(self, z, y, pred=None):
        if z.dim() != 2 or z.shape[1] != self.C:
            raise ValueError(f"Meter: expects [M, {self.C}] outputs (got {tuple(z.shape)})")
        if z.device != self.device:
            raise RuntimeError(f"Meter on {self.device} got outputs on {z.device}")
        if z.is_cuda:
            # a missing kernel is an error here, not a slower path: eval_metrics raises for what it does not take
            BF.eval_metrics(z, y, self.k, self.acc, self.ignore_index, pred=pred)
        else:
            r = _accumulate_torch(self.acc, z, y, self.k, self.ignore_index)
            if pred is not None:
                pred.copy_(r["pred"])
        return self

    def result(self):
        """{"n", "loss", "prec1", "preck", "k", "confusion"}: the counted rows, their mean loss, precision@1
        and @k in percent (NaN for n = 0) and the int64 [C, C] confusion matrix (row = label, column =
        prediction; rows with a label outside [0, C) are in n only) -- one host read."""
        loss_sum, counts = self.acc.read()
        n = int(counts[0])
        nan = float("nan")
        return {"n": n, "loss": loss_sum / n if n else nan,
                "prec1": 100.0 * int(counts[1]) / n if n else nan,
                "preck": 100.0 * int(counts[2]) / n if n else nan,
                "k": self.k, "confusion": counts[3:].reshape(self.C, self.C).clone()}
