"""The evaluation metrics without a GPU: bnn_amd.metrics on CPU tensors (the plain-torch restatement of
the ranking rule in include/bnn.h) against tests/metrics_ref.py and the reference's accuracy formula,
Frozen*.evaluate on CPU tensors, the argument checks of bnn_eval_metrics and the trainer's new flags."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as tF

from metrics_ref import metrics_ref

NAN = float("nan")


def _reference_accuracy(output, target, topk):
    """utils.py:142-155, restated."""
    maxk = max(topk)
    batch_size = target.size(0)
    _, pred = output.float().topk(maxk, 1, True, True)
    pred = pred.t()
    correct = pred.eq(target.view(1, -1).expand_as(pred))
    return [correct[:k].reshape(-1).float().sum(0).mul_(100.0 / batch_size) for k in topk]


def test_accuracy_on_cpu_equals_the_reference_formula():
    from bnn_amd import metrics
    g = torch.Generator().manual_seed(11)
    z = torch.randn(64, 10, generator=g)
    y = torch.randint(0, 10, (64,), generator=g)
    assert all(len(torch.unique(r)) == 10 for r in z)          # no ties: torch.topk's order is determined
    got = metrics.accuracy(z, y, topk=(1, 5))
    ref = _reference_accuracy(z, y, (1, 5))
    assert len(got) == 2
    for a, b in zip(got, ref):
        assert a.dtype == torch.float32 and a.dim() == 0 and torch.equal(a, b)
    assert 0.0 < float(got[0]) <= float(got[1])
    with pytest.raises(ValueError, match="topk"):
        metrics.accuracy(z, y, topk=(1, 11))


# hand-built rows, C = 4: (row, label, the top column, the label's rank or None where it has none)
RULE_ROWS = [
    ([1.0, 3.0, 3.0, 0.0], 2, 1, 1),          # the true class ties with a lower column: that one ranks first
    ([1.0, 3.0, 3.0, 0.0], 1, 1, 0),          # ... and with a higher column: the true class ranks first
    ([5.0, NAN, 7.0, 1.0], 2, 1, 1),          # a NaN in another column ranks above everything
    ([5.0, 2.0, NAN, 9.0], 2, 2, 0),          # a NaN in the true column: top
    ([NAN, 1.0, NAN, 9.0], 2, 0, 1),          # two NaNs: the lower column first
    ([NAN, 1.0, NAN, 9.0], 3, 0, 2),          # ... and both above the largest number
    ([0.5, 2.0, 1.0, 0.0], -100, 1, None),    # label == ignore_index: counted nowhere, pred still given
    ([0.5, 2.0, 1.0, 0.0], 4, 1, None),       # label == C: in counts[0] only, the loss NaN
    ([0.0, -0.0, -1.0, -2.0], 1, 0, 1),       # -0 == +0: a tie
]


def test_hand_built_rows_follow_the_rule():
    from bnn_amd import metrics
    z = torch.tensor([r[0] for r in RULE_ROWS])
    y = torch.tensor([r[1] for r in RULE_ROWS])
    C = 4
    r = metrics.ranking(z, y)
    assert r["pred"].tolist() == [row[2] for row in RULE_ROWS]
    for i, row in enumerate(RULE_ROWS):
        if row[3] is not None:
            assert int(r["rank"][i]) == row[3], i
    for k in (1, 2, 4):
        ref = metrics_ref(z.numpy(), y.numpy(), k)
        assert ref["pred"].tolist() == [row[2] for row in RULE_ROWS]
        ranks = [row[3] for row in RULE_ROWS if row[3] is not None]
        assert ref["counts"][0] == len(RULE_ROWS) - 1                       # all but the ignored row
        assert ref["counts"][1] == sum(rk == 0 for rk in ranks)
        assert ref["counts"][2] == sum(rk < k for rk in ranks)
        assert ref["counts"][3:].sum() == len(ranks)                        # the label == C row has no cell
        m = metrics.Meter(C, k=k, device="cpu")
        pred = torch.empty(len(RULE_ROWS), dtype=torch.int32)
        m.update(z, y, pred=pred)
        assert m.acc.counts.tolist() == ref["counts"].tolist()
        assert pred.tolist() == ref["pred"].tolist()
        assert np.isnan(m.result()["loss"])                                  # NaN rows and the label == C row
    # one row at a time the finite terms are lse - z[y]
    one = metrics.Meter(C, k=1, device="cpu").update(z[:1], y[:1]).result()
    assert one["n"] == 1 and one["loss"] == pytest.approx(float(torch.logsumexp(z[0].double(), 0) - 3.0), rel=1e-12)
    assert one["confusion"][2, 1] == 1 and one["confusion"].sum() == 1 and one["prec1"] == 0.0


def _random_case(M, C, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(M, C, generator=g) * 3.0
    y = torch.randint(0, C, (M,), generator=g)
    z[1, :] = z[1, 0]                   # a row of ties
    z[M // 2, (int(y[M // 2]) + 1) % C] = z[M // 2, int(y[M // 2])]
    y[3] = -100
    return z, y


def test_meter_on_cpu_two_updates_equal_one():
    from bnn_amd import metrics
    z, y = _random_case(301, 10, 5)
    whole = metrics.Meter(10, k=3, device="cpu").update(z, y)
    parts = metrics.Meter(10, k=3, device="cpu").update(z[:120], y[:120]).update(z[120:], y[120:])
    ref = metrics_ref(z.numpy(), y.numpy(), 3)
    assert whole.acc.counts.tolist() == parts.acc.counts.tolist() == ref["counts"].tolist()
    a, b = whole.result(), parts.result()
    assert a["n"] == b["n"] == 300 and a["k"] == 3
    assert abs(a["loss"] - b["loss"]) <= 1e-12 * abs(a["loss"])
    assert abs(a["loss"] - ref["loss_sum"] / 300) <= 1e-12 * abs(a["loss"])
    assert torch.equal(a["confusion"], b["confusion"]) and int(a["confusion"].sum()) == 300
    assert a["prec1"] == 100.0 * int(ref["counts"][1]) / 300 and a["preck"] == 100.0 * int(ref["counts"][2]) / 300
    # reset zeroes in place; k is clipped to C; an empty meter reports NaN
    buf = parts.acc.buf
    parts.reset()
    assert parts.acc.buf is buf and int(buf.abs().sum()) == 0 and np.isnan(parts.result()["loss"])
    assert metrics.Meter(2, k=5, device="cpu").k == 2
    with pytest.raises(ValueError, match=r"\[M, 10\]"):
        whole.update(z[:, :4], y)


# ----------------------------------------------------------------------------- C ABI
@pytest.fixture(scope="module")
def L():
    from bnn_amd import _lib
    return _lib.lib()


def test_eval_metrics_ok_agrees_with_cross_entropy_ok(L):
    for C in range(1, 71):
        assert L.bnn_eval_metrics_ok(C) == L.bnn_cross_entropy_ok(C), C
    assert [C for C in range(1, 71) if L.bnn_eval_metrics_ok(C)] == [2, 10, 16, 32, 64]


def test_eval_metrics_rejects_bad_arguments_without_a_gpu(L):
    """Every call answers BNN_EINVAL before any launch (the fake addresses are never used)."""
    P = ctypes.c_void_p(16)
    M, C = 300, 10
    ws = L.bnn_eval_metrics_workspace(M)
    assert ws == 2 * 8 and L.bnn_eval_metrics_workspace(0) == 0 and L.bnn_eval_metrics_workspace(-3) == 0
    assert L.bnn_eval_metrics_workspace(65536) == 256 * 8

    def call(z=P, y=P, M=M, C=C, k=5, loss=P, counts=P, pred=None, work=P, wb=ws):
        return L.bnn_eval_metrics(z, y, M, C, k, -100, loss, counts, pred, work, wb, None)

    bad = [dict(z=None), dict(y=None), dict(loss=None), dict(counts=None), dict(work=None),      # null pointers, M > 0
           dict(C=3), dict(C=0), dict(C=128),                                                     # unsupported C
           dict(k=0), dict(k=-1), dict(k=11), dict(C=2, k=3),                                     # k < 1, k > C
           dict(wb=ws - 1), dict(wb=0), dict(M=65536, wb=255 * 8),                                # short workspace
           dict(M=-1)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert b"bnn_eval_metrics" in L.bnn_last_error(), kw
    # M == 0 returns 0 and touches nothing, whatever else is passed
    assert call(M=0) == 0
    assert call(M=0, z=None, y=None, loss=None, counts=None, work=None, wb=0, k=0, C=3) == 0


def test_functional_wrappers_refuse_cpu_tensors():
    from bnn_amd import functional as BF
    z, y = torch.zeros(4, 10), torch.zeros(4, dtype=torch.int64)
    assert not BF.eval_metrics_ok(z, y)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        BF.eval_metrics(z, y, 1, BF.MetricAccumulators(10, "cpu"))
    acc = BF.MetricAccumulators(4, "cpu")
    assert acc.loss_sum.dtype == torch.float64 and acc.counts.shape == (3 + 16,) and acc.counts.dtype == torch.int64
    acc.loss_sum += 1.5
    acc.counts[2] += 7
    s, c = acc.read()
    assert s == 1.5 and c[2] == 7 and int(c.sum()) == 7
    import bnn_amd
    assert bnn_amd.metrics.Meter is not None


# ----------------------------------------------------------------------------- frozen models
def _set_running_stats(bns, seed):
    g = torch.Generator().manual_seed(seed)
    for bn, scale in bns:
        n = bn.num_features
        bn.running_mean.copy_(torch.randn(n, generator=g) * 0.3 * scale)
        bn.running_var.copy_((torch.rand(n, generator=g) + 0.5) * scale * scale)
        with torch.no_grad():
            bn.weight.copy_(torch.rand(n, generator=g) + 0.5)
            bn.bias.copy_(torch.randn(n, generator=g) * 0.2)


def _pixels(n, seed=3):
    g = torch.Generator().manual_seed(seed)
    u = torch.randint(0, 256, (n, 1, 28, 28), generator=g)
    u = torch.where(torch.rand((n, 1, 28, 28), generator=g) < 0.8, torch.zeros_like(u), u).to(torch.uint8)
    return u, torch.randint(0, 10, (n,), generator=g)


def frozen_mlp(h=64, seed=0):
    from bnn_amd import freeze, nets
    torch.manual_seed(seed)
    m = nets.MLP(h, h, h, org_protocol=False, mutate_input=False)
    _set_running_stats(((m.bn1, 30.0), (m.bn2, 12.0), (m.bn3, 12.0)), seed + 1)
    return freeze(m.eval())


def frozen_cnn(seed=0):
    from bnn_amd import freeze, nets
    torch.manual_seed(seed)
    m = nets.BinCNN(org_protocol=False, mutate_input=False)
    _set_running_stats(((m.layer1[1], 3.0), (m.layer2[1], 14.0)), seed + 1)
    return freeze(m.eval())


def check_evaluate(fz, x, y, batch, k=5):
    """evaluate against accuracy(), nll_loss of forward and its own counts; returns the result."""
    n = x.shape[0]
    r = fz.evaluate(x, y, k=k, batch=batch)
    assert set(r) == {"n", "loss", "prec1", "preck", "k", "confusion"}
    assert r["n"] == n and r["k"] == k
    hits = round(fz.accuracy(x, y, batch=batch) * n)
    assert abs(r["prec1"] * n / 100 - fz.accuracy(x, y, batch=batch) * n) < 1e-9
    assert int(r["confusion"].diagonal().sum()) == hits
    ref = float(tF.nll_loss(fz.forward(x).double(), y.to(x.device)))
    assert abs(r["loss"] - ref) <= 1e-6, (r["loss"], ref)
    assert int(r["confusion"].sum()) == n and r["confusion"].shape == (10, 10)
    assert torch.equal(r["confusion"].sum(dim=1), torch.bincount(y.cpu(), minlength=10))
    assert r["prec1"] <= r["preck"] <= 100.0
    return r


def test_frozen_mlp_evaluate_on_cpu():
    x, y = _pixels(100)
    r = check_evaluate(frozen_mlp(64), x, y, batch=32)          # 32 + 32 + 32 + 4: the last batch is short
    assert r == r and 0 < r["loss"] < 50


def test_frozen_cnn_evaluate_on_cpu():
    x, y = _pixels(20, seed=5)
    check_evaluate(frozen_cnn(), x, y, batch=32)
    check_evaluate(frozen_cnn(), x, y, batch=8, k=3)


# ----------------------------------------------------------------------------- trainer
def test_trainer_parses_the_new_flags(capsys):
    from bnn_amd import trainer
    a = trainer.parse([])
    assert (a.eval_topk, a.eval_idx_images, a.eval_idx_labels, a.checkpoint_best, a.train_acc) == (0, None, None, None,
                                                                                                  False)
    a = trainer.parse(["--eval", "256", "--eval-topk", "5", "--eval-idx-images", "i.gz", "--eval-idx-labels", "l.gz",
                       "--checkpoint-best", "best.pt", "--train-acc"])
    assert (a.eval, a.eval_topk, a.eval_idx_images, a.eval_idx_labels, a.checkpoint_best, a.train_acc) == (
        256, 5, "i.gz", "l.gz", "best.pt", True)
    with pytest.raises(SystemExit, match="--checkpoint-best needs --eval"):
        trainer.parse(["--checkpoint-best", "best.pt"])
    for one in ("--eval-idx-images", "--eval-idx-labels"):
        with pytest.raises(SystemExit, match="go together"):
            trainer.parse(["--eval", "16", one, "f.gz"])
    with pytest.raises(SystemExit, match="needs --eval"):
        trainer.parse(["--eval-idx-images", "i.gz", "--eval-idx-labels", "l.gz"])
    with pytest.raises(SystemExit, match="needs --eval"):
        trainer.parse(["--eval-topk", "5"])
    with pytest.raises(SystemExit, match="1..10"):
        trainer.parse(["--eval", "16", "--eval-topk", "11"])


def test_checkpoint_prec1_reads_the_best_file(tmp_path):
    from bnn_amd import nets, trainer
    from bnn_amd.checkpoint import save_checkpoint
    m = nets.MLP(64, 64, 64, org_protocol=False, mutate_input=False)
    save_checkpoint(str(tmp_path / "best.pt"), m, None, 3, extra={"prec1": 12.5})
    save_checkpoint(str(tmp_path / "plain.pt"), m, None, 3)
    assert trainer.checkpoint_prec1(str(tmp_path / "best.pt")) == 12.5
    assert trainer.checkpoint_prec1(str(tmp_path / "plain.pt")) is None
