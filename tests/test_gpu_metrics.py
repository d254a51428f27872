"""The evaluation metrics on libbnn (bnn_eval_metrics; bnn_amd.functional.eval_metrics, bnn_amd.metrics,
Frozen*.evaluate, the trainer's --eval-topk / --eval-idx-* / --checkpoint-best / --train-acc).

* counts, predictions and confusion cells equal tests/metrics_ref.py (the rule of include/bnn.h restated
  pair by pair in numpy) exactly, over every row count at which the kernel changes path (1024: the
  one-workgroup kernel's row stride; 16384 / 16385: its bound and the first block + fold batch; 255 .. 257
  and 16641: around and off the 256-row block) and every supported class count, with planted ties, NaNs,
  an ignored row and an out-of-range label, the first and the last row among them;
* the loss: fl32(loss_sum / counts[0]) is within one fp32 ulp of functional.cross_entropy on the same rows
  -- both are double sums of the same fp32 row terms, and a double sum of at most 2^22 positive terms is
  within 2^-31 relative of exact in any order, so only the final rounding can differ -- and within 1e-6 of
  torch's float64 cross-entropy (the bar of tests/test_gpu_loss.py and tests/test_gpu_hinge.py);
* accumulation over calls, bit-identical repeats, graph capture.

The trainer's --graph run is compared with its eager twin, --device-step (the same device-counter dropout
seeds, no graph; tests/test_gpu_graph.py's pairing): a plain eager run draws its dropout masks from the
host generator, so its weights differ from a --graph run's by construction.
"""
import contextlib
import functools
import gzip
import io
import re
import struct

import numpy as np
import pytest
import torch

from metrics_ref import metrics_ref, n_above

pytestmark = pytest.mark.gpu

SHAPES = [(1, 10), (7, 10), (255, 10), (256, 10), (257, 10), (1023, 10), (1024, 10), (1025, 10), (16384, 10),
          (16385, 10), (16641, 10), (65536, 10), (1000, 2), (513, 16), (256, 32), (1000, 64)]

PLANTS = {"clean": ("tie_lower", "tie_higher", "ignored"),
          "nan": ("nan_other", "tie_lower", "nan_true", "ignored", "tie_higher", "two_nans"),
          "oob": ("label_C", "tie_lower", "ignored", "tie_higher", "label_neg")}


@pytest.fixture(scope="module")
def F():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from bnn_amd import functional
    return functional


def _ks(C):
    return sorted({min(k, C) for k in (1, 2, 5, C)})


@functools.lru_cache(maxsize=None)
def _case(M, C, variant):
    """(z, y) on the device: logits randn * 3 and labels, with PLANTS[variant] written to rows 0, M - 1, M / 2,
    M / 3, 2 M / 3, M / 5 in that order (as many as M has), and the numpy reference per k.  Made once per
    (shape, variant) and left unchanged.  A tie copies one of the row's own values, so every finite logit keeps
    the magnitude of randn * 3, at which the fp32 row arithmetic meets the 1e-6 bar on a single row too (a tie
    planted at 50 puts lse at 50.69, whose fp32 spacing alone is 3.8e-6: the one-row case then misses the bar,
    and so does the training criterion, by the same bits)."""
    g = torch.Generator().manual_seed(M * 131 + C)
    z = torch.randn(M, C, generator=g) * 3.0
    y = torch.randint(0, C, (M,), generator=g)
    rows = list(dict.fromkeys([0, M - 1, M // 2, M // 3, (2 * M) // 3, M // 5]))
    for i, plant in zip(rows, PLANTS[variant]):
        if plant == "tie_lower":                    # the true class ties with a lower column
            y[i] = C - 1
            z[i, 0] = z[i, C - 1]
        elif plant == "tie_higher":                 # ... with a higher column
            y[i] = 0
            z[i, C - 1] = z[i, 0]
        elif plant == "ignored":
            y[i] = -100
        elif plant == "nan_other":
            y[i] = 0
            z[i, C - 1] = float("nan")
        elif plant == "nan_true":
            y[i] = C - 1
            z[i, C - 1] = float("nan")
        elif plant == "two_nans":
            y[i] = C - 1
            z[i, 0] = z[i, C - 1] = float("nan")
        elif plant == "label_C":
            y[i] = C
        elif plant == "label_neg":
            y[i] = -1
    zn, yn = z.numpy(), y.numpy()
    refs = {k: metrics_ref(zn, yn, k) for k in _ks(C)}
    return z.cuda(), y.cuda(), refs


def _launch(F, z, y, k, acc=None, pred=None):
    acc = F.MetricAccumulators(z.shape[1], z.device) if acc is None else acc
    F.eval_metrics(z, y, k, acc, pred=pred)
    return acc


def _check_counts(F, M, C, variant):
    """Counts, predictions and the confusion block against the reference for every k; returns per k the
    (loss_sum, counts) read back."""
    z, y, refs = _case(M, C, variant)
    out = {}
    for k, ref in refs.items():
        pred = torch.full((M,), -7, dtype=torch.int32, device="cuda")
        acc = _launch(F, z, y, k, pred=pred)
        loss_sum, counts = acc.read()
        counts = counts.numpy()
        print(f"M={M} C={C} {variant} k={k}: counts[:3]={counts[:3].tolist()} ref={ref['counts'][:3].tolist()} "
              f"loss_sum={loss_sum!r} ref={ref['loss_sum']!r}")
        assert np.array_equal(counts, ref["counts"]), (k, counts[:3], ref["counts"][:3])
        assert np.array_equal(pred.cpu().numpy().astype(np.int64), ref["pred"]), k
        yn, pn = y.cpu().numpy(), ref["pred"]
        ok = (yn != -100) & (yn >= 0) & (yn < C)
        assert np.array_equal(counts[3:], np.bincount(yn[ok] * C + pn[ok], minlength=C * C)), k
        # without pred the same numbers
        l2, c2 = _launch(F, z, y, k).read()
        assert np.array_equal(c2.numpy(), counts) and (l2 == loss_sum or (l2 != l2 and loss_sum != loss_sum))
        out[k] = (loss_sum, counts)
    return out


@pytest.mark.parametrize("M,C", SHAPES)
def test_counts_and_loss_match_the_reference(F, M, C):
    z, y, refs = _case(M, C, "clean")
    got = _check_counts(F, M, C, "clean")
    ce = F.cross_entropy(z, y)                               # the training criterion on the same rows
    f64 = float(torch.nn.functional.cross_entropy(z.double(), y))
    for k, (loss_sum, counts) in got.items():
        n = int(counts[0])
        assert n == M - int((y == -100).sum()) and n > 0
        mean32 = np.float32(loss_sum / n)
        ulp = float(np.spacing(np.float32(abs(float(ce)))))
        print(f"M={M} C={C} k={k}: loss {loss_sum / n!r} fl32 {float(mean32)!r} cross_entropy {float(ce)!r} "
              f"f64 {f64!r} ulp {ulp!r}")
        assert abs(float(mean32) - float(ce)) <= ulp                          # check A
        assert abs(loss_sum / n - f64) <= 1e-6 * max(1.0, abs(f64))           # check B
        assert abs(loss_sum - refs[k]["loss_sum"]) <= 1e-6 * max(1.0, abs(refs[k]["loss_sum"]))
    assert len({v[0] for v in got.values()}) == 1            # k does not touch the loss: the same bits


@pytest.mark.parametrize("M,C", SHAPES)
def test_nan_rows_and_bad_labels_make_the_loss_nan_and_leave_the_counts_exact(F, M, C):
    for variant in ("nan", "oob"):
        for loss_sum, counts in _check_counts(F, M, C, variant).values():
            assert loss_sum != loss_sum, variant
            assert counts[0] > 0


def test_the_planted_rows_are_what_they_claim(F):
    """The cases plant what the docstring says (checked on the reference, no GPU work)."""
    z, y, refs = _case(1025, 10, "nan")
    zn, yn = z.cpu().numpy(), y.cpu().numpy()
    na = n_above(zn)
    assert np.isnan(zn[0, 9]) and refs[1]["pred"][0] == 9 and na[0, yn[0]] >= 1          # nan_other, first row
    row = zn[1024]                                                                        # tie_lower, last row
    assert yn[1024] == 9 and row[0] == row[9] and na[1024, 9] == (row > row[9]).sum() + 1
    zc, yc, refc = _case(1025, 10, "clean")
    row = zc[1024].cpu().numpy()                                                          # tie_higher
    assert int(yc[1024]) == 0 and row[0] == row[9] and n_above(row[None])[0, 0] == (row > row[0]).sum()
    assert int(yc[512]) == -100


def test_accumulation_over_two_calls(F):
    M, C, k = 16641, 10, 5
    z, y, refs = _case(M, C, "clean")
    one = _launch(F, z, y, k)
    h = M // 2                                               # 8320 + 8321 rows: two one-workgroup calls
    two = _launch(F, z[:h].contiguous(), y[:h].contiguous(), k)
    _launch(F, z[h:].contiguous(), y[h:].contiguous(), k, acc=two)
    (l1, c1), (l2, c2) = one.read(), two.read()
    print(f"one call {l1!r}, two calls {l2!r}, rel {abs(l1 - l2) / abs(l1)!r}")
    assert torch.equal(c1, c2) and np.array_equal(c1.numpy(), refs[k]["counts"])
    assert abs(l1 - l2) <= 2.0 ** -40 * abs(l1)
    # a call adds: a second pass over the same rows doubles every count
    _launch(F, z, y, k, acc=one)
    l3, c3 = one.read()
    assert torch.equal(c3, 2 * c1) and abs(l3 - 2 * l1) <= 2.0 ** -40 * abs(l3)


@pytest.mark.parametrize("M", [300, 16641])
def test_a_repeated_call_sequence_gives_the_same_bits(F, M):
    z, y, _ = _case(16641, 10, "clean")
    z, y = z[:M].contiguous(), y[:M].contiguous()
    bits = []
    for _ in range(3):
        acc = F.MetricAccumulators(10, "cuda")
        for _ in range(3):
            _launch(F, z, y, 5, acc=acc)
        bits.append(acc.buf.cpu())
    assert torch.equal(bits[0], bits[1]) and torch.equal(bits[0], bits[2])
    assert int(bits[0][1]) == 3 * int((y != -100).sum())


def test_capture_in_a_graph(F):
    z, y, _ = _case(16641, 10, "clean")
    z, y = z[:300].contiguous(), y[:300].contiguous()
    single = _launch(F, z, y, 5).read()
    eager = F.MetricAccumulators(10, "cuda")
    for _ in range(3):
        _launch(F, z, y, 5, acc=eager)
    acc = F.MetricAccumulators(10, "cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _launch(F, z, y, 5, acc=acc)                         # warm-up: the workspace exists before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    acc.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _launch(F, z, y, 5, acc=acc)
    torch.cuda.synchronize()
    assert int(acc.buf.abs().sum()) == 0                      # the capture itself ran nothing
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    (lg, cg), (le, ce) = acc.read(), eager.read()
    assert torch.equal(cg, 3 * single[1]) and torch.equal(cg, ce)
    assert np.float64(lg).tobytes() == np.float64(le).tobytes()


def test_wrapper_checks(F):
    z, y, _ = _case(257, 10, "clean")
    acc = F.MetricAccumulators(10, "cuda")
    assert F.eval_metrics_ok(z, y)
    assert not F.eval_metrics_ok(z[:, :7].contiguous(), y) and not F.eval_metrics_ok(z, y.int())
    assert not F.eval_metrics_ok(z, y[:-1]) and not F.eval_metrics_ok(z.double(), y)
    with pytest.raises(ValueError, match="eval_metrics needs"):
        F.eval_metrics(z[:, :7].contiguous(), y, 1, F.MetricAccumulators(7, "cuda"))
    with pytest.raises(ValueError, match="accumulators for C = 16"):
        F.eval_metrics(z, y, 1, F.MetricAccumulators(16, "cuda"))
    with pytest.raises(ValueError, match="pred must be"):
        F.eval_metrics(z, y, 1, acc, pred=torch.empty(257, dtype=torch.int64, device="cuda"))
    from bnn_amd._lib import BnnError
    for k in (0, 11):
        with pytest.raises(BnnError, match="bnn_eval_metrics"):
            F.eval_metrics(z, y, k, acc)
    F.eval_metrics(z[:0], y[:0], 1, acc)                      # M == 0: nothing
    assert int(acc.buf.abs().sum().item()) == 0
    # a strided view is made contiguous
    wide = torch.zeros(257, 20, device="cuda")
    wide[:, ::2] = z
    a, b = _launch(F, wide[:, ::2], y, 5).read(), _launch(F, z, y, 5).read()
    assert a[0] == b[0] and torch.equal(a[1], b[1])


@pytest.mark.parametrize("topk", [(1,), (1, 5), (1, 3, 5), (5, 2), (10,)])
def test_accuracy_on_the_device_equals_the_cpu_result(F, topk):
    from bnn_amd import metrics
    z, y, _ = _case(1025, 10, "nan")                          # ties and NaNs: the rule decides, on both paths
    got = metrics.accuracy(z, y, topk=topk)
    ref = metrics.accuracy(z.cpu(), y.cpu(), topk=topk)
    assert len(got) == len(topk)
    for a, b in zip(got, ref):
        assert a.is_cuda and a.dtype == torch.float32 and a.dim() == 0 and torch.equal(a.cpu(), b)
    # launches: one for the pair {1, k}, one more per further distinct k
    timer = F.KernelTimer()
    with F.timing(timer):
        metrics.accuracy(z, y, topk=topk)
    assert len(timer.records) == max(1, len(set(topk) - {1}))
    # a class count libbnn does not take runs the restatement on the device
    q, yq = z[:, :7].contiguous(), y.clamp(0, 6)
    for a, b in zip(metrics.accuracy(q, yq, (1, 3)), metrics.accuracy(q.cpu(), yq.cpu(), (1, 3))):
        assert a.is_cuda and torch.equal(a.cpu(), b)


def test_meter_on_the_device_matches_the_cpu_meter(F):
    from bnn_amd import metrics
    z, y, refs = _case(1025, 10, "clean")
    dev, cpu = metrics.Meter(10, k=5, device="cuda"), metrics.Meter(10, k=5, device="cpu")
    for lo, hi in ((0, 400), (400, 1025)):
        dev.update(z[lo:hi], y[lo:hi])
        cpu.update(z[lo:hi].cpu(), y[lo:hi].cpu())
    a, b = dev.result(), cpu.result()
    assert (a["n"], a["prec1"], a["preck"], a["k"]) == (b["n"], b["prec1"], b["preck"], b["k"])
    assert torch.equal(a["confusion"], b["confusion"]) and abs(a["loss"] - b["loss"]) <= 1e-6
    assert np.array_equal(dev.acc.counts.cpu().numpy(), refs[5]["counts"])
    with pytest.raises(ValueError, match="eval_metrics needs"):
        metrics.Meter(7, device="cuda").update(z[:, :7].contiguous(), y)     # no quiet torch path on the device


# ----------------------------------------------------------------------------- frozen models
def _check_frozen_on_both(fz, x, y, batch):
    from test_metrics import check_evaluate
    cpu = check_evaluate(fz, x, y, batch)
    fz.to("cuda")
    gpu = check_evaluate(fz, x.cuda(), y.cuda(), batch)
    assert (gpu["n"], gpu["k"], gpu["prec1"], gpu["preck"]) == (cpu["n"], cpu["k"], cpu["prec1"], cpu["preck"])
    assert torch.equal(gpu["confusion"], cpu["confusion"])
    print(f"loss gpu {gpu['loss']!r} cpu {cpu['loss']!r}")
    assert abs(gpu["loss"] - cpu["loss"]) <= 1e-6


def test_frozen_mlp_evaluate(F):
    from test_metrics import _pixels, frozen_mlp
    x, y = _pixels(300)
    _check_frozen_on_both(frozen_mlp(256), x, y, batch=128)


def test_frozen_cnn_evaluate(F):
    from test_metrics import _pixels, frozen_cnn
    x, y = _pixels(64, seed=5)
    _check_frozen_on_both(frozen_cnn(), x, y, batch=48)


# ----------------------------------------------------------------------------- trainer
RUN = ["--model", "small", "--epochs", "1", "--max-steps", "3", "--batch-size", "64", "--dataset-size", "512",
       "--eval", "256", "--eval-topk", "5", "--train-acc"]
EVAL_LINE = re.compile(r"^Eval 1 : loss (\d+\.\d{6}) prec@1 (\d+\.\d\d) prec@5 (\d+\.\d\d) on (\d+) samples$", re.M)
ACC_FIELD = re.compile(r"^Train Epoch: 1 \[.*\tLoss: \S+ \t Time: \S+\tAcc: (\d+\.\d\d)$", re.M)


def _train(argv):
    from bnn_amd import trainer
    torch.manual_seed(0)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        trainer.main(argv)
    torch.cuda.synchronize()
    return buf.getvalue()


def test_trainer_prints_the_metrics_and_keeps_the_best(F, tmp_path):
    best = str(tmp_path / "best.pt")
    out = _train(RUN + ["--checkpoint-best", best])
    assert len(re.findall(r"^Eval 1 : accuracy \d\.\d{4} on 256 held-out samples$", out, re.M)) == 1, out
    (loss, p1, p5, n), = EVAL_LINE.findall(out)
    assert n == "256" and 0.0 <= float(p1) <= float(p5) <= 100.0 and float(loss) > 0.0
    accs = ACC_FIELD.findall(out)
    assert len(accs) == 1 and 0.0 <= float(accs[0]) <= 100.0, out       # 3 steps, log interval 10: one line
    acc4 = float(re.search(r"accuracy (\d\.\d{4})", out).group(1))
    assert abs(float(p1) - 100.0 * acc4) <= 0.0051 + 0.0051               # the two lines' roundings
    blob = torch.load(best, map_location="cpu", weights_only=True)
    assert blob["epoch"] == 1 and abs(blob["extra"]["prec1"] - float(p1)) <= 0.0051
    # without the new flags the new text is absent
    plain = _train(RUN[:-3])
    assert "prec@" not in plain and "Acc:" not in plain and "Eval 1 : accuracy" in plain


def test_trainer_graph_run_counts_in_the_captured_step(F, tmp_path):
    """--graph against its eager twin: the same prec@1 values on both new lines (the captured step carries
    the meter launch: were it left out of the replays, batch 0's count would still agree, so the run logs
    every step)."""
    outs = [_train(RUN + ["--log-interval", "1", "--checkpoint-best", str(tmp_path / f"b{i}.pt"), mode])
            for i, mode in enumerate(("--graph", "--device-step"))]
    evals = [EVAL_LINE.findall(o) for o in outs]
    accs = [ACC_FIELD.findall(o) for o in outs]
    assert len(evals[0]) == 1 and evals[0] == evals[1], outs
    assert len(accs[0]) == 3 and accs[0] == accs[1], outs
    from bnn_amd import functional
    assert functional._DEVICE_STEP is None


def _write_idx(path, arr):
    arr = np.ascontiguousarray(arr, np.uint8)
    with gzip.open(path, "wb") as f:
        f.write(struct.pack(">BBBB", 0, 0, 8, arr.ndim) + struct.pack(">" + "I" * arr.ndim, *arr.shape))
        f.write(arr.tobytes())


def test_trainer_evaluates_on_idx_files(F, tmp_path):
    from bnn_amd.data import synthetic_mnist
    x, y = synthetic_mnist(128, seed=99, device="cpu", as_u8=True)
    img, lab = str(tmp_path / "t-images-idx3-ubyte.gz"), str(tmp_path / "t-labels-idx1-ubyte.gz")
    _write_idx(img, x.reshape(128, 28, 28).numpy())
    _write_idx(lab, y.numpy())
    out = _train(RUN + ["--eval-idx-images", img, "--eval-idx-labels", lab])       # --eval 256 > 128: clipped
    (loss, p1, p5, n), = EVAL_LINE.findall(out)
    assert n == "128" and "on 128 held-out samples" in out
