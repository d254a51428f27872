"""Event timing of the fused latent-update passes at the project's own weight shapes:
bnn_sgd_clamp_pack (momentum 0.9), bnn_adam_clamp_pack, the torch path the SGD pass replaces
(torch.optim.SGD(foreach) + clamp_ + sign_pack_fp4), and bnn_bop_pack three ways -- without a
flip counter, counting at a realistic flip ratio (about 1e-3) and with every weight flipping at every launch --
FP4 rows + FP4 transpose, alternating in one process.  Two more legs time the passes that do not re-pack:
``flat`` -- bnn_adam_clamp, bnn_sgd_clamp and bnn_bop over the same shapes as flat tensors and over a tensor of
BinCNN's conv2 weight's size -- and ``multi`` -- bnn_adam_clamp_multi and bnn_sgd_clamp_multi over 16 tensors
of the nets' bias and BatchNorm sizes.  These two go through the C ABI alone, so ``--against <another build's
libbnn.so>`` loads that build beside this one and times every flat / multi pass for both, launch by launch in
turn on the same tensors in one process (two processes do not compare: at 8192 x 8192 the medians of two
runs of one build differ by more than a run's own min-max range); each pass then gets a verdict, this
build's median against the other's min-max range.

    python tools/update_bench.py [--iters 30] [--warmup 3] [--qt-fmt fp4|fp4p] [--passes sgd,adam,torch,bop]
                                 (--passes also takes flat and multi) [--against path/to/other/libbnn.so]

Per shape and pass: the median / min / max of the timed launches (HIP events, a synchronise after each), the
bytes the pass must move (fp32 streams + the packed operands) and the GB/s that is at the median.
"""
import argparse
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "distributed-mnist-bnns_amd"))
from bnn_amd import _lib as L          # noqa: E402
from bnn_amd import functional as F    # noqa: E402

SHAPES = [(8192, 8192), (8192, 784), (3072, 784), (1536, 3072)]      # WideNet fc2/fc3, fc1; Net fc1, fc2
LR, MU, WD = 0.01, 0.9, 5e-4
FLAT_SIZES = [N * K for N, K in SHAPES] + [32 * 16 * 5 * 5]          # ... as flat tensors; BinCNN's conv2 weight
# Net's bn1..bn3 weight / bias and fc biases, WideNet's, the heads' bias, BinCNN's BatchNorm2d parameters
MULTI_SIZES = [3072, 3072, 3072, 1536, 1536, 1536, 768, 768, 768, 8192, 8192, 8192, 10, 16, 32, 32]


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


BUILDS = [("", L.call)]          # (tag, call) per library timed; --against puts the other build first


def against(path):
    """Load another build of libbnn beside this one, with the same signatures (the C ABI is the same)."""
    lib = ctypes.CDLL(path)
    for name, (res, args) in L.signatures().items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args

    def call(name, *args):
        rc = getattr(lib, name)(*args)
        if rc != 0:
            raise L.BnnError(f"{name} failed in {path} (code {rc}): {lib.bnn_last_error().decode()}")
    BUILDS[:] = [(" [other]", call), (" [this]", L.call)]


def run_builds(passes, iters, warmup):
    """run_passes over passes = [(name, fn(call), bytes)] for every build in BUILDS; with two builds, a verdict
    per pass: this build's median within or below the other's min-max range."""
    stats = run_passes([(name + tag, (lambda fn=fn, call=call: fn(call)), nbytes)
                        for name, fn, nbytes in passes for tag, call in BUILDS], iters, warmup, full=True)
    if len(BUILDS) == 2:
        for name, _, _ in passes:
            (_, lo, hi), (med, _, _) = stats[name + BUILDS[0][0]], stats[name + BUILDS[1][0]]
            print(f"  {name}: this build's median {med:.4f} against the other's range {lo:.4f}-{hi:.4f}: "
                  + ("within or below" if med <= hi else "SLOWER"))


def run_passes(passes, iters, warmup, full=False):
    """Time passes = [(name, fn, bytes it must move)] alternating, print a line each, return {name: median ms}
    (full: {name: (median, min, max)})."""
    times = {name: [] for name, _, _ in passes}
    for it in range(warmup + iters):
        for name, fn, _ in passes:                  # alternating: every pass sees the same machine state
            t = timed(fn)
            if it >= warmup:
                times[name].append(t)
    out = {}
    for name, _, nbytes in passes:
        ts = sorted(times[name])
        med = ts[len(ts) // 2]
        out[name] = (med, ts[0], ts[-1]) if full else med
        print(f"  {name:32s} {med:9.4f} {ts[0]:9.4f} {ts[-1]:9.4f}   {nbytes / 1e6:9.1f} MB  "
              f"{nbytes / med / 1e6:8.1f} GB/s")
    return out


def update_tensors(n, seed):
    """p, the gradient and two state tensors of n elements."""
    g0 = torch.Generator(device="cuda").manual_seed(seed)
    p = torch.empty(n, device="cuda").uniform_(-1.1, 1.1, generator=g0)
    return p, torch.randn(n, device="cuda", generator=g0) * 1e-2, torch.zeros_like(p), torch.zeros_like(p)


def bench_flat(n, iters, warmup):
    """The flat passes over n elements: Adam, SGD (momentum 0.9) and Bop without a flip counter."""
    pa, grad, m, v = update_tensors(n, n)
    ps, buf = pa.clone(), torch.zeros_like(pa)
    pb, mb = pa.sign() + (pa == 0).float(), torch.zeros_like(pa)
    step = [0]

    def adam(call):
        step[0] += 1
        call("bnn_adam_clamp", L.ptr(pa), L.ptr(grad), L.ptr(m), L.ptr(v), n, LR, 0.9, 0.999, 1e-8, step[0], 1.0, 1,
             L.stream())

    def sgd(call):
        call("bnn_sgd_clamp", L.ptr(ps), L.ptr(grad), L.ptr(buf), n, LR, MU, 1.0, WD, 0, 0, 1.0, 1, L.stream())

    def bop(call):
        call("bnn_bop", L.ptr(pb), L.ptr(grad), L.ptr(mb), n, 1e-4, 1e-8, 1.0, None, L.stream())

    run_builds([("bnn_adam_clamp", adam, 28 * n), ("bnn_sgd_clamp", sgd, 20 * n), ("bnn_bop flips=NULL", bop, 20 * n)],
               iters, warmup)


def bench_multi(iters, warmup):
    """One multi-tensor launch over MULTI_SIZES: Adam (per-launch bias corrections, step 3) and SGD (momentum
    0.9).  The host arrays are built once: the events time the entry and its launch, not their marshalling."""
    ts = [update_tensors(n, 7 + j) for j, n in enumerate(MULTI_SIZES)]
    sgd_items = [(t[0].clone(), t[1], torch.zeros_like(t[0])) for t in ts]       # p, g, buf: kept alive here
    k, total = len(ts), sum(MULTI_SIZES)
    clamp = [(ctypes.c_int32, [j % 2 for j in range(k)])]
    sgd_arrays = F._multi_arrays(sgd_items, 3, (ctypes.c_int32, [0] * k), *clamp)
    adam_arrays = F._multi_arrays(ts, 4, (ctypes.c_int64, [3] * k), *clamp)

    def adam(call):
        call("bnn_adam_clamp_multi", k, *adam_arrays, LR, 0.9, 0.999, 1e-8, None, None, 1.0, L.stream())

    def sgd(call):
        call("bnn_sgd_clamp_multi", k, *sgd_arrays, LR, MU, 1.0, WD, 0, 1.0, L.stream())

    run_builds([("bnn_adam_clamp_multi", adam, 28 * total), ("bnn_sgd_clamp_multi", sgd, 20 * total)], iters, warmup)


def bench_shape(N, K, iters, warmup, qt_fmt, legs):
    g0 = torch.Generator(device="cuda").manual_seed(N + K)
    p0 = torch.empty(N, K, device="cuda").uniform_(-1.1, 1.1, generator=g0)
    grad = torch.randn(N, K, device="cuda", generator=g0) * 1e-2
    q, qt = F.sign_pack_fp4(p0, want_qt=True, qt_fmt=qt_fmt)
    tail = (1, L.ptr(q), q.shape[1], L.ptr(qt), qt.shape[1], F._QT_CODE[qt_fmt], L.stream())
    packed = q.numel() + qt.numel()

    ps, buf = p0.clone(), torch.zeros_like(p0)
    pa, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    pt = torch.nn.Parameter(p0.clone())
    pt.grad = grad
    topt = torch.optim.SGD([pt], lr=LR, momentum=MU, weight_decay=WD, foreach=True)
    step = [0]

    def sgd():
        L.call("bnn_sgd_clamp_pack", L.ptr(ps), L.ptr(grad), L.ptr(buf), N, K, LR, MU, 1.0, WD, 0, 0, 1.0, 1, *tail)

    def adam():
        step[0] += 1
        L.call("bnn_adam_clamp_pack", L.ptr(pa), L.ptr(grad), L.ptr(m), L.ptr(v), N, K, LR, 0.9, 0.999, 1e-8, step[0],
               1.0, 1, *tail)

    def torch_path():
        topt.step()
        with torch.no_grad():
            pt.clamp_(-1, 1)
        F.sign_pack_fp4(pt.detach(), want_qt=True, qt_fmt=qt_fmt)

    # bytes each pass must move: fp32 streams per element (SGD: p, g, buf read, p, buf written; Adam: p, g, m, v
    # read, p, m, v written) + the packed rows and transpose written once; the torch path cannot move less
    # than the fused SGD pass does
    # Bop: w, g, m read, w, m written.  gamma = 1 makes the average the gradient itself, and the gradient
    # changes sign from launch to launch, so from its second launch on a leg flips exactly the weights with
    # |g| > threshold.  grad is N(0, 1e-2): 3.3e-2 is its 3.3 sigma, about 1e-3 of the weights; the all-flip
    # leg's gradient is +-1 with the weight's sign and threshold 0, so every weight flips at every launch.
    pb = [p0.sign() + (p0 == 0).float() for _ in range(3)]
    mb = [torch.zeros_like(p0) for _ in range(3)]
    flips = torch.zeros(2, dtype=torch.int64, device="cuda")
    gsmall, gflip = [grad, -grad], [pb[2].clone(), -pb[2]]
    nbop = [0, 0, 0]

    def bop(i, gs, thr, ctr):
        nbop[i] += 1
        L.call("bnn_bop_pack", L.ptr(pb[i]), L.ptr(gs[nbop[i] % 2]), L.ptr(mb[i]), N, K, 1.0, thr, 1.0, ctr, *tail)

    passes = [("bnn_sgd_clamp_pack", sgd, 20 * N * K + packed, "sgd"),
              ("bnn_adam_clamp_pack", adam, 28 * N * K + packed, "adam"),
              ("torch SGD+clamp_+sign_pack_fp4", torch_path, 20 * N * K + packed, "torch"),
              ("bnn_bop_pack flips=NULL", lambda: bop(0, gsmall, 3.3e-2, None), 20 * N * K + packed, "bop"),
              ("bnn_bop_pack flips ~1e-3", lambda: bop(1, gsmall, 3.3e-2, L.ptr(flips)), 20 * N * K + packed, "bop"),
              ("bnn_bop_pack every weight flips", lambda: bop(2, gflip, 0.0, L.ptr(flips[1:])), 20 * N * K + packed,
               "bop")]
    out = run_passes([p[:3] for p in passes if p[3] in legs], iters, warmup)
    if "bop" in legs:
        f = flips.tolist()
        print(f"  bop flip ratio per launch: {f[0] / (N * K * (warmup + iters)):.3e} (realistic leg), "
              f"{f[1] / (N * K * (warmup + iters)):.3f} (all-flip leg)")
    s, a = out.get("bnn_sgd_clamp_pack"), out.get("bnn_adam_clamp_pack")
    t, b = out.get("torch SGD+clamp_+sign_pack_fp4"), out.get("bnn_bop_pack flips ~1e-3")
    ratios = [f"sgd / adam = {s / a:.3f}" if s and a else "", f"torch path / sgd = {t / s:.2f}x" if t and s else "",
              f"bop / adam = {b / a:.3f}" if b and a else ""]
    print("  " + "   ".join(r for r in ratios if r) + "   (ratios of pass times, not of training steps)")
    return s <= a if s and a else True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--qt-fmt", default="fp4", choices=("fp4", "fp4p"))
    ap.add_argument("--passes", default="sgd,adam,torch,bop",
                    help="the legs to run, of sgd, adam, torch, bop (the fused passes) and flat, multi")
    ap.add_argument("--against", metavar="LIBBNN_SO", default=None,
                    help="another build of libbnn.so: the flat and multi legs time it beside this one")
    args = ap.parse_args()
    if args.against:
        against(args.against)
    legs = set(args.passes.split(","))
    if not legs or legs - {"sgd", "adam", "torch", "bop", "flat", "multi"}:
        raise SystemExit("--passes: a comma-separated list of sgd, adam, torch, bop, flat, multi")
    print(f"{args.iters} timed launches per pass after {args.warmup} warm-up, the passes alternating, "
          f"HIP events; FP4 rows + {args.qt_fmt} transpose")
    print(f"  {'pass':32s} {'median ms':>9s} {'min':>9s} {'max':>9s}   {'must move':>12s}  at the median")
    ok = True
    for N, K in SHAPES if legs & {"sgd", "adam", "torch", "bop"} else ():
        print(f"[{N} x {K}]")
        ok = bench_shape(N, K, args.iters, args.warmup, args.qt_fmt, legs) and ok
    for n in FLAT_SIZES if "flat" in legs else ():
        print(f"[flat, {n} elements]")
        bench_flat(n, args.iters, args.warmup)
    if "multi" in legs:
        print(f"[multi-tensor, {len(MULTI_SIZES)} tensors, {sum(MULTI_SIZES)} elements]")
        bench_multi(args.iters, args.warmup)
    if {"sgd", "adam"} <= legs:
        print("sgd pack median <= adam pack median at every shape:", ok)


if __name__ == "__main__":
    main()
