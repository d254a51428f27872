"""Event timing of the fused latent-update passes at the project's own weight shapes:
bnn_sgd_clamp_pack (momentum 0.9), bnn_adam_clamp_pack, the torch path the SGD pass replaces
(torch.optim.SGD(foreach) + clamp_ + sign_pack_fp4), and bnn_bop_pack three ways -- without a
flip counter, counting at a realistic flip ratio (about 1e-3) and with every weight flipping at every launch --
FP4 rows + FP4 transpose, alternating in one process.

    python tools/update_bench.py [--iters 30] [--warmup 3] [--qt-fmt fp4|fp4p] [--passes sgd,adam,torch,bop]

Per shape and pass: the median / min / max of the timed launches (HIP events, a synchronise after each), the
bytes the pass must move (fp32 streams + the packed operands) and the GB/s that is at the median.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "distributed-mnist-bnns_amd"))
from bnn_amd import _lib as L          # noqa: E402
from bnn_amd import functional as F    # noqa: E402

SHAPES = [(8192, 8192), (8192, 784), (3072, 784), (1536, 3072)]      # WideNet fc2/fc3, fc1; Net fc1, fc2
LR, MU, WD = 0.01, 0.9, 5e-4


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


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
    passes = [p[:3] for p in passes if p[3] in legs]
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
        out[name] = med
        print(f"  {name:32s} {med:9.4f} {ts[0]:9.4f} {ts[-1]:9.4f}   {nbytes / 1e6:9.1f} MB  "
              f"{nbytes / med / 1e6:8.1f} GB/s")
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
    ap.add_argument("--passes", default="sgd,adam,torch,bop", help="the legs to run, of sgd, adam, torch, bop")
    args = ap.parse_args()
    legs = set(args.passes.split(","))
    if not legs or legs - {"sgd", "adam", "torch", "bop"}:
        raise SystemExit("--passes: a comma-separated list of sgd, adam, torch, bop")
    print(f"{args.iters} timed launches per pass after {args.warmup} warm-up, the passes alternating, "
          f"HIP events; FP4 rows + {args.qt_fmt} transpose")
    print(f"  {'pass':32s} {'median ms':>9s} {'min':>9s} {'max':>9s}   {'must move':>12s}  at the median")
    ok = True
    for N, K in SHAPES:
        print(f"[{N} x {K}]")
        ok = bench_shape(N, K, args.iters, args.warmup, args.qt_fmt, legs) and ok
    if {"sgd", "adam"} <= legs:
        print("sgd pack median <= adam pack median at every shape:", ok)


if __name__ == "__main__":
    main()
