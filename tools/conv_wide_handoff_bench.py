"""Event timing of the wide-conv training hand-off beside the chain of launches the same
transition takes without it, on the five conv-to-conv transitions of the BinaryNet / VGG-style CIFAR stack at batch 256
(the consumers 128 -> 128 ... 512 -> 512, 3x3, pad 1; MaxPool2d(2, 2) where BinaryNet pools), in one process, the legs
alternating.

    python tools/conv_wide_handoff_bench.py [--iters 20] [--warmup 3] [--batch 256]

Per transition, from the producer conv's fp32 output z to the consumer conv's fp32 output, and the consumer's
filter gradient:

  forward fused   bnn_bn2d_fwd_train_planes -> bnn_conv2d_fwd_wide_planes
  forward chain   bnn_bn2d_fwd_train (Hardtanh, pool) -> bnn_conv2d_fwd_wide (input pack, weight pack, GEMM)
  filter fused    bnn_conv2d_bwd_filter_wide_planes on the planes the forward left
  filter chain    bnn_conv2d_bwd_filter_wide on the fp32 activation the chain's forward left

each as median / min / max over the timed calls, and whether the two forms gave the same bits (y; dw and db).
The dispatch rule is DESIGN.md §22's: a class takes the new path by default only if its slowest fused call beats
the chain's fastest call of this run.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "distributed-mnist-bnns_amd"))
from bnn_amd import _lib as L          # noqa: E402

LAYERS = [(128, 128, 32, 0), (128, 256, 32, 2), (256, 256, 16, 0), (256, 512, 16, 2), (512, 512, 8, 0)]   # C, Co, H = W of z, pool
K, PAD, EPS, MOM = 3, 1, 1e-5, 0.1


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def stats(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def bench_layer(N, C, Co, H, pool, iters, warmup):
    lib = L.lib()
    g = torch.Generator(device="cuda").manual_seed(C * 1000 + Co + H)
    z = torch.randn(N, C, H, H, device="cuda", generator=g) * 20
    w = torch.randn(Co, C, K, K, device="cuda", generator=g)
    b = torch.randn(Co, device="cuda", generator=g)
    gamma = torch.randn(C, device="cuda", generator=g)
    beta = torch.randn(C, device="cuda", generator=g)
    PH = H // 2 if pool else H
    dy = torch.randn(N, Co, PH, PH, device="cuda", generator=g)
    shape = (N, C, PH, PH, Co, K, K, 1, PAD, 1, 1)
    if not (lib.bnn_bn2d_fwd_train_planes_ok(N, C, H, H, pool, K, K, PAD) and lib.bnn_conv2d_fwd_wide_ok(*shape)
            and lib.bnn_conv2d_bwd_filter_wide_ok(*shape)):
        raise SystemExit(f"a query refuses {(N, C, H, H, pool)} -> {shape}")
    u8 = lambda n: torch.empty(int(n), dtype=torch.uint8, device="cuda")
    f32 = lambda *s: torch.empty(*s, device="cuda")
    planes = u8(lib.bnn_conv2d_wide_planes_bytes(N, C, PH, PH, K, K, PAD))
    a = f32(N, C, PH, PH)
    bnws, mean, invstd = u8(lib.bnn_bn2d_workspace(N, C)), f32(C), f32(C)
    ws_f, ws_c = u8(lib.bnn_conv2d_fwd_wide_planes_workspace(*shape[:7], PAD)), u8(lib.bnn_conv2d_fwd_wide_workspace(*shape[:7], PAD))
    ws_g = u8(lib.bnn_conv2d_bwd_filter_wide_workspace(*shape[:7], PAD))
    y = {k: f32(N, Co, PH, PH) for k in ("fused", "chain")}
    dw, db = {k: f32(Co, C, K, K) for k in y}, {k: f32(Co) for k in y}

    def fwd_fused():
        L.call("bnn_bn2d_fwd_train_planes", z, N, C, H, H, gamma, beta, None, None, MOM, EPS, mean, invstd, planes, pool,
               K, K, PAD, bnws, L.stream())
        L.call("bnn_conv2d_fwd_wide_planes", planes, w, b, y["fused"], *shape[:7], PAD, ws_f, ws_f.numel(), L.stream())

    def fwd_chain():
        L.call("bnn_bn2d_fwd_train", z, N, C, H, H, gamma, beta, None, None, MOM, EPS, mean, invstd, a, 1, pool, bnws,
               L.stream())
        L.call("bnn_conv2d_fwd_wide", a, w, b, y["chain"], *shape, ws_c, ws_c.numel(), L.stream())

    def filt_fused():
        L.call("bnn_conv2d_bwd_filter_wide_planes", dy, planes, dw["fused"], db["fused"], *shape, ws_g, ws_g.numel(), L.stream())

    def filt_chain():
        L.call("bnn_conv2d_bwd_filter_wide", dy, a, dw["chain"], db["chain"], *shape, ws_g, ws_g.numel(), L.stream())

    legs = [("forward fused", fwd_fused), ("forward chain", fwd_chain), ("filter fused", filt_fused), ("filter chain", filt_chain)]
    times = {name: [] for name, _ in legs}
    for it in range(warmup + iters):
        for name, fn in legs:
            t = timed(fn)
            if it >= warmup:
                times[name].append(t)
    torch.cuda.synchronize()
    same = all(torch.equal(t["fused"], t["chain"]) for t in (y, dw, db))
    print(f"[{C} -> {Co}, z {H} x {H}, pool {pool}, batch {N}]  planes {planes.numel() / 1e6:.1f} MB against "
          f"{a.numel() * 4 / 1e6:.1f} MB of fp32  same bits: {same}")
    out = {}
    for name, _ in legs:
        med, lo, hi = out[name] = stats(times[name])
        print(f"  {name:16s} {med:10.4f} {lo:10.4f} {hi:10.4f}   ({len(times[name])} calls)")
    wins = []
    for leg in ("forward", "filter"):
        f, c = out[leg + " fused"], out[leg + " chain"]
        wins.append(f[2] < c[1])
        print(f"  {leg}: chain / fused = {c[0] / f[0]:.2f}x at the medians; slowest fused {f[2]:.4f} against the fastest "
              f"chain {c[1]:.4f}: {'fused' if wins[-1] else 'chain'}")
    return same, wins


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    args = ap.parse_args()
    print(f"{args.iters} timed calls per leg after {args.warmup} warm-up, the legs alternating, HIP events, "
          f"a synchronise after each; {torch.cuda.get_device_name(0)}")
    print(f"  {'leg':16s} {'median ms':>10s} {'min':>10s} {'max':>10s}")
    res = [bench_layer(args.batch, *layer, args.iters, args.warmup) for layer in LAYERS]
    print("same bits on every transition:", all(s for s, _ in res),
          "  forward wins on:", [l[:3] for l, (_, w) in zip(LAYERS, res) if w[0]],
          "  filter wins on:", [l[:3] for l, (_, w) in zip(LAYERS, res) if w[1]])


if __name__ == "__main__":
    main()
