"""Event timing of the frozen wide-channel conv (bnn_conv2d_fwd_wide_bnsign) beside the chain
of launches the same layer takes without it, on the BinaryNet / VGG-style CIFAR layers at batch 256, all 3x3
with pad 1 and MaxPool2d(2, 2) where BinaryNet pools, in one process, the legs alternating.

    python tools/conv_wide_infer_bench.py [--iters 20] [--warmup 3] [--batch 256]

Per layer, from the layer's input to the next 3x3 / pad 1 layer's FP4 planes:

  fused          bnn_conv2d_fwd_wide_bnsign on planes and a weight packed beforehand (one launch)
  chain          bnn_conv2d_fwd_wide (input pack, weight pack, GEMM) -> bnn_bn2d_fwd_eval (Hardtanh, pool)
                 -> bnn_conv2d_wide_pack_x for the consumer
  chain, packed  the same with the conv's own input pack left out (bnn_conv2d_fwd_wide_set_stages(6)): inside
                 a stack that pack is the previous layer's last launch, so this is the chain's cost per layer

each as median / min / max over the timed launches, and whether the two forms wrote the same planes.  The
dispatch rule of FrozenConvStack is the last column: a layer class takes the fused path only if its slowest
fused call beats the fastest call of the packed chain.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "distributed-mnist-bnns_amd"))
from bnn_amd import _lib as L          # noqa: E402
from bnn_amd import inference          # noqa: E402

LAYERS = [(128, 128, 32, 2), (128, 256, 16, 0), (256, 256, 16, 2), (256, 512, 8, 0), (512, 512, 8, 2)]   # C, Co, H = W, pool
K, PAD, EPS = 3, 1, 1e-5


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
    x = torch.randn(N, C, H, H, device="cuda", generator=g)
    w = torch.randn(Co, C, K, K, device="cuda", generator=g)
    b = torch.randn(Co, device="cuda", generator=g)
    mean = torch.randn(Co, device="cuda", generator=g) * 4
    var = torch.rand(Co, device="cuda", generator=g) * 40 + 4
    gamma = torch.randn(Co, device="cuda", generator=g)
    beta = torch.randn(Co, device="cuda", generator=g)
    invstd = inference._invstd(var, EPS)
    PH = H // 2 if pool else H
    shape = (N, C, H, H, Co, K, K, 1, PAD, 1, 1)
    if not lib.bnn_conv2d_fwd_wide_bnsign_ok(*shape, pool, 0, K, K, PAD):
        raise SystemExit(f"bnn_conv2d_fwd_wide_bnsign_ok refuses {shape}")
    u8 = lambda n: torch.empty(int(n), dtype=torch.uint8, device="cuda")
    planes, wq = u8(lib.bnn_conv2d_wide_planes_bytes(N, C, H, H, K, K, PAD)), u8(lib.bnn_conv2d_wide_wq_bytes(C, Co, K, K))
    nxt = lib.bnn_conv2d_wide_planes_bytes(N, Co, PH, PH, K, K, PAD)
    out_fused, out_chain = u8(nxt).fill_(0xFF), u8(nxt).fill_(0xFF)
    ws = u8(lib.bnn_conv2d_fwd_wide_workspace(N, C, H, H, Co, K, K, PAD))
    z = torch.empty(N, Co, H, H, device="cuda")
    y = torch.empty(N, Co, PH, PH, device="cuda")
    bnws = u8(lib.bnn_bn2d_workspace(N, Co))
    L.call("bnn_conv2d_wide_pack_x", x, planes, N, C, H, H, K, K, PAD, L.stream())
    L.call("bnn_conv2d_wide_pack_w", w, wq, C, Co, K, K, L.stream())

    def fused():
        L.call("bnn_conv2d_fwd_wide_bnsign", planes, wq, b, mean, invstd, gamma, beta, out_fused, N, C, H, H, Co, K, K,
               PAD, pool, 0, K, K, PAD, L.stream())

    def chain(mask=7):
        lib.bnn_conv2d_fwd_wide_set_stages(mask)
        try:
            L.call("bnn_conv2d_fwd_wide", x, w, b, z, *shape, ws, ws.numel(), L.stream())
        finally:
            lib.bnn_conv2d_fwd_wide_set_stages(7)
        L.call("bnn_bn2d_fwd_eval", z, N, Co, H, H, gamma, beta, mean, var, EPS, y, 1, pool, bnws, L.stream())
        L.call("bnn_conv2d_wide_pack_x", y, out_chain, N, Co, PH, PH, K, K, PAD, L.stream())

    legs = [("fused", fused), ("chain", chain), ("chain, packed", lambda: chain(6))]
    times = {name: [] for name, _ in legs}
    for it in range(warmup + iters):
        for name, fn in legs:
            t = timed(fn)
            if it >= warmup:
                times[name].append(t)
    torch.cuda.synchronize()
    same = torch.equal(out_fused, out_chain)
    kernel = lib.bnn_conv2d_fwd_wide_bnsign_kernel(*shape, pool, 0, K, K, PAD).decode()
    print(f"[{C} -> {Co} at {H} x {H}, pool {pool}, batch {N}]  {kernel}  planes out {nxt / 1e6:.1f} MB  same bits: {same}")
    out = {}
    for name, _ in legs:
        med, lo, hi = out[name] = stats(times[name])
        print(f"  {name:16s} {med:10.4f} {lo:10.4f} {hi:10.4f}   ({len(times[name])} launches)")
    f, c = out["fused"], out["chain, packed"]
    wins = f[2] < c[1]
    print(f"  packed chain / fused = {c[0] / f[0]:.2f}x at the medians; slowest fused {f[2]:.4f} against the fastest "
          f"packed chain {c[1]:.4f}: {'fused' if wins else 'two-pass'}")
    return same, wins


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    args = ap.parse_args()
    print(f"{args.iters} timed launches per leg after {args.warmup} warm-up, the legs alternating, HIP events, "
          f"a synchronise after each; {torch.cuda.get_device_name(0)}")
    print(f"  {'leg':16s} {'median ms':>10s} {'min':>10s} {'max':>10s}")
    res = [bench_layer(args.batch, *layer, args.iters, args.warmup) for layer in LAYERS]
    print("same bits on every layer:", all(s for s, _ in res), "  fused wins on:", [l[:3] for l, (_, w) in zip(LAYERS, res) if w])


if __name__ == "__main__":
    main()
