"""Event timing of the stride-2 wide-channel binary conv forward (bnn_conv2d_fwd_wide_s2) beside
bnn_conv2d_fwd at stride 2 -- the generic kernel these shapes took before -- and beside bnn_conv2d_fwd_wide at
stride 1 on the same input, a yardstick that computes four times the positions, on the downsampling layers of
the ResNet-style binarized networks at batch 256, in one process, the legs alternating.

    python tools/conv_wide_s2_bench.py [--iters 20] [--warmup 3] [--batch 256] [--old-every 4]

Per layer: the median / min / max of the whole new call (both pack passes and the GEMM), of its three launches
alone (bnn_conv2d_fwd_wide_s2_set_stages), of the old call and of the stride-1 yardstick; the useful TOP/s of
the new GEMM (2 N Co OH OW C KH KW over its median); the share of phase-grid cells it computes and does not
store, Hq Wq / (OH OW); and whether the new and the old entry wrote the same bits.  The old kernel is timed at
every --old-every-th round only (it is orders slower): 5 launches at the defaults.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "distributed-mnist-bnns_amd"))
from bnn_amd import _lib as L          # noqa: E402

LAYERS = [(3, 1, 64, 128, 32), (3, 1, 128, 256, 32), (3, 1, 256, 512, 16), (1, 0, 128, 256, 32)]   # K, pad, C, Co, H = W


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


def bench_layer(N, K, pad, C, Co, H, iters, warmup, old_every):
    lib = L.lib()
    g = torch.Generator(device="cuda").manual_seed(C * 1000 + Co + H + K)
    x = torch.randn(N, C, H, H, device="cuda", generator=g)
    w = torch.randn(Co, C, K, K, device="cuda", generator=g)
    b = torch.randn(Co, device="cuda", generator=g)
    shape, shape1 = (N, C, H, H, Co, K, K, 2, pad, 1, 1), (N, C, H, H, Co, K, K, 1, pad, 1, 1)
    if not lib.bnn_conv2d_fwd_wide_s2_ok(*shape) or not lib.bnn_conv2d_fwd_wide_ok(*shape1):
        raise SystemExit(f"refused: {shape}")
    O, O1 = (H + 2 * pad - K) // 2 + 1, H + 2 * pad - K + 1
    ws = torch.empty(lib.bnn_conv2d_fwd_wide_s2_workspace(N, C, H, H, Co, K, K, pad), dtype=torch.uint8, device="cuda")
    ws1 = torch.empty(lib.bnn_conv2d_fwd_wide_workspace(N, C, H, H, Co, K, K, pad), dtype=torch.uint8, device="cuda")
    y_old, y_new = (torch.empty(N, Co, O, O, device="cuda") for _ in range(2))
    y1 = torch.empty(N, Co, O1, O1, device="cuda")

    def old():
        L.call("bnn_conv2d_fwd", x, 1, w, b, y_old, *shape, L.stream())

    def new(mask=7):
        lib.bnn_conv2d_fwd_wide_s2_set_stages(mask)
        try:
            L.call("bnn_conv2d_fwd_wide_s2", x, w, b, y_new, *shape, ws, ws.numel(), L.stream())
        finally:
            lib.bnn_conv2d_fwd_wide_s2_set_stages(7)

    def stride1():
        L.call("bnn_conv2d_fwd_wide", x, w, b, y1, *shape1, ws1, ws1.numel(), L.stream())

    legs = [("bnn_conv2d_fwd, stride 2 (old path)", old), ("bnn_conv2d_fwd_wide_s2 (whole)", new),
            ("  input pack", lambda: new(1)), ("  weight pack", lambda: new(2)), ("  GEMM", lambda: new(4)),
            ("bnn_conv2d_fwd_wide, stride 1", stride1)]
    times = {name: [] for name, _ in legs}
    for it in range(warmup + iters):
        for name, fn in legs:
            if fn is old and it >= warmup and (it - warmup) % old_every:
                continue
            t = timed(fn)
            if it >= warmup:
                times[name].append(t)
    old()
    new()
    torch.cuda.synchronize()
    same = torch.equal(y_old, y_new)
    macs = N * Co * O * O * C * K * K
    Hq = (H + 2 * pad + 1) // 2
    print(f"[{K}x{K} pad {pad}, {C} -> {Co} at {H} x {H}, batch {N}]  "
          f"{lib.bnn_conv2d_fwd_wide_s2_kernel(*shape).decode()}  workspace {ws.numel() / 1e6:.1f} MB  "
          f"Hq Wq / (OH OW) = {Hq * Hq / (O * O):.3f}  same bits: {same}")
    out = {}
    for name, _ in legs:
        med, lo, hi = out[name] = stats(times[name])
        extra = f"   {2 * macs / med / 1e9:8.1f} useful TOP/s" if name.strip() == "GEMM" else ""
        print(f"  {name:38s} {med:10.4f} {lo:10.4f} {hi:10.4f}   ({len(times[name])} launches){extra}")
    o, n, s1 = out[legs[0][0]], out[legs[1][0]], out[legs[5][0]]
    print(f"  old / new = {o[0] / n[0]:.1f}x at the medians; the slowest new call against the fastest old call "
          f"{o[1] / n[2]:.1f}x; stride-1 yardstick / new = {s1[0] / n[0]:.2f}x at the medians")
    return same and n[2] < o[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--old-every", type=int, default=4)
    args = ap.parse_args()
    print(f"{args.iters} timed launches per leg after {args.warmup} warm-up, the legs alternating, HIP events, "
          f"a synchronise after each; {torch.cuda.get_device_name(0)}")
    print(f"  {'leg':38s} {'median ms':>10s} {'min':>10s} {'max':>10s}")
    ok = True
    for K, pad, C, Co, H in LAYERS:
        ok = bench_layer(args.batch, K, pad, C, Co, H, args.iters, args.warmup, args.old_every) and ok
    print("same bits, and every new call faster than every old call, on every layer:", ok)


if __name__ == "__main__":
    main()
