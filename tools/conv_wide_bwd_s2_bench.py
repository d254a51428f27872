"""Event timing of the stride-2 wide-channel binary conv input gradient (bnn_conv2d_bwd_data_wide_s2, DESIGN.md
§27) beside bnn_conv2d_bwd_data -- the generic kernel these shapes took before -- on the downsampling layers of
the ResNet-style binarized networks at batch 256, in one process, the passes alternating.

    python tools/conv_wide_bwd_s2_bench.py [--iters 20] [--warmup 3] [--batch 256] [--old-every 4]

Per layer: the median / min / max of the whole new call (both pack passes and the GEMM) and of the old call, then
the new call's three launches alone (bnn_conv2d_bwd_data_wide_s2_set_stages: the dy pack, the weight pack, the GEMM
on an already packed workspace), the useful TOP/s of the GEMM (2 N Co OH OW C KH KW over its median; the three
planes make the MFMA work three times that), the norm-wise relative difference of the two dX, barred at 1e-5, and
as a yardstick bnn_conv2d_bwd_data_wide at stride 1 with the same C, Co, H, W (four times the MACs).  The old
kernel is timed at every --old-every-th round only (it is slow): 5 launches at the defaults.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "distributed-mnist-bnns_amd"))
from bnn_amd import _lib as L          # noqa: E402

LAYERS = [(64, 128, 32, 3, 1), (128, 256, 32, 3, 1), (256, 512, 16, 3, 1), (128, 256, 32, 1, 0)]   # C, Co, H = W, K, pad
BAR = 1e-5


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


def bench_layer(N, C, Co, H, K, pad, iters, warmup, old_every):
    g = torch.Generator(device="cuda").manual_seed(C * 1000 + Co + H)
    OH = (H + 2 * pad - K) // 2 + 1
    OH1 = H + 2 * pad - K + 1
    dy = torch.randn(N, Co, OH, OH, device="cuda", generator=g)
    dy1 = torch.randn(N, Co, OH1, OH1, device="cuda", generator=g)
    w = torch.randn(Co, C, K, K, device="cuda", generator=g)
    shape, shape1 = (N, C, H, H, Co, K, K, 2, pad, 1, 1), (N, C, H, H, Co, K, K, 1, pad, 1, 1)
    lib = L.lib()
    if not lib.bnn_conv2d_bwd_data_wide_s2_ok(*shape) or not lib.bnn_conv2d_bwd_data_wide_ok(*shape1):
        raise SystemExit(f"bnn_conv2d_bwd_data_wide_s2_ok or the stride-1 query refuses {shape}")
    ws = torch.empty(lib.bnn_conv2d_bwd_data_wide_s2_workspace(N, C, H, H, Co, K, K, pad), dtype=torch.uint8, device="cuda")
    ws1 = torch.empty(lib.bnn_conv2d_bwd_data_wide_workspace(N, C, H, H, Co, K, K, pad), dtype=torch.uint8, device="cuda")
    dx_old, dx_new, dx1 = (torch.empty(N, C, H, H, device="cuda") for _ in range(3))

    def old():
        L.call("bnn_conv2d_bwd_data", dy, w, dx_old, *shape, L.stream())

    def new(mask=7):
        lib.bnn_conv2d_bwd_data_wide_s2_set_stages(mask)
        try:
            L.call("bnn_conv2d_bwd_data_wide_s2", dy, w, dx_new, *shape, ws, ws.numel(), L.stream())
        finally:
            lib.bnn_conv2d_bwd_data_wide_s2_set_stages(7)

    def wide1():
        L.call("bnn_conv2d_bwd_data_wide", dy1, w, dx1, *shape1, ws1, ws1.numel(), L.stream())

    passes = [("bnn_conv2d_bwd_data (old path)", old), ("bnn_conv2d_bwd_data_wide_s2 (whole)", new),
              ("  dy pack", lambda: new(1)), ("  weight pack", lambda: new(2)), ("  GEMM", lambda: new(4)),
              ("bnn_conv2d_bwd_data_wide at stride 1", wide1)]
    times = {name: [] for name, _ in passes}
    for it in range(warmup + iters):
        for name, fn in passes:
            if fn is old and it >= warmup and (it - warmup) % old_every:
                continue
            t = timed(fn)
            if it >= warmup:
                times[name].append(t)
    old()
    new()
    torch.cuda.synchronize()
    diff = float((dx_new.double() - dx_old.double()).norm() / dx_old.double().norm())
    macs = N * Co * OH * OH * C * K * K
    print(f"[dX of {C} -> {Co}, {K}x{K} stride 2 at {H} x {H}, batch {N}]  "
          f"{lib.bnn_conv2d_bwd_data_wide_s2_kernel(*shape).decode()}  workspace {ws.numel() / 1e6:.1f} MB  "
          f"|dx_new - dx_old| / |dx_old| = {diff:.2e}")
    out = {}
    for name, _ in passes:
        med, lo, hi = out[name] = stats(times[name])
        extra = f"   {2 * macs / med / 1e9:8.1f} useful TOP/s" if name.strip() == "GEMM" else ""
        print(f"  {name:38s} {med:10.4f} {lo:10.4f} {hi:10.4f}   ({len(times[name])} launches){extra}")
    o, n = out[passes[0][0]], out[passes[1][0]]
    print(f"  old / new = {o[0] / n[0]:.1f}x at the medians; the slowest new call against the fastest old call "
          f"{o[1] / n[2]:.1f}x")
    return diff < BAR and n[2] < o[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--old-every", type=int, default=4)
    args = ap.parse_args()
    print(f"{args.iters} timed launches per pass after {args.warmup} warm-up, the passes alternating, HIP events, "
          f"a synchronise after each; {torch.cuda.get_device_name(0)}")
    print(f"  {'pass':38s} {'median ms':>10s} {'min':>10s} {'max':>10s}")
    ok = True
    for C, Co, H, K, pad in LAYERS:
        ok = bench_layer(args.batch, C, Co, H, K, pad, args.iters, args.warmup, args.old_every) and ok
    print(f"dX within {BAR:g} of the old path, and every new call faster than every old call, on every layer:", ok)


if __name__ == "__main__":
    main()
