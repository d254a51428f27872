"""Event timing of the wide-channel binary conv filter gradient (bnn_conv2d_bwd_filter_wide)
beside bnn_conv2d_bwd_filter -- the generic kernel these shapes took before -- on the BinaryNet / VGG-style
CIFAR layers at batch 256, all 3x3 with pad 1, in one process, the passes alternating.

    python tools/conv_wide_bwd_filter_bench.py [--iters 20] [--warmup 3] [--batch 256] [--old-every 4]

Per layer: the median / min / max of the whole wide call (both packs, the GEMM and the reduce) and of the old
call, then the wide call's four launches alone (bnn_conv2d_bwd_filter_wide_set_stages: the dy pack, the x
pack, the GEMM on an already packed workspace, the reduce of already written partials), the useful TOP/s of
the GEMM (2 N OH OW Co C KH KW over its median; the three planes make the MFMA work three times that), the
bytes of fp32 partials the GEMM writes and the reduce reads, and the norm-wise relative difference of the two
dW, barred at 1e-5.  The old kernel is timed at every --old-every-th round only: 5 launches at the defaults.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "distributed-mnist-bnns_amd"))
from bnn_amd import _lib as L          # noqa: E402

LAYERS = [(128, 128, 32), (128, 256, 16), (256, 256, 16), (256, 512, 8), (512, 512, 8)]   # C, Co, H = W
K, PAD = 3, 1
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


def bench_layer(N, C, Co, H, iters, warmup, old_every):
    g = torch.Generator(device="cuda").manual_seed(C * 1000 + Co + H)
    dy = torch.randn(N, Co, H, H, device="cuda", generator=g)
    x = torch.randn(N, C, H, H, device="cuda", generator=g)
    shape = (N, C, H, H, Co, K, K, 1, PAD, 1, 1)
    if not L.lib().bnn_conv2d_bwd_filter_wide_ok(*shape):
        raise SystemExit(f"bnn_conv2d_bwd_filter_wide_ok refuses {shape}")
    ws = torch.empty(L.lib().bnn_conv2d_bwd_filter_wide_workspace(N, C, H, H, Co, K, K, PAD), dtype=torch.uint8, device="cuda")
    ws_old = torch.empty(L.lib().bnn_conv2d_bwd_filter_workspace(N, C, Co, K, K, 1), dtype=torch.uint8, device="cuda")
    dw_old, dw_new = (torch.empty(Co, C, K, K, device="cuda") for _ in range(2))
    db_old, db_new = (torch.empty(Co, device="cuda") for _ in range(2))

    def old():
        L.call("bnn_conv2d_bwd_filter", dy, x, 1, dw_old, db_old, ws_old, *shape, L.stream())

    def wide(mask=15):
        L.lib().bnn_conv2d_bwd_filter_wide_set_stages(mask)
        try:
            L.call("bnn_conv2d_bwd_filter_wide", dy, x, dw_new, db_new, *shape, ws, ws.numel(), L.stream())
        finally:
            L.lib().bnn_conv2d_bwd_filter_wide_set_stages(15)

    passes = [("bnn_conv2d_bwd_filter (old path)", old), ("bnn_conv2d_bwd_filter_wide (whole)", wide),
              ("  dy pack", lambda: wide(1)), ("  x pack", lambda: wide(2)), ("  GEMM", lambda: wide(4)),
              ("  reduce", lambda: wide(8))]
    times = {name: [] for name, _ in passes}
    for it in range(warmup + iters):
        for name, fn in passes:
            if fn is old and it >= warmup and (it - warmup) % old_every:
                continue
            t = timed(fn)
            if it >= warmup:
                times[name].append(t)
    old()
    wide()
    torch.cuda.synchronize()
    diff = float((dw_new.double() - dw_old.double()).norm() / dw_old.double().norm())
    dbdiff = float((db_new.double() - db_old.double()).norm() / db_old.double().norm())
    macs = N * C * H * H * Co * K * K
    name = L.lib().bnn_conv2d_bwd_filter_wide_kernel(*shape).decode()
    splits = int(name.split("splits=")[1].split()[0])
    part = splits * K * K * ((Co + 63) // 64 * 64) * C * 4
    print(f"[dW of {C} -> {Co} at {H} x {H}, batch {N}]  {name}  workspace {ws.numel() / 1e6:.1f} MB  "
          f"partials {part / 1e6:.1f} MB  |dw_wide - dw_old| / |dw_old| = {diff:.2e}  db: {dbdiff:.2e}")
    out = {}
    for name, _ in passes:
        med, lo, hi = out[name] = stats(times[name])
        extra = f"   {2 * macs / med / 1e9:8.1f} useful TOP/s" if name.strip() == "GEMM" else ""
        print(f"  {name:34s} {med:10.4f} {lo:10.4f} {hi:10.4f}   ({len(times[name])} launches){extra}")
    o, n = out[passes[0][0]], out[passes[1][0]]
    print(f"  old / wide = {o[0] / n[0]:.1f}x at the medians; the slowest wide call against the fastest old call "
          f"{o[1] / n[2]:.1f}x")
    return diff < BAR and dbdiff < BAR and n[2] < o[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--old-every", type=int, default=4)
    args = ap.parse_args()
    print(f"{args.iters} timed launches per pass after {args.warmup} warm-up, the passes alternating, HIP events, "
          f"a synchronise after each; {torch.cuda.get_device_name(0)}")
    print(f"  {'pass':34s} {'median ms':>10s} {'min':>10s} {'max':>10s}")
    ok = True
    for C, Co, H in LAYERS:
        ok = bench_layer(args.batch, C, Co, H, args.iters, args.warmup, args.old_every) and ok
    print(f"dW and db within {BAR:g} of the old path, and every wide call faster than every old call, on every layer:", ok)


if __name__ == "__main__":
    main()
