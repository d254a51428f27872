"""Event timing of the first-layer conv entries (bnn_conv2d_fwd_first / bnn_conv2d_bwd_filter_first)
beside bnn_conv2d_fwd / bnn_conv2d_bwd_filter(binarize_input = 0) -- the generic kernels this layer took before
-- on the 3 -> 128, 3x3, pad 1, 32 x 32 layer at batch 256, in one process, the passes alternating.

    python tools/conv_first_bench.py [--iters 20] [--warmup 3] [--batch 256] [--limit 300] [--log profiles/conv_first_bench.log]

Per pass the median / min / max, and beside them two plain passes over the big tensor in the same run: a fill of
y (the forward's 134 MB of stores) and a sum of dy (the filter gradient's one read).  Then the norm-wise relative
difference of the two paths' y, dw and db, barred at 1e-5, and the dispatch rule: a class takes the new path by
default only if its slowest new call beats the fastest old call.  The measuring step runs as a child process
under --limit seconds; its output is the log.
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "distributed-mnist-bnns_amd"))

C, CO, HW, K, PAD = 3, 128, 32, 3, 1
BAR = 1e-5


def measure(N, iters, warmup):
    import torch
    from bnn_amd import _lib as L

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e)

    g = torch.Generator(device="cuda").manual_seed(23)
    x = torch.randn(N, C, HW, HW, device="cuda", generator=g)
    w = torch.randn(CO, C, K, K, device="cuda", generator=g)
    b = torch.randn(CO, device="cuda", generator=g)
    dy = torch.randn(N, CO, HW, HW, device="cuda", generator=g)
    shape = (N, C, HW, HW, CO, K, K, 1, PAD, 1, 1)
    lib = L.lib()
    if not lib.bnn_conv2d_fwd_first_ok(*shape):
        raise SystemExit(f"bnn_conv2d_fwd_first_ok refuses {shape}")
    ws = torch.empty(lib.bnn_conv2d_bwd_filter_first_workspace(N, C, HW, HW, CO, K, K, PAD), dtype=torch.uint8, device="cuda")
    ws_old = torch.empty(lib.bnn_conv2d_bwd_filter_workspace(N, C, CO, K, K, 1), dtype=torch.uint8, device="cuda")
    y_old, y_new = (torch.empty(N, CO, HW, HW, device="cuda") for _ in range(2))
    dw_old, dw_new = (torch.empty(CO, C, K, K, device="cuda") for _ in range(2))
    db_old, db_new = (torch.empty(CO, device="cuda") for _ in range(2))
    passes = [
        ("bnn_conv2d_fwd (old path)", lambda: L.call("bnn_conv2d_fwd", x, 0, w, b, y_old, *shape, L.stream())),
        ("bnn_conv2d_fwd_first", lambda: L.call("bnn_conv2d_fwd_first", x, w, b, y_new, *shape, L.stream())),
        ("  plain fill of y", lambda: y_new.fill_(1.0)),
        ("bnn_conv2d_bwd_filter (old path)",
         lambda: L.call("bnn_conv2d_bwd_filter", dy, x, 0, dw_old, db_old, ws_old, *shape, L.stream())),
        ("bnn_conv2d_bwd_filter_first",
         lambda: L.call("bnn_conv2d_bwd_filter_first", dy, x, dw_new, db_new, *shape, ws, ws.numel(), L.stream())),
        ("  plain sum of dy", lambda: dy.sum()),
    ]
    times = {name: [] for name, _ in passes}
    for it in range(warmup + iters):
        for name, fn in passes:
            t = timed(fn)
            if it >= warmup:
                times[name].append(t)
    for _, fn in passes[:2] + passes[3:5]:
        fn()
    torch.cuda.synchronize()
    rel = lambda a, r: float((a.double() - r.double()).norm() / r.double().norm())
    diffs = (rel(y_new, y_old), rel(dw_new, dw_old), rel(db_new, db_old))
    print(f"{iters} timed launches per pass after {warmup} warm-up, the passes alternating, HIP events, a synchronise "
          f"after each; {torch.cuda.get_device_name(0)}")
    print(f"[{C} -> {CO}, {K}x{K}, pad {PAD}, {HW} x {HW}, batch {N}]  y and dy {y_new.numel() * 4 / 1e6:.1f} MB  "
          f"partials {ws.numel() / 1e6:.1f} MB")
    print(f"  {lib.bnn_conv2d_fwd_first_kernel(*shape).decode()}\n  {lib.bnn_conv2d_bwd_filter_first_kernel(*shape).decode()}")
    print(f"  {'pass':34s} {'median ms':>10s} {'min':>10s} {'max':>10s}")
    out = {}
    for name, _ in passes:
        ts = sorted(times[name])
        out[name] = (ts[len(ts) // 2], ts[0], ts[-1])
        print(f"  {name:34s} {out[name][0]:10.4f} {out[name][1]:10.4f} {out[name][2]:10.4f}   ({len(ts)} launches)")
    ok = max(diffs) < BAR
    print(f"  |new - old| / |old|: y {diffs[0]:.2e}  dw {diffs[1]:.2e}  db {diffs[2]:.2e}  (bar {BAR:g}: {ok})")
    for cls, o, n in (("forward", 0, 1), ("filter gradient", 3, 4)):
        o, n = out[passes[o][0]], out[passes[n][0]]
        wins = n[2] < o[1]
        ok = ok and wins
        print(f"  {cls}: old / new = {o[0] / n[0]:.1f}x at the medians; the slowest new call against the fastest old "
              f"call {o[1] / n[2]:.1f}x -> new path by default: {wins}")
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--limit", type=int, default=300, help="seconds the measuring step may take")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "conv_first_bench.log"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        sys.exit(0 if measure(args.batch, args.iters, args.warmup) else 1)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--iters", str(args.iters), "--warmup", str(args.warmup),
           "--batch", str(args.batch)]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.limit)
    except subprocess.TimeoutExpired as e:
        print(e.stdout or "")
        raise SystemExit(f"the measuring step did not end within {args.limit} s")
    print(r.stdout, end="")
    os.makedirs(os.path.dirname(args.log), exist_ok=True)
    with open(args.log, "w") as f:
        f.write(r.stdout)
    sys.exit(r.returncode)


if __name__ == "__main__":
    main()
