"""Event timing of the frozen first-layer conv (bnn_conv2d_fwd_first_bnsign) beside the chain of
launches the same layer takes without it, on the RGB layer of the BinaryNet / VGG-style CIFAR stacks (3 -> 128,
3x3, pad 1, 32x32, batch 256, no pool, consumer 3x3 pad 1), in one process, the legs alternating.

    python tools/conv_first_infer_bench.py [--iters 20] [--warmup 3] [--batch 256]

From the fp32 images to the next layer's FP4 planes:

  fused   bnn_conv2d_fwd_first_bnsign (one launch)
  chain   bnn_conv2d_fwd_first -> bnn_bn2d_fwd_eval (Hardtanh) -> bnn_conv2d_wide_pack_x

each as median / min / max over the timed launches, with the chain's three launches timed on their own as well,
and whether the two forms wrote the same planes (asserted).  The dispatch rule of FrozenConvStack is the last
line: the block takes the fused path only if its slowest fused call beats the fastest chained call.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "distributed-mnist-bnns_amd"))
from bnn_amd import _lib as L          # noqa: E402
from bnn_amd import inference          # noqa: E402

C, CO, HW, K, PAD, POOL, EPS = 3, 128, 32, 3, 1, 0, 1e-5


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    args = ap.parse_args()
    N, lib = args.batch, L.lib()
    g = torch.Generator(device="cuda").manual_seed(C * 1000 + CO + HW)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    x, w, b, mean, gamma, beta = rnd(N, C, HW, HW), rnd(CO, C, K, K), rnd(CO), rnd(CO), rnd(CO), rnd(CO)
    var = torch.rand(CO, device="cuda", generator=g) * 40 + 4
    invstd = inference._invstd(var, EPS)
    shape = (N, C, HW, HW, CO, K, K, 1, PAD, 1, 1)
    if not lib.bnn_conv2d_fwd_first_bnsign_ok(*shape, POOL, 0, K, K, PAD):
        raise SystemExit(f"bnn_conv2d_fwd_first_bnsign_ok refuses {shape}")
    u8 = lambda n: torch.empty(int(n), dtype=torch.uint8, device="cuda")
    nxt = lib.bnn_conv2d_wide_planes_bytes(N, CO, HW, HW, K, K, PAD)
    out_fused, out_chain = u8(nxt).fill_(0xFF), u8(nxt).fill_(0xFF)
    z, y = torch.empty(N, CO, HW, HW, device="cuda"), torch.empty(N, CO, HW, HW, device="cuda")
    bnws = u8(lib.bnn_bn2d_workspace(N, CO))

    def fused():
        L.call("bnn_conv2d_fwd_first_bnsign", x, w, b, mean, invstd, gamma, beta, out_fused, N, C, HW, HW, CO, K, K, PAD,
               POOL, 0, K, K, PAD, L.stream())

    conv = lambda: L.call("bnn_conv2d_fwd_first", x, w, b, z, *shape, L.stream())
    bn = lambda: L.call("bnn_bn2d_fwd_eval", z, N, CO, HW, HW, gamma, beta, mean, var, EPS, y, 1, POOL, bnws, L.stream())
    pack = lambda: L.call("bnn_conv2d_wide_pack_x", y, out_chain, N, CO, HW, HW, K, K, PAD, L.stream())

    def chain():
        conv(), bn(), pack()

    legs = [("fused", fused), ("chain", chain), ("  conv alone", conv), ("  bn alone", bn), ("  pack alone", pack)]
    times = {name: [] for name, _ in legs}
    for it in range(args.warmup + args.iters):
        for name, fn in legs:
            t = timed(fn)
            if it >= args.warmup:
                times[name].append(t)
    same = torch.equal(out_fused, out_chain)
    kernel = lib.bnn_conv2d_fwd_first_bnsign_kernel(*shape, POOL, 0, K, K, PAD).decode()
    print(f"{args.iters} timed launches per leg after {args.warmup} warm-up, the legs alternating, HIP events, a "
          f"synchronise after each; {torch.cuda.get_device_name(0)}")
    print(f"[{C} -> {CO} at {HW} x {HW}, pool {POOL}, batch {N}]  {kernel}  fp32 map {z.numel() * 4 / 1e6:.0f} MB, "
          f"planes out {nxt / 1e6:.1f} MB  same bits: {same}")
    print(f"  {'leg':16s} {'median ms':>10s} {'min':>10s} {'max':>10s}")
    out = {}
    for name, _ in legs:
        med, lo, hi = out[name] = stats(times[name])
        print(f"  {name:16s} {med:10.4f} {lo:10.4f} {hi:10.4f}   ({len(times[name])} launches)")
    f, c = out["fused"], out["chain"]
    print(f"  chain / fused = {c[0] / f[0]:.2f}x at the medians; slowest fused {f[2]:.4f} against the fastest chain "
          f"{c[1]:.4f}: {'fused' if f[2] < c[1] else 'two-pass'}")
    assert same, "the fused call and the chain wrote different planes"


if __name__ == "__main__":
    main()
