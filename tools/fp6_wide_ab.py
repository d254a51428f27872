"""Interleaved A/B of the FP6 weight-gradient GEMM's tile forms on the wide-MLP dW shape
(8192 x 8192 x 65536, B in panels, no residual plane; random data, one process): the default
128 x 512 tile with B staged through LDS against the 64 x 1024 tile with B loaded straight into
registers (bnn_gemm_fp6_set_wide) at several raster groups.  Every form's C is asserted
bit-identical to the default's before anything is timed.

    python tools/fp6_wide_ab.py "d w:0 w:4 w:8 w:16 w:32" [rounds] [reps] [MxNxK]

d = the default tile (bnn_gemm_fp6_set_wide 0), w:G = the 64 x 1024 tile at raster group G (0 = the
library's default group).  Reports median and minimum per form over the rounds.  Run it under a
timeout; a fault ends the process and with it every later form.
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "distributed-mnist-bnns_amd"))
import torch  # noqa: E402

from bnn_amd import _lib as L  # noqa: E402
from bnn_amd import functional as BF  # noqa: E402


def main():
    M, N, K = (int(v) for v in sys.argv[4].split("x")) if len(sys.argv) > 4 else (8192, 8192, 65536)
    cfgs = (sys.argv[1] if len(sys.argv) > 1 else "d w:0 w:4 w:8 w:16 w:32").split()
    rounds = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 5
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    torch.manual_seed(0)
    x = torch.randn(M, K, device="cuda")
    op = BF.quant6_rows(x)
    op.res = None
    del x
    w = torch.randint(-1, 2, (N, K), device="cuda").float()
    w4, _ = BF.sign_pack_fp4(w)
    del w
    panels = BF.fp4_panels(w4, N, K)
    C = torch.empty(M, N, device="cuda")
    prev = L.lib().bnn_gemm_fp6_set_wide(-1)

    def run(c):
        wide = c != "d"
        L.call("bnn_gemm_fp6_set_wide", 1 if wide else 0)
        L.call("bnn_gemm_fp6_set_wide_group", int(c.split(":")[1]) if wide else 0)
        BF.gemm_fp6(op, None, N, out=C, panels=panels, panel_ks=K // 64)

    try:
        run("d")
        torch.cuda.synchronize()
        ref = C.clone()
        for c in cfgs:
            run(c)
            torch.cuda.synchronize()
            assert torch.equal(C, ref), (c, float((C - ref).abs().max()))
            print(f"{c:5s} {L.lib().bnn_gemm_fp6_kernel_kr(M, N, K, 0).decode()} "
                  f"[{L.lib().bnn_gemm_fp6_instance(M, N, K, 0, 1).decode()}]: equal to the default", flush=True)
        times = {c: [] for c in cfgs}
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(rounds):
            for c in cfgs:
                run(c)
                s.record()
                for _ in range(reps):
                    run(c)
                e.record()
                torch.cuda.synchronize()
                times[c].append(s.elapsed_time(e) / reps)
        for c in cfgs:
            med, mn = statistics.median(times[c]), min(times[c])
            print(f"{M}x{N}x{K} {c:5s}: median {med:7.3f} ms  min {mn:7.3f}  {2.0 * M * N * K / med / 1e9:7.1f} TOPS alg", flush=True)
    finally:
        L.call("bnn_gemm_fp6_set_wide", prev)
        L.call("bnn_gemm_fp6_set_wide_group", 0)


if __name__ == "__main__":
    main()
