"""Event timing of the stochastic pack passes against their deterministic twins at [65536, 8192]."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "distributed-mnist-bnns_amd"))
from bnn_amd import _lib as L          # noqa: E402
from bnn_amd import functional as F    # noqa: E402

M, C = 65536, 8192
WARM, ITERS = 3, 40
g = torch.Generator(device="cuda").manual_seed(1)
z = torch.randint(-40, 41, (M, C), generator=g, device="cuda").float() + torch.randn(C, generator=g, device="cuda")
gam = torch.rand(C, generator=g, device="cuda") + 0.5
bet = torch.randn(C, generator=g, device="cuda") * 0.2
mean, invstd, lo = (torch.empty(C, device="cuda") for _ in range(3))
ws = torch.empty((L.lib().bnn_bn_workspace(M, C),), dtype=torch.uint8, device="cuda")
L.call("bnn_bn_fwd_train", L.ptr(z), M, C, L.ptr(gam), L.ptr(bet), None, None, -1.0, 1e-5, L.ptr(mean), L.ptr(invstd),
       L.ptr(lo), None, 1, L.ptr(ws), L.stream())
q = torch.empty((M, C // 2), dtype=torch.uint8, device="cuda")
qt = F._qt_buffer(C, M, "fp4p", "cuda")
h = torch.rand((M, C), generator=g, device="cuda") * 2.6 - 1.3
SEED = 0x123456789ABC


def apply_pack(stoch):
    nb = 4 * M * C + q.numel() + qt.numel()
    with F._timed("bn_apply_pack_stoch" if stoch else "bn_apply_pack", 0, nb):
        if stoch:
            L.call("bnn_bn_apply_pack_stoch", L.ptr(z), M, C, L.ptr(mean), L.ptr(invstd), L.ptr(lo), L.ptr(gam),
                   L.ptr(bet), 1, L.ptr(q), q.shape[1], L.ptr(qt), qt.shape[1], 2, SEED, 0, L.stream())
        else:
            L.call("bnn_bn_apply_pack", L.ptr(z), M, C, L.ptr(mean), L.ptr(invstd), L.ptr(lo), L.ptr(gam), L.ptr(bet),
                   1, L.ptr(q), q.shape[1], L.ptr(qt), qt.shape[1], 2, L.stream())


def torch_stoch(t):
    """The torch-op Binarize(t, 'stoch') this change replaces on CUDA tensors."""
    with F._timed("torch_ops_binarize_stoch", 0, 0):
        noise = torch.rand(t.size(), device=t.device, dtype=t.dtype) - 0.5
        prob = t.add_(1.0).div_(2.0).add_(noise).clamp_(0.0, 1.0)
        return prob.round().mul_(2.0).sub_(1.0)


def sign_f32(t):
    with F._timed("sign_f32_k", 0, 8 * t.numel()):
        return F.sign(t)


timer = F.KernelTimer()
for it in range(WARM + ITERS):
    if it == WARM:
        torch.cuda.synchronize()
        ctx = F.timing(timer)
        ctx.__enter__()
    apply_pack(False)
    apply_pack(True)
    F.sign_pack_fp4_writeback(h, want_qt=True)
    F.stoch_pack_fp4_writeback(h, SEED, want_qt=True)
    sign_f32(h)
    F.binarize_stochastic(h, SEED)
    torch_stoch(h.clone())
ctx.__exit__(None, None, None)
torch.cuda.synchronize()
per = {}
for name, s0, e0, ops, nb in timer.records:
    per.setdefault(name, ([], nb))[0].append(s0.elapsed_time(e0))
print(f"shape [{M}, {C}], {ITERS} timed launches each after {WARM} warm-up, the seven passes alternating, HIP events")
print(f"{'pass':28s} {'median ms':>10s} {'min':>8s} {'max':>8s}  GB/s at the median (algorithmic bytes)")
for name in ("bn_apply_pack", "bn_apply_pack_stoch", "sign_pack_fp4_out", "stoch_pack_fp4_out", "sign_f32_k",
             "stoch_f32_k", "torch_ops_binarize_stoch"):
    ts, nb = per[name]
    ts = sorted(ts)
    med = ts[len(ts) // 2]
    bw = f"{nb / med / 1e6:8.1f}" if nb else "       -"
    print(f"{name:28s} {med:10.4f} {ts[0]:8.4f} {ts[-1]:8.4f}  {bw}")
