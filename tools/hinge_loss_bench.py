"""Kernel times of the hinge criteria at M = 65536, C = 10 next to the cross-entropy kernels, by the
project's kernel timer (functional.KernelTimer: HIP events around each libbnn call), averaged over 200
criterion steps (logits -> d logits) after 50 warm-up ones.

    python tools/hinge_loss_bench.py [LOG]        # profiles/r08_hinge_timing.log is one run of it
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "distributed-mnist-bnns_amd"))
from bnn_amd import functional as F  # noqa: E402
from bnn_amd.nn import CrossEntropyLoss, HingeLoss, SqrtHingeLoss  # noqa: E402

M, C, WARM, IT = 65536, 10, 50, 200
out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None


def say(*a):
    s = " ".join(str(x) for x in a)
    print(s, flush=True)
    if out is not None:
        out.write(s + "\n")
        out.flush()


g = torch.Generator(device="cuda").manual_seed(1)
z = (torch.randn(M, C, generator=g, device="cuda") * 3.0).requires_grad_(True)
y = torch.randint(0, C, (M,), generator=g, device="cuda")
T = torch.where(y.unsqueeze(1) == torch.arange(C, device="cuda"), 1.0, -1.0)
ce, hl, sq = CrossEntropyLoss(), HingeLoss(), SqrtHingeLoss()
steps = {
    "log_softmax + libbnn cross-entropy": lambda: ce(torch.log_softmax(z, 1), y),
    "libbnn hinge (labels)": lambda: hl(z, y),
    "libbnn squared hinge (labels)": lambda: sq(z, y),
    "libbnn squared hinge (dense +-1)": lambda: sq(z, T),
}


def run(fn, n):
    for _ in range(n):
        z.grad = None
        fn().backward()


say(f"M={M} C={C} warmup={WARM} iterations={IT} device={torch.cuda.get_device_name(0)}")
for name, fn in steps.items():
    run(fn, WARM)
    torch.cuda.synchronize()
    t = F.KernelTimer()
    with F.timing(t):
        run(fn, IT)
    for k, d in sorted(t.summary().items()):
        say(f"kernel timer [{name}] {k}: {d['avg_ms'] * 1e3:.2f} us avg over {d['launches']} launches, "
            f"{d['avg_bytes'] / 1e6:.2f} MB algorithmic")
if out is not None:
    out.close()
