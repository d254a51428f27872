#!/usr/bin/env python3
"""Inference timing: the existing eval path against the frozen forward (bnn_amd.inference).

In one process, alternating per repeat:
  (a) eval    -- model.eval() under no_grad: fused_bn=True, org_protocol=False, FP4 backend, u8 input
                 (GEMM -> fp32 z -> bn_apply_pack per hidden layer, bn_fwd_eval + torch's fc4);
  (b) frozen  -- freeze(model)(u): BN-sign GEMM epilogues + the eval head;
  (c) frozen2 -- the frozen forward with every hidden layer in its two-pass form (GEMM + bn_apply_pack),
                 which separates the epilogue's share from the head's and the bookkeeping's.
Sizes: WideNet at batch 65,536; Net at 4,096 and 10,000 (``--only wide:65536`` picks one); ``--only
cnn:4096`` times the BinCNN the same way -- (a) model.eval() on the fp32 images, (b) FrozenCNN on the u8
pixels (conv epilogues: BN-sign-pool, BN-pool-Linear), (c) FrozenCNN with every layer as conv +
bnn_bn2d_fwd_eval (+ linear_nsmall).  Each leg is
warmed up, then timed with device events over ~``--seconds`` of work per repeat; the line printed is one
JSON object with the median ms per batch of every leg, every repeat's figure, the per-layer epilogue
bytes computed from the shapes, and labels_equal, the fraction of rows on which (a) and (b) agree.

A GPU is required.  For per-kernel times run it under ``rocprofv3 --kernel-trace --stats`` with
``--seconds 0.2 --repeats 1``.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "distributed-mnist-bnns_amd"))

SIZES = [("wide", 65536), ("mlp", 4096), ("mlp", 10000)]


def _time_leg(fn, seconds):
    """ms per call of fn over about ``seconds`` of device work (events around the whole run)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    n = max(3, int(seconds * 1e3 / max(e0.elapsed_time(e1), 1e-3)))
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n, n


def _time_legs(legs, seconds, repeats):
    outs = {k: f() for k, f in legs.items()}          # warm-up (packs the weight caches, allocates buffers)
    for f in legs.values():
        f()
    torch.cuda.synchronize()
    runs = {k: [] for k in legs}
    iters = {}
    for _ in range(repeats):
        for k, f in legs.items():
            ms, n = _time_leg(f, seconds)
            runs[k].append(round(ms, 4))
            iters[k] = n
    return outs, runs, iters


def _fill_stats(bns):
    """Running statistics of the scale the layers produce (timing does not depend on them; labels_equal does
    not either, both legs read the same ones)."""
    with torch.no_grad():
        for bn, fan_in in bns:
            bn.running_mean.normal_(0.0, 0.2 * fan_in ** 0.5)
            bn.running_var.uniform_(0.5 * fan_in, 1.5 * fan_in)


def _run_legs(model, fz, x_eval, u, seconds, repeats):
    """Times the three legs -- model.eval() on x_eval, fz on the u8 pixels u, fz in its two-pass form -- and
    returns their first outputs and the fields every size reports."""
    def leg_eval():
        with torch.no_grad():
            return model(x_eval)

    def leg_frozen():
        fz.two_pass = False
        return fz(u)

    def leg_frozen2():
        fz.two_pass = True
        out = fz(u)
        fz.two_pass = False
        return out

    outs, runs, iters = _time_legs({"eval": leg_eval, "frozen": leg_frozen, "frozen_two_pass": leg_frozen2},
                                   seconds, repeats)
    return outs, {"eval_ms": round(statistics.median(runs["eval"]), 4),
                  "frozen_ms": round(statistics.median(runs["frozen"]), 4),
                  "frozen_two_pass_ms": round(statistics.median(runs["frozen_two_pass"]), 4),
                  "runs_ms": runs, "iters_per_run": iters,
                  "labels_equal": float((outs["eval"].argmax(1) == outs["frozen"].argmax(1)).float().mean())}


def run_cnn(batch, seconds, repeats):
    from bnn_amd import freeze, nets
    from bnn_amd import functional as BF
    from bnn_amd.data import synthetic_mnist
    torch.manual_seed(0)
    model = nets.BinCNN(org_protocol=False, mutate_input=False, fused_bn=True).cuda().eval()
    _fill_stats(((model.layer1[1], 25 * 0.2), (model.layer2[1], 400)))
    u, _ = synthetic_mnist(batch, seed=5, device="cuda", as_u8=True)
    fz = freeze(model)
    outs, res = _run_legs(model, fz, BF.pixels_to_float(u), u, seconds, repeats)
    fz.two_pass = True
    h2 = fz.hidden_signs(u)
    fz.two_pass = False
    shp = fz._shapes()
    per = {}
    for i, (C, Co, KH, KW, pad, H, W, PH, PW) in enumerate(shp, 1):
        full, pooled = Co * 4 * PH * PW * 4, Co * PH * PW * 4
        # eval: conv writes fp32, bn2d reads it and writes the pooled fp32 map, the consumer reads that
        per[f"layer{i}"] = {"eval_bytes": int(batch * (2 * full + 2 * pooled)),
                            "frozen_bytes": int(batch * (2 * PH * PW * ((Co + 15) // 16 * 16) if i < len(shp) else 40))}
    return {"net": "cnn", "batch": batch, **res,
            "two_pass_labels_equal": float((outs["frozen_two_pass"].argmax(1) == outs["frozen"].argmax(1)).float().mean()),
            "two_pass_hidden_signs_identical": bool(torch.equal(fz.hidden_signs(u), h2)),
            "max_abs_diff_to_eval": float((outs["eval"] - outs["frozen"]).abs().max()),
            "intermediate_bytes": per}


def run_size(name, batch, seconds, repeats):
    if name == "cnn":
        return run_cnn(batch, seconds, repeats)
    from bnn_amd import freeze, nets
    from bnn_amd.data import synthetic_mnist
    torch.manual_seed(0)
    model = nets.MODELS[name](org_protocol=False, mutate_input=False, fused_bn=True).cuda().eval()
    _fill_stats(((model.bn1, 784 * 0.05), (model.bn2, model.fc2.in_features), (model.bn3, model.fc3.in_features)))
    u, _ = synthetic_mnist(batch, seed=5, device="cuda", as_u8=True)
    fz = freeze(model)
    outs, res = _run_legs(model, fz, u, u, seconds, repeats)
    h1, h2, h3 = fz.widths
    epi = {f"fc{i}": {"two_pass_bytes": int(batch * h * 8.5), "bnsign_bytes": int(batch * h * 0.5)}
           for i, h in ((1, h1), (2, h2))}
    return {"net": name, "widths": [h1, h2, h3], "batch": batch, **res,
            "two_pass_bit_identical": bool(torch.equal(outs["frozen"], outs["frozen_two_pass"])),
            "epilogue_bytes": epi}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seconds", type=float, default=1.0, help="device work per leg and repeat")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", action="append", default=None, metavar="NET:BATCH", help="e.g. wide:65536")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("infer_bench: needs a ROCm GPU")
    sizes = SIZES if not args.only else [(s.split(":")[0], int(s.split(":")[1])) for s in args.only]
    res = [run_size(n, b, args.seconds, args.repeats) for n, b in sizes]
    print(json.dumps({"bench": "infer", "device": torch.cuda.get_device_name(0), "seconds_per_leg": args.seconds,
                      "repeats": args.repeats, "sizes": res}))


if __name__ == "__main__":
    main()
