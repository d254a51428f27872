"""bench.py's command line: a plain run measures the headline figure only, --full adds the rest,
--dump-outputs writes the last timed step's results as float32 .npy files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

import bench


def _args(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_full_and_dump_outputs_are_off_by_default(monkeypatch):
    a = _args(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    a = _args(monkeypatch, "--full", "--dump-outputs", "somewhere")
    assert a.full is True and a.dump_outputs == "somewhere"


def test_dump_outputs_files_and_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 64)
    torch.manual_seed(3)
    model = torch.nn.Sequential(torch.nn.Linear(20, 10), torch.nn.BatchNorm1d(10), torch.nn.Linear(10, 4))
    out = model(torch.randn(8, 20))
    loss = out.square().mean()
    loss.backward()
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), model, loss, out.detach())
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert set(got) == ({"loss", "log_probs"} | {"param." + n for n, _ in model.named_parameters()}
                        | {"grad." + n for n, _ in model.named_parameters()}
                        | {"buffer." + n for n, _ in model.named_buffers()})
    assert all(v.dtype == np.float32 for v in got.values())
    assert got["loss"] == np.float32(loss.item())
    assert np.array_equal(got["log_probs"], out.detach().numpy())            # small: whole, in its shape
    assert np.array_equal(got["param.2.weight"], model[2].weight.detach().numpy())
    # 200 > 64 elements: a sample, the same elements for the parameter and its gradient's twin run
    w = model[0].weight.detach().numpy().reshape(-1)
    assert got["param.0.weight"].shape == (64,) and np.isin(got["param.0.weight"], w).all()
    for f in os.listdir(tmp_path / "a"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


@pytest.mark.gpu
def test_plain_run_line_and_dump(tmp_path):
    """One plain run of the published small configuration: the contract fields, none of --full's
    measurements, and the dump of the last of the 3 timed steps."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--config", "small", "--dump-outputs", str(tmp_path / "dump")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-2000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in r
    assert r["steps"] == 3 and r["ms_per_step"] > 0
    assert abs(r["value"] - 64 / (r["ms_per_step"] * 1e-3)) <= 1e-2 * r["value"]
    assert r["roofline"] is None and r["cpu_baseline"] is None
    assert not {"kernels", "dropin", "dropin_bn", "gpu_torch_fp32", "binary_gemm_tops"} & set(r)
    files = sorted(os.listdir(tmp_path / "dump"))
    assert "loss.npy" in files and "log_probs.npy" in files and "param.fc2.weight.npy" in files
    arrs = {f: np.load(tmp_path / "dump" / f) for f in files}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
    assert arrs["log_probs.npy"].shape == (64, 10)
    assert abs(float(arrs["loss.npy"]) - r["config"]["loss_last_step"]) <= 1e-5
    assert np.abs(arrs["param.fc2.weight.npy"]).max() <= 1.0                # latent weights stay clamped
