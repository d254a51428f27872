"""CPU-side checks of Bop: the numpy restatement of bop_elem (tests/bop_ref.py) equals the same formula in
torch CPU fp32 ops bit for bit, the tie cases behave as the header states, the makers' flip share lies in
its band, the C entries are declared, bound and reject bad arguments before any launch, and LatentBop /
the trainer's flags and resume check know the optimizer."""
import ctypes
import os

import numpy as np
import pytest
import torch

import bop_ref as R
from conftest import ROOT

F32 = np.float32
SIZES = [1, 7, 37, 3700, 65536]


def _torch_step(w, g, m, gamma, threshold, gscale):
    """bop_elem in torch CPU fp32 ops, each rounded on its own."""
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    gi = g * f(gscale)
    m2 = m + f(gamma) * (gi - m)
    s = torch.where(w < 0, f(-1.0), f(1.0))
    flip = s * m2 > f(threshold)
    return torch.where(flip, -s, s), m2, int(flip.sum())


@pytest.mark.parametrize("gscale", R.GSCALES)
@pytest.mark.parametrize("gamma,threshold", [(R.GAMMA, R.THRESHOLD), (1e-4, 1e-8), (1.0, 0.0), (0.3, float("inf"))])
def test_restatement_equals_torch_ops_bit_for_bit(gamma, threshold, gscale):
    for n in SIZES:
        rng = np.random.default_rng(2000 + n)
        w = R.make_w0(n, rng)
        m = np.zeros(n, F32)
        tw, tm = torch.from_numpy(w.copy()), torch.from_numpy(m.copy())
        for s in range(4):
            g = R.make_grad(n, rng)
            w, m, flips = R.bop_step(w, g, m, gamma, threshold, gscale)
            tw, tm, tflips = _torch_step(tw, torch.from_numpy(g), tm, gamma, threshold, gscale)
            assert np.array_equal(w.view(np.uint32), tw.numpy().view(np.uint32)), (n, s)
            assert np.array_equal(m.view(np.uint32), tm.numpy().view(np.uint32)), (n, s)
            assert flips == tflips
            assert np.all(np.abs(w) == 1.0)
        if threshold == float("inf"):
            assert flips == 0


def test_zero_negative_zero_and_nan_count_as_plus_one():
    w = np.array([0.0, -0.0, np.nan, -np.nan, 0.3, -0.3, 1.0, -1.0], F32)
    g = np.zeros(8, F32)
    w2, m2, flips = R.bop_step(w, g, np.zeros(8, F32), 0.5, 0.0)
    assert w2.tolist() == [1.0, 1.0, 1.0, 1.0, 1.0, -1.0, 1.0, -1.0] and flips == 0 and not m2.any()
    # a NaN average does not flip, and stays NaN
    w2, m2, flips = R.bop_step(np.array([1.0, -1.0], F32), np.array([np.nan, np.nan], F32), np.zeros(2, F32), 0.5, 0.0)
    assert w2.tolist() == [1.0, -1.0] and flips == 0 and np.isnan(m2).all()


def test_tie_does_not_flip():
    rng = np.random.default_rng(11)
    for thr in (2.0 ** -7, 2.0 ** -20, 1.0):
        w, g, must, kw = R.make_tie(4096, rng, thr)
        w2, m2, flips = R.bop_step(w, g, np.zeros_like(w), **kw)
        assert np.all(np.abs(m2) >= F32(thr)) and (np.abs(m2) == F32(thr)).any()      # exact ties occurred
        s = np.where(w < 0, F32(-1), F32(1))
        assert np.array_equal(w2 != s, must) and flips == int(must.sum()) and 0 < flips < len(w)
        assert not (w2 != s)[np.abs(m2) == F32(thr)].any()


@pytest.mark.parametrize("gscale", R.GSCALES)
def test_makers_flip_share_on_the_second_step(gscale):
    rng = np.random.default_rng(3)
    n = 65536
    w, m = R.make_w0(n, rng), np.zeros(n, F32)
    w, m, _ = R.bop_step(w, R.make_grad(n, rng), m, R.GAMMA, R.THRESHOLD, gscale)
    _, _, flips = R.bop_step(w, R.make_grad(n, rng), m, R.GAMMA, R.THRESHOLD, gscale)
    assert 0.05 < flips / n < 0.5, flips / n


# ------------------------------------------------------------------ C ABI
def test_header_declares_the_entries_and_the_binding_has_them():
    from bnn_amd import _lib
    with open(os.path.join(ROOT, "include", "bnn.h")) as f:
        text = f.read()
    assert "int bnn_bop(float* w, const float* grad, float* m, int64_t n, float gamma, float threshold" in text
    assert "int bnn_bop_pack(float* w, const float* grad, float* m, int64_t N, int64_t K, float gamma" in text
    sigs = _lib.signatures()
    assert len(sigs["bnn_bop"][1]) == 9 and len(sigs["bnn_bop_pack"][1]) == 16
    for name in ("bnn_bop", "bnn_bop_pack"):
        args = sigs[name][1]
        assert [a for a in args if a is ctypes.c_float] == [ctypes.c_float] * 3
        flips = args[7 if name == "bnn_bop" else 8]
        assert isinstance(flips, _lib.Pointer) and torch.int64 in flips.dtypes and torch.float32 not in flips.dtypes
        assert hasattr(_lib.lib(), name)


@pytest.fixture(scope="module")
def L():
    from bnn_amd import _lib
    return _lib.lib()


PTR = ctypes.c_void_p(4096)        # never dereferenced: every call below fails its argument check


def _flat(L, w=PTR, g=PTR, m=PTR, n=8, gamma=0.5, thr=0.1, flips=None):
    return L.bnn_bop(w, g, m, n, gamma, thr, 1.0, flips, None)


def _pack(L, w=PTR, g=PTR, m=PTR, N=64, K=64, gamma=0.5, thr=0.1, fmt=0, q=PTR, ldq=64, qt=None, ldqt=0, qt_fmt=0):
    return L.bnn_bop_pack(w, g, m, N, K, gamma, thr, 1.0, None, fmt, q, ldq, qt, ldqt, qt_fmt, None)


def test_bop_entries_reject_bad_arguments_without_a_gpu(L):
    assert _flat(L, w=None) == -1 and b"bnn_bop" in L.bnn_last_error()
    assert _flat(L, g=None) == -1 and _flat(L, m=None) == -1 and _flat(L, n=-1) == -1
    assert _flat(L, w=None, g=None, m=None, n=0) == 0                  # nothing to do
    assert _pack(L, w=None) == -1 and _pack(L, g=None) == -1 and _pack(L, m=None) == -1
    for f in (_flat, _pack):
        for gamma in (0.0, -0.1, 1.5, float("nan")):
            assert f(L, gamma=gamma) == -1, gamma
        for thr in (-1e-9, float("nan"), float("-inf")):
            assert f(L, thr=thr) == -1, thr
    assert b"bnn_bop_pack" in L.bnn_last_error()
    # the pack entry's layout conditions (bnn_adam_clamp_pack's)
    assert _pack(L, K=100, ldq=100) == -1 and _pack(L, K=100, ldq=64) == -1
    assert _pack(L, fmt=1, K=256, ldq=64) == -1 and _pack(L, fmt=2) == -1
    assert _pack(L, q=None, qt=None) == -1
    assert _pack(L, q=None, qt=PTR, ldqt=100) == -1 and _pack(L, N=100, q=None, qt=PTR, ldqt=64) == -1
    assert _pack(L, N=0) == -1 and _pack(L, K=0) == -1


# ------------------------------------------------------------------ LatentBop (host side) and the trainer
@pytest.mark.parametrize("kw", [dict(gamma=0.0), dict(gamma=-0.1), dict(gamma=1.5), dict(gamma=float("nan")),
                                dict(threshold=-1e-9), dict(threshold=float("nan"))])
def test_latent_bop_rejects_bad_hyper_parameters(kw):
    from bnn_amd.optim import LatentBop
    with pytest.raises(ValueError, match="gamma|threshold"):
        LatentBop([torch.nn.Parameter(torch.zeros(3))], **kw)


def test_latent_bop_groups_and_state_dict():
    from bnn_amd.optim import LatentAdam, LatentBop
    ps = [torch.nn.Parameter(torch.zeros(4, 3)), torch.nn.Parameter(torch.zeros(4))]
    opt = LatentBop(ps, bop_params=ps[:1])
    assert isinstance(opt, LatentAdam)
    g = opt.state_dict()["param_groups"][0]
    assert (g["lr"], g["betas"], g["eps"], g["gamma"], g["threshold"]) == (1e-3, (0.9, 0.999), 1e-8, 1e-4, 1e-8)   # larq's
    opt = LatentBop([{"params": ps[:1], "gamma": 0.5}, {"params": ps[1:]}], gamma=0.01, threshold=0.25)
    assert [(g["gamma"], g["threshold"]) for g in opt.param_groups] == [(0.5, 0.25), (0.01, 0.25)]
    other = LatentBop(ps)
    other.load_state_dict(LatentBop(ps, gamma=0.125, threshold=0.5).state_dict())
    assert (other.param_groups[0]["gamma"], other.param_groups[0]["threshold"]) == (0.125, 0.5)
    assert opt.flip_counts() == {}
    with pytest.raises(ValueError, match="gamma"):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(2))], "gamma": 2.0})


def test_binary_weights_are_the_binarized_modules_weights():
    from bnn_amd import nets
    m = nets.MLP(64, 64, 64)
    bw, bp = nets.binary_weights(m), nets.binary_params(m)
    assert bw and all(p.dim() == 2 for p in bw)
    assert {id(p) for p in bw} == {id(p) for p in bp if p.dim() > 1}
    c = nets.BinCNN()
    assert [tuple(p.shape) for p in nets.binary_weights(c)] == [(16, 1, 5, 5), (32, 16, 5, 5)]


def test_trainer_flags_and_optimizer_kind(tmp_path):
    from bnn_amd import trainer
    from bnn_amd.optim import LatentBop
    a = trainer.parse(["--optimizer", "bop", "--bop-gamma", "1e-3", "--bop-threshold", "1e-6"])
    assert (a.optimizer, a.bop_gamma, a.bop_threshold) == ("bop", 1e-3, 1e-6)
    a = trainer.parse([])
    assert (a.optimizer, a.bop_gamma, a.bop_threshold) == ("adam", 1e-4, 1e-8)
    p = [torch.nn.Parameter(torch.zeros(2))]
    assert trainer.optimizer_kind(LatentBop(p, bop_params=p).state_dict()) == "bop"
    assert trainer.optimizer_kind(torch.optim.SGD(p, lr=0.1).state_dict()) == "sgd"
    assert trainer.optimizer_kind(torch.optim.Adam(p).state_dict()) == "adam"
    path = str(tmp_path / "ck.pt")
    torch.save({"format": "bnn_amd.checkpoint/1", "optimizer": LatentBop(p, bop_params=p).state_dict()}, path)
    with pytest.raises(SystemExit, match="bop.*adam"):
        trainer.check_resume_optimizer(path, "adam")
    trainer.check_resume_optimizer(path, "bop")
    torch.save({"format": "bnn_amd.checkpoint/1", "optimizer": torch.optim.Adam(p).state_dict()}, path)
    with pytest.raises(SystemExit, match="adam.*bop"):
        trainer.check_resume_optimizer(path, "bop")
