"""CPU-side checks of the fused latent SGD: the numpy restatement of sgd_elem (tests/sgd_ref.py) equals
torch.optim.SGD in fp32 on the CPU followed by clamp_(-1, 1) bit for bit, the three C entries reject bad
arguments before any launch, and LatentSGD / the trainer's flags behave as torch's SGD does."""
import ctypes

import numpy as np
import pytest
import torch

import sgd_ref as R

F32 = np.float32
SIZES = [1, 7, 37, 3700, 65536]
STEPS = 6


@pytest.mark.parametrize("foreach", [False, True])
@pytest.mark.parametrize("gscale", R.GSCALES)
@pytest.mark.parametrize("setting", R.SETTINGS)
def test_restatement_equals_torch_sgd_bit_for_bit(setting, gscale, foreach):
    mu, damp, wd, nest = setting
    lr = 0.05
    for n in SIZES:
        rng = np.random.default_rng(1000 + n)
        p0 = R.make_p0(n, rng)
        P = torch.nn.Parameter(torch.from_numpy(p0.copy()))
        opt = torch.optim.SGD([P], lr=lr, momentum=mu, dampening=damp, weight_decay=wd, nesterov=nest,
                              foreach=foreach)
        p, buf = p0.copy(), None
        for s in range(STEPS):
            g = R.make_grad(n, rng)
            # torch sees the scaled gradient: the kernel's first operation is the same fp32 product
            P.grad = torch.from_numpy((g * F32(gscale)).astype(F32))
            opt.step()
            with torch.no_grad():
                P.clamp_(-1, 1)
            p, buf = R.sgd_step(p, g, buf, lr, mu, damp, wd, nest, first=(s == 0), gscale=gscale, clamp=True)
            assert np.array_equal(p.view(np.uint32), P.detach().numpy().view(np.uint32)), (n, s)
            if mu != 0:
                tb = opt.state[P]["momentum_buffer"].numpy()
                assert np.array_equal(buf.view(np.uint32), tb.view(np.uint32)), (n, s)
            else:
                assert buf is None and "momentum_buffer" not in opt.state[P]
        assert np.abs(p).max() <= 1.0
        if n >= 3700:
            assert (np.abs(p) == 1.0).any()          # the clamp occurred


def test_restatement_fma_is_not_the_separately_rounded_form():
    """The form with every product rounded on its own is a different function: the reason sgd_elem is
    written with fmaf."""
    rng = np.random.default_rng(5)
    p, g = R.make_p0(65536, rng), R.make_grad(65536, rng)
    fused, _ = R.sgd_step(p, g, None, 0.05, clamp=False)
    split = (p - (F32(0.05) * g).astype(F32)).astype(F32)
    assert 0 < (fused != split).mean() < 0.5


# ------------------------------------------------------------------ C ABI: rejected before any launch
@pytest.fixture(scope="module")
def L():
    from bnn_amd import _lib
    return _lib.lib()


PTR = ctypes.c_void_p(4096)        # never dereferenced: every call below fails its argument check


def _flat(L, p=PTR, g=PTR, buf=PTR, n=8, lr=0.1, mu=0.9, omd=1.0, wd=0.0, nest=0, first=0):
    return L.bnn_sgd_clamp(p, g, buf, n, lr, mu, omd, wd, nest, first, 1.0, 1, None)


def _pack(L, p=PTR, g=PTR, buf=PTR, N=64, K=64, lr=0.1, mu=0.9, omd=1.0, wd=0.0, nest=0, fmt=0, q=PTR, ldq=64,
          qt=None, ldqt=0, qt_fmt=0):
    return L.bnn_sgd_clamp_pack(p, g, buf, N, K, lr, mu, omd, wd, nest, 0, 1.0, 1, fmt, q, ldq, qt, ldqt, qt_fmt, None)


def _multi(L, count, mu=0.9, omd=1.0, lr=0.1, wd=0.0, nest=0, null_buf=False, null_p=False):
    k = max(count, 1)
    ptrs = (ctypes.c_void_p * k)(*[4096] * k)
    nulls = (ctypes.c_void_p * k)(*[None] * k)
    n = (ctypes.c_int64 * k)(*[8] * k)
    flags = (ctypes.c_int32 * k)(*[0] * k)
    c = lambda a: ctypes.cast(a, ctypes.c_void_p)
    return L.bnn_sgd_clamp_multi(count, c(nulls if null_p else ptrs), c(ptrs), c(nulls if null_buf else ptrs), c(n),
                                 c(flags), c(flags), lr, mu, omd, wd, nest, 1.0, None)


def test_sgd_entries_reject_bad_arguments_without_a_gpu(L):
    # null pointers with n > 0
    assert _flat(L, p=None) == -1 and b"bnn_sgd_clamp" in L.bnn_last_error()
    assert _flat(L, g=None) == -1
    assert _flat(L, n=-1) == -1
    assert _pack(L, p=None) == -1 and _pack(L, g=None) == -1
    assert _multi(L, 2, null_p=True) == -1
    # buf == NULL with momentum != 0 (and allowed -- nothing to do at n == 0 -- with momentum == 0)
    assert _flat(L, buf=None) == -1
    assert _pack(L, buf=None) == -1
    assert _multi(L, 2, null_buf=True) == -1
    assert _flat(L, buf=None, mu=0.0, n=0) == 0
    # Nesterov with momentum <= 0 or omd != 1
    for f in (_flat, _pack):
        assert f(L, nest=1, mu=0.0, buf=None) == -1
        assert f(L, nest=1, mu=0.9, omd=0.9) == -1
    assert _multi(L, 2, nest=1, mu=0.0) == -1 and _multi(L, 2, nest=1, omd=0.5) == -1
    # negative lr, momentum, weight decay
    for f in (_flat, _pack):
        assert f(L, lr=-0.1) == -1 and f(L, mu=-0.5) == -1 and f(L, wd=-1e-3) == -1
    assert _multi(L, 2, lr=-0.1) == -1 and _multi(L, 2, mu=-0.5) == -1 and _multi(L, 2, wd=-1e-3) == -1
    # count > 16
    assert _multi(L, 17) == -1 and b"at most 16" in L.bnn_last_error()
    assert _multi(L, -1) == -1
    assert _multi(L, 0) == 0
    # the pack entry's ldq / ldqt conditions (bnn_adam_clamp_pack's)
    assert _pack(L, K=100, ldq=100) == -1                          # int8 rows: ldq a multiple of 64
    assert _pack(L, K=100, ldq=64) == -1                           # ... covering K
    assert _pack(L, fmt=1, K=256, ldq=64) == -1                    # FP4 rows: ldq a multiple of 128
    assert _pack(L, fmt=2) == -1
    assert _pack(L, q=None, qt=None) == -1                         # nothing to write
    assert _pack(L, q=None, qt=PTR, ldqt=100) == -1                # int8 transpose: ldqt a multiple of 64
    assert _pack(L, N=100, q=None, qt=PTR, ldqt=64) == -1          # ... covering N
    assert _pack(L, N=0) == -1 and _pack(L, K=0) == -1
    assert b"bnn_sgd_clamp_pack" in L.bnn_last_error()


# ------------------------------------------------------------------ LatentSGD (host side)
@pytest.mark.parametrize("kw", [dict(lr=-1.0), dict(momentum=-0.1), dict(weight_decay=-1e-3),
                                dict(nesterov=True), dict(nesterov=True, momentum=0.9, dampening=0.1)])
def test_latent_sgd_raises_what_torch_raises(kw):
    from bnn_amd.optim import LatentSGD
    full = dict(lr=0.1)
    full.update(kw)
    with pytest.raises(ValueError) as want:
        torch.optim.SGD([torch.nn.Parameter(torch.zeros(3))], **full)
    with pytest.raises(ValueError) as got:
        LatentSGD([torch.nn.Parameter(torch.zeros(3))], **full)
    assert str(got.value) == str(want.value)


def test_latent_sgd_loads_a_torch_sgd_state_dict():
    from bnn_amd.optim import LatentSGD
    torch.manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(5, 3)), torch.nn.Parameter(torch.randn(4))]
    ref = torch.optim.SGD(ps, lr=0.05, momentum=0.9, dampening=0.1, weight_decay=5e-4)
    for p in ps:
        p.grad = torch.randn_like(p)
    ref.step()
    sd = ref.state_dict()
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    opt = LatentSGD(qs, lr=1.0, clamp_params=qs[:1])
    opt.load_state_dict(sd)
    g = opt.param_groups[0]
    assert (g["lr"], g["momentum"], g["dampening"], g["weight_decay"], g["nesterov"]) == (0.05, 0.9, 0.1, 5e-4, False)
    for p, q in zip(ps, qs):
        assert torch.equal(opt.state[q]["momentum_buffer"], ref.state[p]["momentum_buffer"])
    assert set(opt.state_dict()["state"][0]) == {"momentum_buffer"}
    # momentum 0: no state at all, as torch
    assert LatentSGD(qs, lr=0.1).state_dict()["state"] == {}
    # a maximizing group is refused
    sd["param_groups"][0]["maximize"] = True
    with pytest.raises(ValueError, match="maximize"):
        LatentSGD(qs, lr=0.1).load_state_dict(sd)


def test_trainer_flags_and_resume_mismatch(tmp_path):
    from bnn_amd import trainer
    a = trainer.parse([])
    assert (a.optimizer, a.momentum, a.dampening, a.weight_decay, a.nesterov) == ("adam", 0.0, 0.0, 0.0, False)
    assert a.lr == 0.01 and a.batch_size == 64 and a.graph is False
    a = trainer.parse(["--optimizer", "sgd", "--momentum", "0.9", "--dampening", "0.1", "--weight-decay", "5e-4"])
    assert (a.optimizer, a.momentum, a.dampening, a.weight_decay, a.nesterov) == ("sgd", 0.9, 0.1, 5e-4, False)
    assert trainer.parse(["--optimizer", "sgd", "--momentum", "0.9", "--nesterov"]).nesterov is True
    with pytest.raises(SystemExit):
        trainer.parse(["--optimizer", "rmsprop"])
    # the kind of a stored optimizer state, and the refusal that names both
    p = [torch.nn.Parameter(torch.zeros(2))]
    assert trainer.optimizer_kind(torch.optim.SGD(p, lr=0.1).state_dict()) == "sgd"
    assert trainer.optimizer_kind(torch.optim.Adam(p).state_dict()) == "adam"
    path = str(tmp_path / "ck.pt")
    torch.save({"format": "bnn_amd.checkpoint/1", "optimizer": torch.optim.Adam(p).state_dict()}, path)
    with pytest.raises(SystemExit, match="adam.*sgd"):
        trainer.check_resume_optimizer(path, "sgd")
    trainer.check_resume_optimizer(path, "adam")
