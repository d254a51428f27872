"""The fused latent SGD on the GPU (bnn_sgd_clamp / _multi / _pack, optim.LatentSGD, the trainer's
--optimizer sgd).

* the flat and multi-tensor kernels equal the numpy restatement of sgd_elem (tests/sgd_ref.py, itself held
  to torch.optim.SGD's CPU fp32 result bit for bit by tests/test_sgd.py) bit for bit in p and buf;
* the fused update + pack equals sgd_clamp_ followed by sign-packing the result, in all three kernel forms;
* against torch.optim.SGD in float64 on the device, within a bound that does not depend on contraction;
* LatentSGD on the fused trainer path, under GraphedStep, through a checkpoint, and from the trainer.
"""
import os

import numpy as np
import pytest
import torch

import sgd_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32
LR = 0.05


@pytest.fixture(scope="module")
def F():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from bnn_amd import functional
    return functional


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def same(t, a):
    return np.array_equal(bits(t), np.asarray(a, F32).view(np.uint32))


# ------------------------------------------------------------------ flat and multi-tensor kernels
@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("setting", R.SETTINGS)
def test_sgd_clamp_equals_restatement(F, setting, clamp):
    mu, damp, wd, nest = setting
    for n in (1, 37, 1001, 65536 + 3):
        for gscale in R.GSCALES:
            rng = np.random.default_rng(7 * n + int(clamp))
            p_ref, buf_ref = R.make_p0(n, rng), None
            p = dev(p_ref)
            buf = torch.full((n,), float("nan"), device="cuda") if mu != 0 else None      # first: never read
            for first in (True, False):
                g = R.make_grad(n, rng)
                F.sgd_clamp_(p, dev(g), buf, LR, mu, damp, wd, nest, first=first, grad_scale=gscale, clamp=clamp)
                p_ref, buf_ref = R.sgd_step(p_ref, g, buf_ref, LR, mu, damp, wd, nest, first, gscale, clamp)
                assert same(p, p_ref), (n, gscale, first)
                if mu != 0:
                    assert same(buf, buf_ref), (n, gscale, first)


@pytest.mark.parametrize("setting", R.SETTINGS)
def test_sgd_clamp_multi_equals_restatement(F, setting):
    """16 tensors of mixed sizes in one launch, mixed first / clamp flags, one of them empty."""
    mu, damp, wd, nest = setting
    sizes = [1, 37, 1001, 65536 + 3, 0, 7, 64, 255, 256, 257, 4096, 3, 1023, 513, 100, 2]
    rng = np.random.default_rng(31)
    items, want = [], []
    for j, n in enumerate(sizes):
        first, clamp = j % 3 == 0, j % 2 == 0
        p0, g = R.make_p0(n, rng), R.make_grad(n, rng)
        b0 = (0.5 * R.make_grad(n, rng)).astype(F32)
        buf = None
        if mu != 0:
            buf = torch.full((n,), float("nan"), device="cuda") if first else dev(b0)
        items.append((dev(p0), dev(g), buf, first, clamp))
        want.append(R.sgd_step(p0, g, b0, LR, mu, damp, wd, nest, first, 1.0 / 3.0, clamp))
    assert len(items) == F.ADAM_MULTI_MAX
    F.sgd_clamp_multi_(items, LR, mu, damp, wd, nest, grad_scale=1.0 / 3.0)
    for (p, _, buf, _, _), (p_ref, buf_ref) in zip(items, want):
        assert same(p, p_ref)
        if mu != 0:
            assert same(buf, buf_ref)


# ------------------------------------------------------------------ the fused update + pack
def _pack_inputs(N, K, seed):
    """The CPU test's recipe on the device; the gradient is zero on half of p0's exact zeros, so some
    updated weights stay exactly zero (the zero sign code is packed)."""
    g0 = torch.Generator(device="cuda").manual_seed(seed)
    p0 = torch.empty(N, K, device="cuda").uniform_(-1.1, 1.1, generator=g0)
    zero = torch.rand(N, K, device="cuda", generator=g0) < 0.01
    p0[zero] = 0.0
    gs = []
    for _ in range(2):
        g = torch.randn(N, K, device="cuda", generator=g0)
        g[zero & (torch.rand(N, K, device="cuda", generator=g0) < 0.5)] = 0.0
        gs.append(g)
    return p0, gs


def _pack_buffers(F, N, K, fmt, qt_fmt):
    if fmt == 1:
        q = torch.full((N, F.round_up(K, 256) // 2), 0x77, dtype=torch.uint8, device="cuda")
    else:
        q = torch.full((N, F.round_up(K)), 7, dtype=torch.int8, device="cuda")
    if qt_fmt >= 1:
        qt = torch.full((K, F.round_up(N, 256) // 2), 0x77, dtype=torch.uint8, device="cuda")
    else:
        qt = torch.full((K, F.round_up(N)), 7, dtype=torch.int8, device="cuda")
    return q, qt


def _sgd_pack(F, p, g, buf, setting, first, fmt, q, qt, qt_fmt):
    from bnn_amd import _lib as L
    mu, damp, wd, nest = setting
    N, K = p.shape
    L.call("bnn_sgd_clamp_pack", L.ptr(p), L.ptr(g), L.ptr(buf), N, K, LR, mu, float(R.omd_of(damp)), wd, int(nest),
           int(first), 1.0 / 3.0, 1, fmt, L.ptr(q), q.shape[1], L.ptr(qt), qt.shape[1], qt_fmt, L.stream())


def _check_pack_matches_unfused(F, N, K, fmt, qt_fmt, setting):
    mu, damp, wd, nest = setting
    p0, gs = _pack_inputs(N, K, N + K + fmt)
    a, b = p0.clone(), p0.clone()
    abuf = torch.full_like(p0, float("nan")) if mu != 0 else None
    bbuf = torch.full_like(p0, float("nan")) if mu != 0 else None
    for first, g in zip((True, False), gs):
        F.sgd_clamp_(a, g, abuf, LR, mu, damp, wd, nest, first=first, grad_scale=1.0 / 3.0, clamp=True)
        q, qt = _pack_buffers(F, N, K, fmt, qt_fmt)            # pre-filled: the padding must be rewritten
        _sgd_pack(F, b, g, bbuf, setting, first, fmt, q, qt, qt_fmt)
        assert torch.equal(a, b), first
        if mu != 0:
            assert torch.equal(abuf, bbuf), first
        if fmt == 1:
            q_ref, _ = F.sign_pack_fp4(a)
        else:
            q_ref, _ = F.sign_pack(a, True, False)
        _, qt_ref = F.sign_pack_fp4(a, want_qt=True, qt_fmt="fp4" if qt_fmt == 1 else "i8", want_q=False)
        assert torch.equal(q, q_ref) and torch.equal(qt, qt_ref), first
    assert int((a == 0).sum()) > 0 and int((a.abs() == 1).sum()) > 0      # the zero sign and the clamp occurred


@pytest.mark.parametrize("N,K", [(100, 37), (64, 784), (300, 1000), (512, 768)])
@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("qt_fmt", [0, 1])
def test_sgd_clamp_pack_matches_unfused(F, N, K, fmt, qt_fmt):
    """bnn_sgd_clamp_pack: p, buf bit-identical to bnn_sgd_clamp; q / qt bit-identical to sign-packing the
    updated weight (padding zero).  A first step (buffer written only), then a second (read and written)."""
    for setting in ((0.9, 0.1, 5e-4, False), (0.95, 0.0, 5e-4, True)):
        _check_pack_matches_unfused(F, N, K, fmt, qt_fmt, setting)


@pytest.mark.parametrize("fmt,qt_fmt", [(0, 0), (1, 1)])
def test_sgd_clamp_pack_without_momentum(F, fmt, qt_fmt):
    """momentum 0: buf is NULL and the pass reads p and g only (64 x 64 tiles at the ragged shape)."""
    _check_pack_matches_unfused(F, 100, 37, fmt, qt_fmt, (0.0, 0.0, 1e-2, False))


@pytest.mark.parametrize("N,K,qt_fmt,setting", [(256, 256, 1, (0.9, 0.1, 5e-4, False)),
                                                (256, 256, 1, (0.0, 0.0, 1e-2, False)),
                                                (512, 768, 1, (0.95, 0.0, 5e-4, True)),
                                                (1024, 2048, 2, (0.9, 0.1, 5e-4, False))])
def test_sgd_pack_tile256_equals_tile64(F, N, K, qt_fmt, setting):
    """The 256 x 256-tile form of bnn_sgd_clamp_pack (forced: bnn_adam_pack_set_tile256(2)) against the
    64 x 64-tile kernel: p, buf, q, qt bit-identical, on a first and a second step; the 64 x 64 result is
    also the unfused one."""
    from bnn_amd import _lib as L
    mu, damp, wd, nest = setting
    p0, gs = _pack_inputs(N, K, N + K)
    outs = []
    try:
        for tile256 in (2, 0):
            L.call("bnn_adam_pack_set_tile256", tile256)
            p = p0.clone()
            buf = torch.full_like(p0, float("nan")) if mu != 0 else None
            rec = []
            for first, g in zip((True, False), gs):
                q = torch.full((N, K // 2), 0x77, dtype=torch.uint8, device="cuda")
                qt = torch.full((K, N // 2), 0x77, dtype=torch.uint8, device="cuda")
                _sgd_pack(F, p, g, buf, setting, first, 1, q, qt, qt_fmt)
                rec += [p.clone(), q, qt] + ([buf.clone()] if mu != 0 else [])
            outs.append(rec)
    finally:
        L.call("bnn_adam_pack_set_tile256", int(os.environ.get("BNN_ADAM_TILE256", "1") != "0"))
    for x, y in zip(*outs):
        assert torch.equal(x, y)
    a = p0.clone()
    abuf = torch.full_like(p0, float("nan")) if mu != 0 else None
    for first, g in zip((True, False), gs):
        F.sgd_clamp_(a, g, abuf, LR, mu, damp, wd, nest, first=first, grad_scale=1.0 / 3.0, clamp=True)
    n = 4 if mu != 0 else 3                       # the second step's entries: p, q, qt (, buf)
    assert torch.equal(a, outs[0][n])
    if mu != 0:
        assert torch.equal(abuf, outs[0][n + 3])
    q_ref, qt_ref = F.sign_pack_fp4(a, want_qt=True, qt_fmt="fp4" if qt_fmt == 1 else "fp4p")
    assert torch.equal(outs[0][n + 1], q_ref) and torch.equal(outs[0][n + 2].view(-1), qt_ref.view(-1))


# ------------------------------------------------------------------ against torch itself
@pytest.mark.parametrize("setting", R.SETTINGS)
def test_sgd_clamp_vs_torch_float64_on_device(F, setting):
    """One step, and one more, of torch.optim.SGD in float64 on the GPU from the same fp32 state.  Each fp32
    result lies within 8 * 2^-24 * (|p| + lr * (|g * gscale| + wd * |p| + (1 + mu) * |buf|)) of it
    element-wise: a path has at most four roundings of intermediates no larger than that sum (|buf| is
    the larger of the buffer before and after the step; the buffer itself is held to the same sum without
    the |p| term and the factor lr).  Independent of whether torch's kernels contract: this pins the
    semantics -- first-step rule, Nesterov, where weight decay enters -- to torch on the device."""
    mu, damp, wd, nest = setting
    n, gscale, eps = 65536 + 3, 1.0 / 3.0, 8.0 * 2.0 ** -24
    rng = np.random.default_rng(77)
    p = dev(R.make_p0(n, rng))
    buf = torch.full((n,), float("nan"), device="cuda") if mu != 0 else None
    for first in (True, False):
        g = dev(R.make_grad(n, rng))
        P = torch.nn.Parameter(p.double())
        opt = torch.optim.SGD([P], lr=LR, momentum=mu, dampening=damp, weight_decay=wd, nesterov=nest)
        b_old = torch.zeros_like(P)
        if mu != 0 and not first:
            b_old = buf.double()
            opt.state[P]["momentum_buffer"] = b_old.clone()
        P.grad = g.double() * gscale
        p_old = P.detach().clone()
        opt.step()
        F.sgd_clamp_(p, g, buf, LR, mu, damp, wd, nest, first=first, grad_scale=gscale, clamp=False)
        b_new = opt.state[P]["momentum_buffer"] if mu != 0 else b_old
        inner = P.grad.abs() + wd * p_old.abs() + (1 + mu) * torch.maximum(b_old.abs(), b_new.abs())
        err = (p.double() - P.detach()).abs()
        bound = eps * (p_old.abs() + LR * inner)
        print(f"{setting} first={first}: max err / bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= bound).all()), first
        if mu != 0:
            assert bool(((buf.double() - b_new).abs() <= eps * inner).all()), first


# ------------------------------------------------------------------ LatentSGD
def _mlp(seed, p_drop=0.0):
    from bnn_amd import nets
    torch.manual_seed(seed)
    return nets.MLP(320, 192, 128, p_drop=p_drop, org_protocol=False, mutate_input=False, fused_bn=True).cuda().train()


def _sgd(m, device_step=None):
    from bnn_amd.nets import binary_params
    from bnn_amd.optim import LatentSGD
    return LatentSGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=5e-4, clamp_params=binary_params(m),
                     device_step=device_step)


def _state(m, opt):
    out = {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}
    for i, p in enumerate(m.parameters()):
        st = opt.state.get(p, {})
        if "momentum_buffer" in st:
            out[f"opt{i}.momentum_buffer"] = st["momentum_buffer"].cpu().numpy().copy()
    return out


def _step_fn(m, opt, x, y):
    crit = torch.nn.CrossEntropyLoss()

    def step():
        for p in m.parameters():
            p.grad = None
        loss = crit(m(x), y)
        loss.backward()
        opt.step()
        return loss
    return step


def test_latent_sgd_uses_repacked_weights(F):
    """LatentSGD rewrites the next forward's packed weight operands in place (bnn_sgd_clamp_pack): a run that
    drops the cache before every forward must produce bit-identical losses and parameters."""
    from bnn_amd.data import synthetic_mnist
    runs = []
    for drop_cache in (False, True):
        model = _mlp(21)
        opt = _sgd(model)
        rec = []
        for s in range(4):
            x, y = synthetic_mnist(256, seed=100 + s, device="cuda")
            if drop_cache:
                for p in model.parameters():
                    F.invalidate_packed(p)
            for p in model.parameters():
                p.grad = None
            loss = torch.nn.functional.cross_entropy(model(x), y)
            loss.backward()
            rec.append(loss.item())
            opt.step()
        rec += [p.detach().cpu().numpy() for p in model.parameters()]
        if not drop_cache:
            ent = getattr(model.fc2.weight, "_bnn_pack", None)
            assert ent is not None and ent["key"] == F._pack_key(model.fc2.weight)      # survived, still valid
            assert set(opt.state[model.fc2.weight]) == {"momentum_buffer"}
        runs.append(rec)
    for a, b in zip(*runs):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    assert runs[0][0] != runs[0][3]                       # the steps moved the loss


def _graph_case(F, make_model, x, y):
    from bnn_amd.graph import GraphedStep
    runs = []
    for graphed in (False, True):
        m = make_model()
        torch.manual_seed(99)                       # the DeviceStep's base dropout seed
        ds = F.DeviceStep().activate()
        try:
            opt = _sgd(m, ds)
            step = _step_fn(m, opt, x, y)
            losses = []
            if graphed:
                g = GraphedStep(step, opt, ds, warmup=2)       # 2 eager steps + capture
                for _ in range(3):
                    losses.append(float(g().item()))
            else:
                for i in range(5):
                    loss = step()
                    if i >= 2:
                        losses.append(float(loss.item()))
            torch.cuda.synchronize()
            assert ds.steps == 5 and int(ds.ctr.item()) == 5
            runs.append((_state(m, opt), losses))
        finally:
            ds.deactivate()
    (a, la), (b, lb) = runs
    assert la == lb
    assert any(k.endswith("momentum_buffer") for k in a)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_graph_replays_equal_eager_device_steps_mlp(F):
    """n replays of a captured LatentSGD step equal n eager device-step steps bit for bit, dropout included."""
    g = torch.Generator(device="cuda").manual_seed(3)
    u = torch.randint(0, 256, (256, 1, 28, 28), generator=g, device="cuda").to(torch.uint8)
    y = torch.randint(0, 10, (256,), generator=g, device="cuda")
    _graph_case(F, lambda: _mlp(5, p_drop=0.3), u, y)


def test_graph_replays_equal_eager_device_steps_cnn(F):
    from bnn_amd import nets
    from bnn_amd.data import synthetic_mnist
    x, y = synthetic_mnist(64, seed=9, device="cuda", as_u8=False)

    def make():
        torch.manual_seed(6)
        return nets.BinCNN(org_protocol=False, mutate_input=False, fused_bn=True).cuda().train()
    _graph_case(F, make, x, y)


def test_capturing_a_first_step_raises(F):
    """A captured step cannot allocate the momentum buffers: an optimizer that has not stepped raises."""
    from bnn_amd.data import synthetic_mnist
    m = _mlp(8)
    ds = F.DeviceStep().activate()
    try:
        opt = _sgd(m, ds)
        x, y = synthetic_mnist(64, seed=1, device="cuda")
        torch.nn.functional.cross_entropy(m(x), y).backward()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with pytest.raises(RuntimeError, match="first"):
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                opt.step()
        assert not opt.state_dict()["state"] and ds.steps == 0
        opt.step()                                   # eager: allocates the buffers and steps
        torch.cuda.synchronize()
        assert ds.steps == 1 and "momentum_buffer" in opt.state[m.fc2.weight]
    finally:
        ds.deactivate()


def test_checkpoint_resumes_bit_for_bit(F, tmp_path):
    """2 steps, save, a fresh model and LatentSGD, load, 2 more steps == 4 uninterrupted steps."""
    from bnn_amd.checkpoint import load_checkpoint, save_checkpoint
    from bnn_amd.data import synthetic_mnist
    batches = [synthetic_mnist(256, seed=200 + s, device="cuda") for s in range(4)]

    def run(m, opt, which):
        for s in which:
            _step_fn(m, opt, *batches[s])()

    full = _mlp(31)
    full_opt = _sgd(full)
    run(full, full_opt, range(4))
    a = _mlp(31)
    a_opt = _sgd(a)
    run(a, a_opt, range(2))
    path = str(tmp_path / "sgd.pt")
    save_checkpoint(path, a, a_opt, epoch=1)
    b = _mlp(32)                                       # other initial weights: everything comes from the file
    b_opt = _sgd(b)
    assert load_checkpoint(path, b, b_opt) == 1
    run(b, b_opt, range(2, 4))
    torch.cuda.synchronize()
    want, got = _state(full, full_opt), _state(b, b_opt)
    assert set(want) == set(got) and any(k.endswith("momentum_buffer") for k in want)
    for k in want:
        assert np.array_equal(want[k], got[k]), k


# ------------------------------------------------------------------ the trainer
TRAINER = ["--model", "cnn", "--optimizer", "sgd", "--momentum", "0.9", "--lr", "1e-4", "--batch-size", "100",
           "--dataset-size", "400", "--epochs", "1"]


def test_trainer_sgd_cnn(F):
    from bnn_amd import nets, trainer
    m = trainer.main(TRAINER)
    assert isinstance(m, nets.BinCNN) and F._DEVICE_STEP is None
    for p in m.parameters():
        assert torch.isfinite(p).all()
    for p in nets.binary_params(m):
        assert float(p.min()) >= -1.0 and float(p.max()) <= 1.0


def test_trainer_sgd_graph_equals_device_step(F):
    from bnn_amd import trainer
    states = []
    for mode in ("--graph", "--device-step"):
        torch.manual_seed(0)
        m = trainer.main(TRAINER + [mode])
        torch.cuda.synchronize()
        states.append({k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()})
    assert F._DEVICE_STEP is None
    a, b = states
    for k in a:
        assert np.array_equal(a[k], b[k]), k
