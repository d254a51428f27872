"""Bop on the GPU (bnn_bop / bnn_bop_pack, optim.LatentBop, the trainer's --optimizer bop).

* the flat kernel equals the numpy restatement of bop_elem (tests/bop_ref.py, itself held to the same formula
  in torch CPU fp32 ops bit for bit by tests/test_bop.py) bit for bit in w and m, and in the flip count;
* the fused update + pack equals bop_ followed by sign-packing the result, in all three kernel forms;
* LatentBop on the fused trainer path: one whole step against the restatement and LatentAdam, under
  GraphedStep, through a checkpoint, and from the trainer;
* it learns real digits as well as the CPU reference run does.
"""
import os

import numpy as np
import pytest
import torch

import bop_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

F32 = np.float32
GAMMA, THR = R.GAMMA, R.THRESHOLD


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


def counter():
    return torch.zeros(1, dtype=torch.int64, device="cuda")


# ------------------------------------------------------------------ the flat kernel
@pytest.mark.parametrize("gscale", R.GSCALES)
@pytest.mark.parametrize("n", [1, 37, 1001, 65536 + 3])
def test_bop_equals_restatement(F, n, gscale):
    rng = np.random.default_rng(7 * n)
    w_ref, m_ref, total = R.make_w0(n, rng), np.zeros(n, F32), 0
    w, m, flips = dev(w_ref), dev(m_ref), counter()
    for step in range(2):
        g = R.make_grad(n, rng)
        F.bop_(w, dev(g), m, GAMMA, THR, grad_scale=gscale, flips=flips)
        w_ref, m_ref, f = R.bop_step(w_ref, g, m_ref, GAMMA, THR, gscale)
        total += f
        assert same(w, w_ref) and same(m, m_ref), step
        assert int(flips.item()) == total, step
    if n > 1000:
        assert 0 < total < 2 * n


def test_bop_tie_cases(F):
    rng = np.random.default_rng(5)
    n = 65536 + 3
    w0, g, must, kw = R.make_tie(n, rng)
    w, m, flips = dev(w0), torch.zeros(n, device="cuda"), counter()
    F.bop_(w, dev(g), m, kw["gamma"], kw["threshold"], grad_scale=kw["gscale"], flips=flips)
    w_ref, m_ref, f = R.bop_step(w0, g, np.zeros(n, F32), **kw)
    assert same(w, w_ref) and same(m, m_ref) and int(flips.item()) == f == int(must.sum())
    s = np.where(w0 < 0, F32(-1), F32(1))
    assert np.array_equal(w.cpu().numpy() != s, must)
    assert (np.abs(m_ref) == F32(kw["threshold"])).any()


def test_bop_misaligned_views_and_no_counter(F):
    """Views offset by one element (4-B aligned only: the scalar form), and flips=None."""
    rng = np.random.default_rng(9)
    n = 1001
    w0, g = R.make_w0(n, rng), R.make_grad(n, rng)
    m0 = (0.3 * R.make_grad(n, rng)).astype(F32)
    base = [torch.full((n + 1,), 7.0, device="cuda") for _ in range(3)]
    w, gd, m = (b[1:] for b in base)
    w.copy_(dev(w0)), gd.copy_(dev(g)), m.copy_(dev(m0))
    assert w.data_ptr() % 16 == 4
    flips = counter()
    F.bop_(w, gd, m, GAMMA, THR, flips=flips)
    w_ref, m_ref, f = R.bop_step(w0, g, m0, GAMMA, THR)
    assert same(w, w_ref) and same(m, m_ref) and int(flips.item()) == f and f > 0
    assert all(float(b[0]) == 7.0 for b in base)
    # only the weight misaligned, no counter
    w2, m2 = base[0][1:], dev(m0)
    w2.copy_(dev(w0))
    F.bop_(w2, dev(g), m2, GAMMA, THR, flips=None)
    assert same(w2, w_ref) and same(m2, m_ref)


# ------------------------------------------------------------------ the fused update + pack
def _pack_inputs(N, K, seed):
    rng = np.random.default_rng(seed)
    w0 = dev(R.make_w0(N * K, rng).reshape(N, K))
    gs = [dev(R.make_grad(N * K, rng).reshape(N, K)) for _ in range(2)]
    return w0, gs


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


def _bop_pack(w, g, m, flips, fmt, q, qt, qt_fmt, gamma=GAMMA, thr=THR):
    from bnn_amd import _lib as L
    N, K = w.shape
    return L.lib().bnn_bop_pack(L.ptr(w), L.ptr(g), L.ptr(m), N, K, gamma, thr, 1.0 / 3.0, L.ptr(flips), fmt, L.ptr(q),
                                q.shape[1], L.ptr(qt), qt.shape[1], qt_fmt, L.stream())


@pytest.mark.parametrize("N,K", [(100, 37), (64, 784), (300, 1000), (512, 768)])
@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("qt_fmt", [0, 1])
def test_bop_pack_matches_unfused(F, N, K, fmt, qt_fmt):
    """bnn_bop_pack: w, m and the count bit-identical to bnn_bop; q / qt bit-identical to sign-packing the
    updated weight (padding zero).  A first step (any initial value) and a second (+-1 weights)."""
    w0, gs = _pack_inputs(N, K, N + K + fmt)
    a, b = w0.clone(), w0.clone()
    am, bm = torch.zeros_like(w0), torch.zeros_like(w0)
    af, bf = counter(), counter()
    for step, g in enumerate(gs):
        F.bop_(a, g, am, GAMMA, THR, grad_scale=1.0 / 3.0, flips=af)
        q, qt = _pack_buffers(F, N, K, fmt, qt_fmt)            # pre-filled: the padding must be rewritten
        assert _bop_pack(b, g, bm, bf, fmt, q, qt, qt_fmt) == 0
        assert torch.equal(a, b) and torch.equal(am, bm), step
        assert int(af.item()) == int(bf.item()), step
        if fmt == 1:
            q_ref, _ = F.sign_pack_fp4(a)
        else:
            q_ref, _ = F.sign_pack(a, True, False)
        _, qt_ref = F.sign_pack_fp4(a, want_qt=True, qt_fmt="fp4" if qt_fmt == 1 else "i8", want_q=False)
        assert torch.equal(q, q_ref) and torch.equal(qt, qt_ref), step
    assert int(af.item()) > 0 and bool((a.abs() == 1).all())      # flips occurred; nothing but +-1 remains


@pytest.mark.parametrize("N,K,qt_fmt", [(256, 256, 1), (512, 768, 1), (1024, 2048, 2)])
def test_bop_pack_tile256_equals_tile64(F, N, K, qt_fmt):
    """The 256 x 256-tile form of bnn_bop_pack (forced: bnn_adam_pack_set_tile256(2)) against the 64 x 64-tile
    kernel: w, m, flips, q, qt bit-identical on a first and a second step; the 64 x 64 result is also the
    unfused one."""
    from bnn_amd import _lib as L
    w0, gs = _pack_inputs(N, K, N + K)
    outs = []
    try:
        for tile256 in (2, 0):
            L.call("bnn_adam_pack_set_tile256", tile256)
            w, m, flips = w0.clone(), torch.zeros_like(w0), counter()
            rec = []
            for g in gs:
                q = torch.full((N, K // 2), 0x77, dtype=torch.uint8, device="cuda")
                qt = torch.full((K, N // 2), 0x77, dtype=torch.uint8, device="cuda")
                assert _bop_pack(w, g, m, flips, 1, q, qt, qt_fmt) == 0
                rec += [w.clone(), m.clone(), flips.clone(), q, qt]
            outs.append(rec)
    finally:
        L.call("bnn_adam_pack_set_tile256", int(os.environ.get("BNN_ADAM_TILE256", "1") != "0"))
    for x, y in zip(*outs):
        assert torch.equal(x, y)
    a, am, af = w0.clone(), torch.zeros_like(w0), counter()
    for g in gs:
        F.bop_(a, g, am, GAMMA, THR, grad_scale=1.0 / 3.0, flips=af)
    w, m, flips, q, qt = outs[0][5:]
    assert torch.equal(a, w) and torch.equal(am, m) and torch.equal(af, flips) and int(af.item()) > 0
    q_ref, qt_ref = F.sign_pack_fp4(a, want_qt=True, qt_fmt="fp4" if qt_fmt == 1 else "fp4p")
    assert torch.equal(q, q_ref) and torch.equal(qt.view(-1), qt_ref.view(-1))


def test_bop_argument_errors_leave_the_tensors_untouched(F):
    from bnn_amd import _lib as L
    N, K = 64, 64
    w0, gs = _pack_inputs(N, K, 1)
    w, g, m, flips = w0.clone(), gs[0], torch.zeros_like(w0), counter()
    q, qt = _pack_buffers(F, N, K, 0, 0)
    lib = L.lib()
    for gamma, thr in ((0.0, THR), (1.5, THR), (float("nan"), THR), (GAMMA, -1.0), (GAMMA, float("nan"))):
        assert lib.bnn_bop(L.ptr(w), L.ptr(g), L.ptr(m), N * K, gamma, thr, 1.0, L.ptr(flips), L.stream()) == -1
        assert _bop_pack(w, g, m, flips, 0, q, qt, 0, gamma=gamma, thr=thr) == -1
    assert lib.bnn_bop(L.ptr(w), None, L.ptr(m), N * K, GAMMA, THR, 1.0, L.ptr(flips), L.stream()) == -1
    assert _bop_pack(w, g, m, flips, 2, q, qt, 0) == -1
    assert lib.bnn_bop(None, None, None, 0, GAMMA, THR, 1.0, None, L.stream()) == 0
    with pytest.raises(L.BnnError, match="bnn_bop"):
        F.bop_(w, g, m, 2.0, THR)
    torch.cuda.synchronize()
    assert torch.equal(w, w0) and not bool(m.any()) and int(flips.item()) == 0
    assert bool((q == 7).all()) and bool((qt == 7).all())


# ------------------------------------------------------------------ LatentBop
OPT_GAMMA, OPT_THR = 0.05, 1e-5        # both nets flip weights from their first steps on at these (asserted below)


def _mlp(seed, p_drop=0.0):
    from bnn_amd import nets
    torch.manual_seed(seed)
    return nets.MLP(320, 192, 128, p_drop=p_drop, org_protocol=False, mutate_input=False, fused_bn=True).cuda().train()


def _cnn(seed):
    from bnn_amd import nets
    torch.manual_seed(seed)
    return nets.BinCNN(org_protocol=False, mutate_input=False, fused_bn=True).cuda().train()


def _bop(m, device_step=None):
    from bnn_amd.nets import binary_params, binary_weights
    from bnn_amd.optim import LatentBop
    return LatentBop(m.parameters(), lr=0.01, gamma=OPT_GAMMA, threshold=OPT_THR, bop_params=binary_weights(m),
                     clamp_params=binary_params(m), device_step=device_step)


def _state(m, opt):
    out = {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}
    for i, p in enumerate(m.parameters()):
        for k, v in opt.state.get(p, {}).items():
            out[f"opt{i}.{k}"] = v.detach().cpu().numpy().copy() if torch.is_tensor(v) else np.asarray(v)
    for gi, g in enumerate(opt.param_groups):
        out[f"group{gi}"] = np.asarray([g["gamma"], g["threshold"], g["lr"]])
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


def _whole_step_case(F, make_model, x, y):
    """Two steps; before the second, the gradient and the state go to the host: every Bop weight, its average
    and its counter equal the restatement, every other parameter what LatentAdam makes of the same state."""
    from bnn_amd.nets import binary_params, binary_weights
    from bnn_amd.optim import LatentAdam
    m = make_model()
    opt = _bop(m)
    step = _step_fn(m, opt, x, y)
    step()                                               # the first: binarizes, allocates the state
    bw = {id(p) for p in binary_weights(m)}
    assert all(bool((p.abs() == 1).all()) for p in binary_weights(m))
    for p in m.parameters():
        p.grad = None
    torch.nn.functional.cross_entropy(m(x), y).backward()
    before = {id(p): (p.detach().cpu().numpy().copy(), p.grad.cpu().numpy().copy()) for p in m.parameters()}
    st0 = {id(p): {k: (v.clone() if torch.is_tensor(v) else v) for k, v in opt.state[p].items()} for p in m.parameters()}
    # the Adam twin: clones of the other parameters with the same state and gradient
    others = [p for p in m.parameters() if id(p) not in bw]
    twins = [torch.nn.Parameter(p.detach().clone()) for p in others]
    clamp = {id(p) for p in binary_params(m)}
    adam = LatentAdam(twins, lr=0.01, clamp_params=[t for t, p in zip(twins, others) if id(p) in clamp])
    for t, p in zip(twins, others):
        t.grad = p.grad.clone()
        adam.state[t] = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st0[id(p)].items()}
    opt.step()
    adam.step()
    torch.cuda.synchronize()
    nbop = 0
    for p in m.parameters():
        if id(p) in bw:
            w0, g = before[id(p)]
            s0 = st0[id(p)]
            w_ref, m_ref, f = R.bop_step(w0, g, s0["bop_m"].cpu().numpy(), OPT_GAMMA, OPT_THR, 1.0)
            st = opt.state[p]
            assert same(p, w_ref) and same(st["bop_m"], m_ref), tuple(p.shape)
            assert int(st["flips"].item()) == int(s0["flips"].item()) + f
            assert st["step"] == 2 and "exp_avg" not in st
            nbop += f
    assert nbop > 0
    for t, p in zip(twins, others):
        assert torch.equal(t.detach(), p.detach()), tuple(p.shape)
        assert torch.equal(adam.state[t]["exp_avg"], opt.state[p]["exp_avg"])
        assert torch.equal(adam.state[t]["exp_avg_sq"], opt.state[p]["exp_avg_sq"])
    counts = opt.flip_counts()
    assert {id(p) for p in counts} == bw
    for p, (f, n, s) in counts.items():
        assert (f, n, s) == (int(opt.state[p]["flips"].item()), p.numel(), 2)
    opt.flip_counts(reset=True)
    assert all(v == (0, p.numel(), 0) for p, v in opt.flip_counts().items())


def test_latent_bop_whole_step_mlp(F):
    from bnn_amd.data import synthetic_mnist
    x, y = synthetic_mnist(256, seed=100, device="cuda")
    _whole_step_case(F, lambda: _mlp(21), x, y)


def test_latent_bop_whole_step_cnn(F):
    """The conv weights are 4-D: the flat kernel."""
    from bnn_amd.data import synthetic_mnist
    x, y = synthetic_mnist(64, seed=9, device="cuda", as_u8=False)
    _whole_step_case(F, lambda: _cnn(6), x, y)


def test_latent_bop_uses_repacked_weights(F):
    """LatentBop rewrites the next forward's packed weight operands in place (bnn_bop_pack): a run that drops
    the cache before every forward must produce bit-identical losses and parameters."""
    from bnn_amd.data import synthetic_mnist
    runs = []
    for drop_cache in (False, True):
        model = _mlp(21)
        opt = _bop(model)
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
        rec += [int(opt.state[p]["flips"].item()) for p in (model.fc1.weight, model.fc2.weight, model.fc3.weight)]
        if not drop_cache:
            ent = getattr(model.fc2.weight, "_bnn_pack", None)
            assert ent is not None and ent["key"] == F._pack_key(model.fc2.weight)      # survived, still valid
            assert set(opt.state[model.fc2.weight]) == {"step", "bop_m", "flips", "flips_since"}
        runs.append(rec)
    for a, b in zip(*runs):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    assert runs[0][0] != runs[0][3] and runs[0][-2] > 0           # the steps moved the loss; fc2 flipped


def _graph_case(F, make_model, x, y):
    from bnn_amd.graph import GraphedStep
    runs = []
    for graphed in (False, True):
        m = make_model()
        torch.manual_seed(99)                       # the DeviceStep's base dropout seed
        ds = F.DeviceStep().activate()
        try:
            opt = _bop(m, ds)
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
    flips = [k for k in a if k.endswith(".flips")]
    assert flips and any(int(a[k][0]) > 0 for k in flips) and any(k.endswith(".bop_m") for k in a)
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_graph_replays_equal_eager_device_steps_mlp(F):
    """n replays of a captured LatentBop step equal n eager device-step steps bit for bit, dropout and the
    flip counters included."""
    g = torch.Generator(device="cuda").manual_seed(3)
    u = torch.randint(0, 256, (256, 1, 28, 28), generator=g, device="cuda").to(torch.uint8)
    y = torch.randint(0, 10, (256,), generator=g, device="cuda")
    _graph_case(F, lambda: _mlp(5, p_drop=0.3), u, y)


def test_graph_replays_equal_eager_device_steps_cnn(F):
    from bnn_amd.data import synthetic_mnist
    x, y = synthetic_mnist(64, seed=9, device="cuda", as_u8=False)
    _graph_case(F, lambda: _cnn(6), x, y)


def test_capturing_a_first_step_raises(F):
    """A captured step cannot allocate the averages and counters: an optimizer that has not stepped raises."""
    from bnn_amd.data import synthetic_mnist
    m = _mlp(8)
    ds = F.DeviceStep().activate()
    try:
        opt = _bop(m, ds)
        x, y = synthetic_mnist(64, seed=1, device="cuda")
        torch.nn.functional.cross_entropy(m(x), y).backward()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with pytest.raises(RuntimeError, match="first"):
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                opt.step()
        assert not opt.state_dict()["state"] and ds.steps == 0
        opt.step()                                   # eager: allocates the state and steps
        torch.cuda.synchronize()
        assert ds.steps == 1 and "bop_m" in opt.state[m.fc2.weight]
    finally:
        ds.deactivate()


def test_checkpoint_resumes_bit_for_bit(F, tmp_path):
    """2 steps, save, a fresh model and LatentBop, load, 2 more steps == 4 uninterrupted steps."""
    from bnn_amd.checkpoint import load_checkpoint, save_checkpoint
    from bnn_amd.data import synthetic_mnist
    from bnn_amd.nets import binary_params, binary_weights
    from bnn_amd.optim import LatentBop
    batches = [synthetic_mnist(256, seed=200 + s, device="cuda") for s in range(4)]

    def run(m, opt, which):
        for s in which:
            _step_fn(m, opt, *batches[s])()

    full = _mlp(31)
    full_opt = _bop(full)
    run(full, full_opt, range(4))
    a = _mlp(31)
    a_opt = _bop(a)
    run(a, a_opt, range(2))
    path = str(tmp_path / "bop.pt")
    save_checkpoint(path, a, a_opt, epoch=1)
    b = _mlp(32)                                       # other initial weights and settings: all come from the file
    b_opt = LatentBop(b.parameters(), lr=0.5, gamma=0.9, threshold=3.0, bop_params=binary_weights(b),
                      clamp_params=binary_params(b))
    assert load_checkpoint(path, b, b_opt) == 1
    assert b_opt.state[b.fc2.weight]["flips"].dtype == torch.int64
    run(b, b_opt, range(2, 4))
    torch.cuda.synchronize()
    want, got = _state(full, full_opt), _state(b, b_opt)
    assert set(want) == set(got)
    assert any(k.endswith(".bop_m") for k in want) and any(k.endswith(".flips") and int(want[k][0]) > 0 for k in want)
    assert want["group0"].tolist() == [OPT_GAMMA, OPT_THR, 0.01]
    for k in want:
        assert np.array_equal(want[k], got[k]), k


# ------------------------------------------------------------------ the trainer
TRAINER = ["--model", "cnn", "--optimizer", "bop", "--bop-gamma", "0.05", "--bop-threshold", "1e-5", "--lr", "1e-3",
           "--batch-size", "100", "--dataset-size", "400", "--epochs", "1"]


def test_trainer_bop_cnn(F, capsys):
    from bnn_amd import nets, trainer
    m = trainer.main(TRAINER)
    assert isinstance(m, nets.BinCNN) and F._DEVICE_STEP is None
    for p in m.parameters():
        assert torch.isfinite(p).all()
    for p in nets.binary_weights(m):
        assert bool((p.abs() == 1).all())
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Flips 1 :")]
    assert len(lines) == 1
    fields = lines[0].split(":", 1)[1].split()
    assert fields[0::2] == ["layer1.0.weight", "layer2.0.weight"]
    assert all(0.0 <= float(v) <= 1.0 for v in fields[1::2]) and any(float(v) > 0 for v in fields[1::2])


def test_trainer_bop_graph_equals_device_step(F):
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


# ------------------------------------------------------------------ it learns
# The CPU reference run: oracle/bnn_torch.py's RefMLP at SmallNet's widths with tests/bop_ref.py's
# bop_step on the three binarized weights and torch.optim.Adam(lr 0.01) + the bias clamp on the rest, no dropout,
# the split, batches, initial weights (torch.manual_seed(5)) and settings below.
LEARN_GAMMA, LEARN_THR, LEARN_STEPS, LEARN_BATCH = 0.01, 1e-5, 400, 100
# Held-out accuracy of that CPU run, measured on the host in fp32 with this file's bop_ref: 1864 of 2000, at a mean
# flip ratio of 1.04e-3.  The same run with threshold = inf (no flips, only the Adam parameters learn): 0.8200.
A_REF = 0.9320


def test_bop_learns_real_digits(F):
    """SmallNet + LatentBop on the first 8000 t10k digits, held out: the last 2000.  The flip decisions
    diverge chaotically between implementations, so the bar is statistical: the held-out accuracy is no lower
    than the CPU reference run's less 3 binomial standard errors at 2000 samples, and the mean flip ratio
    over the run lies in (0, 0.5)."""
    from bnn_amd import nets
    from bnn_amd.data import load_idx_dataset
    from bnn_amd.inference import freeze
    from bnn_amd.optim import LatentBop
    x, y = load_idx_dataset(os.path.join(GOLDEN, "t10k-images-idx3-ubyte.gz"),
                            os.path.join(GOLDEN, "t10k-labels-idx1-ubyte.gz"), "cuda")
    xtr, ytr, xho, yho = x[:8000], y[:8000], x[8000:], y[8000:]
    torch.manual_seed(5)
    state = {k: v.clone() for k, v in nets.SmallNet(p_drop=0.0).state_dict().items()}
    m = nets.SmallNet(p_drop=0.0, org_protocol=False, mutate_input=False, fused_bn=True)
    m.load_state_dict(state)
    m = m.cuda().train()
    opt = LatentBop(m.parameters(), lr=0.01, gamma=LEARN_GAMMA, threshold=LEARN_THR, bop_params=nets.binary_weights(m),
                    clamp_params=nets.binary_params(m))
    nb = len(xtr) // LEARN_BATCH
    for s in range(LEARN_STEPS):
        b = s % nb
        for p in m.parameters():
            p.grad = None
        sl = slice(b * LEARN_BATCH, (b + 1) * LEARN_BATCH)
        torch.nn.functional.cross_entropy(m(xtr[sl]), ytr[sl]).backward()
        opt.step()
    counts = opt.flip_counts()
    ratio = sum(f for f, _, _ in counts.values()) / sum(n * s for _, n, s in counts.values())
    acc = freeze(m).accuracy(xho, yho, batch=2000)
    bar = A_REF - 3 * (A_REF * (1 - A_REF) / 2000) ** 0.5
    print(f"\nheld-out accuracy {acc:.4f} (reference {A_REF:.4f}, bar {bar:.4f}); mean flip ratio {ratio:.3e}")
    assert acc >= bar
    assert 0.0 < ratio < 0.5
