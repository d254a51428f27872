"""The hinge criteria on libbnn (bnn_hinge_fwd / bnn_hinge_bwd; bnn_amd.functional.hinge_loss,
bnn_amd.nn.HingeLoss / SqrtHingeLoss), the nets' log_softmax=False switch and the trainer's --loss.

The kernels' arithmetic is fixed (include/bnn.h): v = fl(margin - fl(x*t)), h = (v <= 0) ? 0 : v, the
terms h or fl(h*h) summed in double, loss = fl(S / (M*C)); dx = (v <= 0) ? 0 : fl(-t*g) or
fl(fl(fl(-2t)*v)*g) with g = fl(go / fl(M*C)).  So:

* the loss is within one fp32 ulp (2^-23 relative) of the float64 mean of the same fp32 terms restated
  elementwise in torch -- at most 2^22 non-negative terms are summed in double, so the sum is within
  2^-31 of exact whatever the order and only the final rounding to fp32 shows -- and within 1e-6 of the
  torch-ops module path (the project's cross-entropy bar);
* the gradient is bit-identical to the elementwise torch restatement, exact zeros at the ties included,
  for go = 1 and go = 3; int64 labels and their dense +-1 one-vs-all target agree bit for bit;
* over every row count at which the forward changes path (1024: the one-workgroup kernel's row stride;
  16384 / 16385: its upper bound and the first block + fold batch; 16641: not a multiple of the block)
  and every supported class count.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 10), (7, 10), (300, 10), (1023, 10), (1024, 10), (1025, 10), (16384, 10), (16385, 10), (16641, 10),
          (65536, 10), (1000, 2), (513, 16), (256, 32), (1000, 64)]


@pytest.fixture(scope="module")
def F():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from bnn_amd import functional
    return functional


def _one_vs_all(y, C):
    return torch.where(y.unsqueeze(1) == torch.arange(C, device=y.device), 1.0, -1.0)


def _case(M, C, seed, margin=1.0):
    """(x, y, T): logits randn * 3, labels, their +-1 one-vs-all target; a handful of exact ties
    x = margin * t planted (the first and the last element among them)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(M, C, generator=g, device="cuda") * 3.0
    y = torch.randint(0, C, (M,), generator=g, device="cuda")
    T = _one_vs_all(y, C)
    n = M * C
    ties = torch.tensor(sorted({0, n // 3, n // 2, (2 * n) // 3 + 1, n - 1}), device="cuda")
    x.view(-1)[ties] = margin * T.view(-1)[ties]
    return x, y, T, ties


def _restate(x, T, margin, squared, go):
    """(float64 mean of the fp32 terms, fp32 gradient) in the kernels' arithmetic order, one torch op per
    rounding."""
    M, C = x.shape
    v = margin - x * T
    dead = v <= 0
    h = torch.where(dead, torch.zeros_like(v), v)
    terms = h * h if squared else h
    ref = float(terms.double().sum() / float(M * C))
    # g on the host: one IEEE fp32 division of two exactly representable numbers
    g = (torch.tensor(float(go), dtype=torch.float32) / torch.tensor(float(M * C), dtype=torch.float32)).cuda()
    d = ((-2.0 * T) * v) * g if squared else (-T) * g
    return ref, torch.where(dead, torch.zeros_like(d), d)


def _run(F, x, target, margin, squared, scale):
    a = x.clone().requires_grad_(True)
    loss = F.hinge_loss(a, target, margin, squared)
    (loss if scale == 1.0 else scale * loss).backward()
    return loss.detach(), a.grad


@pytest.mark.parametrize("M,C", SHAPES)
def test_loss_and_gradient_match_the_restatement(F, M, C):
    from bnn_amd.nn import HingeLoss, SqrtHingeLoss
    x, y, T, ties = _case(M, C, M * 7 + C)
    for squared in (False, True):
        ref, dref1 = _restate(x, T, 1.0, squared, 1.0)
        _, dref3 = _restate(x, T, 1.0, squared, 3.0)
        ll, gl = _run(F, x, y, 1.0, squared, 1.0)          # labels
        ld, gd = _run(F, x, T, 1.0, squared, 1.0)          # dense +-1
        print(f"M={M} C={C} squared={squared}: loss {float(ll)!r} ref {ref!r} rel "
              f"{abs(float(ll) - ref) / max(abs(ref), 1e-300):.3e}")
        assert abs(float(ll) - ref) <= 2.0 ** -23 * abs(ref)
        assert torch.equal(ll, ld) and torch.equal(gl, gd)
        assert torch.equal(gl, dref1)
        assert bool((gl.view(-1)[ties] == 0).all())
        for target in (y, T):
            l3, g3 = _run(F, x, target, 1.0, squared, 3.0)
            assert torch.equal(l3, ll) and torch.equal(g3, dref3)
        # the torch-ops module path (C = 7 or CPU tensors take it; here called directly)
        tops = torch.relu(1.0 - x * T)
        tops = float((tops.pow(2) if squared else tops).mean())
        assert abs(float(ll) - tops) <= 1e-6 * max(1.0, abs(ref))
        crit = SqrtHingeLoss() if squared else HingeLoss()
        assert torch.equal(crit(x, y), ll) and torch.equal(crit(x, T), ll)


def test_dense_targets_of_any_values(F):
    """t is not only +-1: the reference's input.mul(target) takes any dense target.  Ties at t = 2, x = 0.5."""
    M, C = 1025, 10
    g = torch.Generator(device="cuda").manual_seed(21)
    x = torch.randn(M, C, generator=g, device="cuda") * 3.0
    T = torch.randn(M, C, generator=g, device="cuda")
    x[::100, 3] = 0.5
    T[::100, 3] = 2.0
    for squared in (False, True):
        for margin in (1.0, 0.25):
            ref, dref = _restate(x, T, margin, squared, 3.0)
            loss, grad = _run(F, x, T, margin, squared, 3.0)
            assert abs(float(loss) - ref) <= 2.0 ** -23 * abs(ref)
            assert torch.equal(grad, dref)
            if margin == 1.0:
                assert bool((grad[::100, 3] == 0).all())


def test_deterministic_nan_input_and_label_out_of_range(F):
    M, C = 65536, 10
    x, y, T, _ = _case(M, C, 3)
    for squared in (False, True):
        l1, g1 = _run(F, x, y, 1.0, squared, 1.0)
        l2, g2 = _run(F, x, y, 1.0, squared, 1.0)
        assert torch.equal(l1, l2) and torch.equal(g1, g2) and bool(torch.isfinite(l1))
        xn = x.clone()
        xn[4321, 7] = float("nan")
        assert torch.isnan(F.hinge_loss(xn, y, 1.0, squared)).item()
        assert torch.isnan(F.hinge_loss(xn, T, 1.0, squared)).item()
        # a label equal to C: compared with j only, never an address -- NaN loss, that row's gradient NaN,
        # every other row as without it
        y2 = y.clone()
        y2[123] = C
        lb, gb = _run(F, x, y2, 1.0, squared, 1.0)
        torch.cuda.synchronize()
        assert torch.isnan(lb).item()
        assert bool(torch.isnan(gb[123]).all())
        keep = torch.arange(M, device="cuda") != 123
        assert torch.equal(gb[keep], g1[keep])
    y3 = torch.full((300,), -1, dtype=torch.int64, device="cuda")        # one-workgroup path, negative label
    assert torch.isnan(F.hinge_loss(x[:300].contiguous(), y3)).item()


def test_modules_route_and_fall_back(F):
    from bnn_amd.nn import HingeLoss, SqrtHingeLoss
    x, y, T, _ = _case(300, 10, 9)
    for crit, squared in ((HingeLoss(), False), (SqrtHingeLoss(), True)):
        assert torch.equal(crit(x, y), F.hinge_loss(x, y, 1.0, squared))
        assert torch.equal(crit(x, T), F.hinge_loss(x, T, 1.0, squared))

        def f64(xx, TT, margin):
            h = torch.relu(margin - xx.double() * TT.double())
            return float((h.pow(2) if squared else h).mean())
        # C = 7: the torch path
        q, yq, Tq, _ = _case(300, 7, 9)
        assert not F.hinge_loss_ok(q, yq)
        for target in (yq, Tq):
            assert abs(float(crit(q, target)) - f64(q, Tq, 1.0)) <= 1e-6 * f64(q, Tq, 1.0)
        # a target that requires grad: the torch path, which gives it its gradient
        Tg = T.clone().requires_grad_(True)
        assert not F.hinge_loss_ok(x, Tg)
        loss = crit(x, Tg)
        loss.backward()
        assert abs(float(loss.detach()) - f64(x, T, 1.0)) <= 1e-6 * f64(x, T, 1.0)
        assert Tg.grad is not None and float(Tg.grad.abs().sum()) > 0
        # margin is read at call time, on both paths
        crit.margin = 0.5
        assert torch.equal(crit(x, y), F.hinge_loss(x, y, 0.5, squared))
        assert abs(float(crit(x, y)) - f64(x, T, 0.5)) <= 1e-6 * f64(x, T, 0.5)
        assert abs(float(crit(q, yq)) - f64(q, Tq, 0.5)) <= 1e-6 * f64(q, Tq, 0.5)
        assert abs(f64(x, T, 0.5) - f64(x, T, 1.0)) > 1e-3 * f64(x, T, 1.0)
    with pytest.raises(ValueError):
        F.hinge_loss(q, yq)                                   # functional has no torch fallback


def test_sqrt_hinge_function_on_the_gpu(F):
    from bnn_amd.nn import SqrtHingeLossFunction
    x, y, T, ties = _case(300, 10, 13)
    ref, dref = _restate(x, T, 1.0, True, 3.0)
    a = x.clone().requires_grad_(True)
    loss = SqrtHingeLossFunction.apply(a, T)
    (3.0 * loss).backward()
    assert torch.equal(loss.detach(), F.hinge_loss(x, T, 1.0, True))
    assert torch.equal(a.grad, dref)
    assert bool((a.grad.view(-1)[ties] == 0).all())


def _mlp(nets, widths=(512, 256, 128), **kw):
    torch.manual_seed(0)
    return nets.MLP(*widths, p_drop=0.0, org_protocol=False, mutate_input=False, fused_bn=True, **kw).cuda()


@pytest.mark.parametrize("widths", [(512, 256, 128), (256, 256, 256)])     # the unfused tail, the fused head
def test_mlp_logits_are_the_log_softmax_input(F, widths):
    from bnn_amd import nets
    g = torch.Generator(device="cuda").manual_seed(4)
    u = torch.randint(0, 256, (2048, 1, 28, 28), generator=g, device="cuda").to(torch.uint8)
    a, b = _mlp(nets, widths, log_softmax=False), _mlp(nets, widths)
    assert list(a.state_dict()) == list(b.state_dict())
    for mode in ("train", "eval"):
        getattr(a, mode)()
        getattr(b, mode)()
        with torch.no_grad():
            z, p = a(u), b(u)
        assert torch.equal(torch.log_softmax(z, dim=1), p), mode
        assert not torch.equal(z, p)


def test_cnn_logits_are_the_log_softmax_input(F):
    from bnn_amd import nets
    from bnn_amd.data import synthetic_mnist
    x, _ = synthetic_mnist(256, seed=7, device="cuda", as_u8=False)
    ms = []
    for kw in ({"log_softmax": False}, {}):
        torch.manual_seed(0)
        ms.append(nets.BinCNN(org_protocol=False, mutate_input=False, fused_bn=True, **kw).cuda())
    a, b = ms
    assert list(a.state_dict()) == list(b.state_dict())
    for mode in ("train", "eval"):
        getattr(a, mode)()
        getattr(b, mode)()
        with torch.no_grad():
            z, p = a(x.clone()), b(x.clone())
        assert torch.equal(torch.log_softmax(z, dim=1), p), mode
        assert not torch.equal(z, p)


def test_mlp_step_with_libbnn_sqrt_hinge(F):
    """A fused-MLP training step on the logits with the libbnn squared hinge on the labels against the
    same step with the torch-ops criterion: loss within 1e-6, every parameter gradient within 1e-5
    norm-wise (the project's gradient bar) except fc1 / fc2 / fc3's biases -- ahead of a BatchNorm,
    analytically zero, so a relative bar on them means nothing."""
    from bnn_amd import nets
    from bnn_amd.nn import SqrtHingeLoss
    g = torch.Generator(device="cuda").manual_seed(4)
    u = torch.randint(0, 256, (2048, 1, 28, 28), generator=g, device="cuda").to(torch.uint8)
    y = torch.randint(0, 10, (2048,), generator=g, device="cuda")
    T = _one_vs_all(y, 10)
    ours = SqrtHingeLoss()
    res = []
    for crit in (lambda z: ours(z, y), lambda z: torch.relu(1 - z * T).pow(2).mean()):
        m = _mlp(nets, log_softmax=False).train()
        z = m(u)
        loss = crit(z)
        loss.backward()
        res.append((float(loss), {k: p.grad.detach().clone() for k, p in m.named_parameters()}))
    assert F.hinge_loss_ok(z, y)
    (la, ga), (lb, gb) = res
    assert abs(la - lb) <= 1e-6 * max(1.0, abs(lb))
    skipped = []
    for k in gb:
        if k in ("fc1.bias", "fc2.bias", "fc3.bias"):
            skipped.append(k)
            continue
        err = (ga[k] - gb[k]).norm().item() / max(gb[k].norm().item(), 1e-30)
        print(k, err)
        assert err <= 1e-5, (k, err)
    assert sorted(skipped) == ["fc1.bias", "fc2.bias", "fc3.bias"] and len(gb) - len(skipped) == 11


def test_graph_replays_with_libbnn_sqrt_hinge(F):
    from bnn_amd import nets
    from bnn_amd.graph import GraphedStep
    from bnn_amd.nets import binary_params
    from bnn_amd.nn import SqrtHingeLoss
    from bnn_amd.optim import LatentAdam
    g = torch.Generator(device="cuda").manual_seed(3)
    u = torch.randint(0, 256, (256, 1, 28, 28), generator=g, device="cuda").to(torch.uint8)
    y = torch.randint(0, 10, (256,), generator=g, device="cuda")
    crit = SqrtHingeLoss()
    runs = []
    for graphed in (False, True):
        torch.manual_seed(5)
        m = nets.MLP(256, 128, 64, p_drop=0.3, org_protocol=False, mutate_input=False, fused_bn=True,
                     log_softmax=False).cuda().train()
        torch.manual_seed(99)
        ds = F.DeviceStep().activate()
        try:
            opt = LatentAdam(m.parameters(), lr=0.01, clamp_params=binary_params(m), device_step=ds)

            def step():
                for p in m.parameters():
                    p.grad = None
                loss = crit(m(u), y)
                loss.backward()
                opt.step()
                return loss
            losses = []
            if graphed:
                gs = GraphedStep(step, opt, ds, warmup=2)
                for _ in range(3):
                    losses.append(float(gs().item()))
            else:
                for i in range(5):
                    loss = step()
                    if i >= 2:
                        losses.append(float(loss.item()))
            torch.cuda.synchronize()
            runs.append(({k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}, losses))
        finally:
            ds.deactivate()
    (a, la), (b, lb) = runs
    assert la == lb and all(np.isfinite(la))
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("extra", [[], ["--graph"]])
def test_trainer_runs_with_the_squared_hinge(F, capsys, extra):
    from bnn_amd import trainer
    trainer.main(["--model", "small", "--loss", "sqhinge", "--batch-size", "256", "--dataset-size", "2048",
                  "--epochs", "1", "--max-steps", "4", "--eval", "512"] + extra)
    out = capsys.readouterr().out
    assert any(ln.startswith("Eval 1 : accuracy ") for ln in out.splitlines()), out
    assert "Loss: nan" not in out
