"""GPU checks of stochastic binarization, fixed seeds throughout.

1. ``binarize_stochastic`` equals the numpy restatement of the rule (stoch_ref.py) bit for bit.
2. Every packed form equals the deterministic packer applied to (1)'s fp32 result, byte for byte, pads
   included; the 256 x 256-tile forms are reached through ``force`` at small shapes.
3. The fused ``bn_apply_pack_stoch`` (fp32, z16 and s20 inputs) equals (1) applied to the y = bn(z) of
   the deterministic fp32 BatchNorm pass, packed.
4. A stochastic layer in training mode equals the deterministic layer fed the draw; in eval mode it is the
   deterministic layer.
5. Frequencies and cross-seed agreement within 5 binomial sigma.
6. A captured forward under a DeviceStep draws afresh per replay.
7. The nets train; the frozen model and ``model.eval()`` stay deterministic and agree.
"""
import copy

import numpy as np
import pytest
import torch

import stoch_ref as R

pytestmark = pytest.mark.gpu

PLANTED = [0.0, 1.0, -1.0, -0.0, np.nan, np.inf, -np.inf, 1.0 - 2.0 ** -24, -1.0 + 2.0 ** -23]
SHAPES = [(1, 1), (3, 70), (65, 192), (256, 256), (512, 256)]


@pytest.fixture(scope="module")
def F():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from bnn_amd import functional
    return functional


def host(t):
    return t.detach().cpu().numpy()


def eq(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


def eqp(a, b, K):
    """eq for FP4 transposes in the panel layout ([ceil(K/512)][ldqt/32][512][32 B]): the slots of rows
    beyond K are unspecified (bnn.h), every other byte must agree."""
    if not (a.shape == b.shape and a.dtype == b.dtype):
        return False
    P = a.shape[0] // 512
    av, bv = a.reshape(P, -1, 512, 32), b.reshape(P, -1, 512, 32)
    return all(torch.equal(av[p, :, :min(512, K - 512 * p)], bv[p, :, :min(512, K - 512 * p)]) for p in range(P))


def eqt(a, b, K, qt_fmt):
    return eqp(a, b, K) if qt_fmt in ("fp4p", 2) else eq(a, b)


def _input(shape, seed):
    """Uniform in [-1.3, 1.3] with the special values planted at spread positions (where they fit)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.3, 1.3, shape).astype(np.float32)
    flat = x.reshape(-1)
    if flat.size >= 4 * len(PLANTED):
        for rep in range(3):
            pos = rng.choice(flat.size, len(PLANTED), replace=False)
            flat[pos] = np.array(PLANTED, np.float32)
    return x


@pytest.fixture(scope="module")
def drawn(F):
    """(x on the GPU, seed, binarize_stochastic(x, seed)) per shape: computed once, never modified."""
    out = {}
    for i, shape in enumerate(SHAPES + [(300, 256)]):
        x = torch.from_numpy(_input(shape, 100 + i)).cuda()
        seed = (0x1234567 * (i + 1)) ^ (1 << (40 + i))
        out[shape] = (x, seed, F.binarize_stochastic(x, seed))
    return out


# ------------------------------------------------------------------ 1. exact draw
@pytest.mark.parametrize("shape", SHAPES)
def test_binarize_stochastic_equals_the_restatement(F, drawn, shape):
    x, seed, s = drawn[shape]
    want = R.binarize(host(x), seed)
    got = host(s)
    assert got.dtype == np.float32 and np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(got == 0, np.isnan(host(x)))
    y = x.clone()
    r = F.binarize_stochastic(y, seed, out=y)                   # aliased output
    assert r is y and eq(y, s)


def test_binarize_stochastic_special_values_and_seeds(F):
    for v in PLANTED:
        x = torch.full((1, 1), float(v), device="cuda")
        for seed in (0, 1, 2 ** 64 - 1, 2 ** 63 + 977):
            assert np.array_equal(host(F.binarize_stochastic(x, seed)), R.binarize(host(x), seed)), (v, seed)
    # an unaligned buffer (the scalar path) and a 1-D / 4-D view: the element index is the flat index
    base = torch.from_numpy(_input((1, 4099), 7)).cuda().reshape(-1)
    x = base[1:4098]
    assert x.data_ptr() % 16 != 0
    assert np.array_equal(host(F.binarize_stochastic(x, 5)), R.binarize(host(x), 5))
    x4 = base[:4096].reshape(4, 4, 16, 16)
    assert np.array_equal(host(F.binarize_stochastic(x4, 5)), R.binarize(host(x4), 5))


# ------------------------------------------------------------------ 2. all forms agree
@pytest.mark.parametrize("shape", SHAPES + [(300, 256)])
def test_packed_forms_equal_the_deterministic_packers_of_the_draw(F, drawn, shape):
    x, seed, s = drawn[shape]
    M, K = shape
    for want_q, want_qt in ((True, True), (True, False), (False, True)):
        a, b = F.stoch_pack(x, seed, want_q=want_q, want_qt=want_qt), F.sign_pack(s, want_q=want_q, want_qt=want_qt)
        assert (a[0] is None) == (not want_q) and (a[1] is None) == (not want_qt)
        assert all(u is None or eq(u, v) for u, v in zip(a, b)), ("i8", want_q, want_qt)
    forces = (False, True) if K % 256 == 0 else (False,)
    for qt_fmt in ("i8", "fp4", "fp4p"):
        want = F.sign_pack_fp4(s, want_qt=True, qt_fmt=qt_fmt)
        for force in forces:                                     # True: the 256 x 256-tile kernel (FP4 transposes)
            got = F.stoch_pack_fp4(x, seed, want_qt=True, qt_fmt=qt_fmt, force=force)
            assert eq(got[0], want[0]) and eqt(got[1], want[1], K, qt_fmt), (qt_fmt, force)
    assert eq(F.stoch_pack_fp4(x, seed)[0], want[0])                                        # rows only
    assert eq(F.stoch_pack_fp4(x, seed, want_qt=True, qt_fmt="fp4", want_q=False)[1],
              F.sign_pack_fp4(s, want_qt=True, qt_fmt="fp4", want_q=False)[1])              # transpose only
    q4, qt = F.sign_pack_fp4(s, want_qt=True, qt_fmt="fp4p")
    for force in forces:                                         # True: one kernel with the fp32 write-back
        so, a4, at = F.stoch_pack_fp4_writeback(x, seed, want_qt=True, force=force)
        assert eq(so, s) and eq(a4, q4) and eqp(at, qt, K), force
    so, a4, at = F.stoch_pack_fp4_writeback(x, seed, want_qt=False)
    assert eq(so, s) and eq(a4, q4) and at is None


@pytest.mark.parametrize("force", [0, 1])
def test_writeback_into_the_input_itself(F, drawn, force):
    """sout == x (the drop-in's input.data write-back may reuse the buffer): same three results."""
    from bnn_amd import _lib as L
    x, seed, s = drawn[(512, 256)]
    M, K = x.shape
    q4w, qtw = F.sign_pack_fp4(s, want_qt=True, qt_fmt="fp4p")
    y = x.clone()
    q4 = torch.full_like(q4w, 0x55)
    qt = F._qt_buffer(K, M, "fp4p", "cuda")
    L.call("bnn_stoch_pack_fp4_out", L.ptr(y), M, K, L.ptr(q4), q4.shape[1], L.ptr(qt), qt.shape[1], 2, L.ptr(y),
           seed, force, L.stream())
    assert eq(y, s) and eq(q4, q4w) and eqp(qt, qtw, K)


# ------------------------------------------------------------------ 3. fused apply-pack
def _bn_fp32(F, z, gam, bet):
    """The deterministic fp32 BatchNorm pass: batch statistics and y = bn(z) (no Hardtanh)."""
    from bnn_amd import _lib as L
    M, C = z.shape
    mean, invstd, lo = (torch.empty(C, device="cuda") for _ in range(3))
    y = torch.empty_like(z)
    ws = torch.empty((L.lib().bnn_bn_workspace(M, C),), dtype=torch.uint8, device="cuda")
    L.call("bnn_bn_fwd_train", L.ptr(z), M, C, L.ptr(gam), L.ptr(bet), None, None, -1.0, 1e-5, L.ptr(mean),
           L.ptr(invstd), L.ptr(lo), L.ptr(y), 0, L.ptr(ws), L.stream())
    return mean, invstd, lo, y


def _affine(C, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    gam = torch.rand(C, generator=g, device="cuda") * 0.8 + 0.3           # y ~ N(0, 0.3 .. 1.1): both regimes
    gam[1] = -0.6
    bet = torch.randn(C, generator=g, device="cuda") * 0.2
    return gam, bet


@pytest.mark.parametrize("M,C", [(65, 192), (256, 256)])
def test_bn_apply_pack_stoch_fp32_equals_the_draw_of_bn(F, M, C):
    from bnn_amd import _lib as L
    g = torch.Generator(device="cuda").manual_seed(M + C)
    z = torch.randint(-30, 31, (M, C), generator=g, device="cuda").float() + torch.randn(C, generator=g, device="cuda")
    gam, bet = _affine(C, 3)
    mean, invstd, lo, y = _bn_fp32(F, z, gam, bet)
    seed = 0xABCDEF0123 + M
    s = F.binarize_stochastic(y, seed)
    assert float((s != torch.sign(y)).float().mean()) > 0.02               # the draw is not the sign
    for ga, be, mlo in ((gam, bet, lo), (None, None, None)):
        if ga is None:                                                     # no affine part, no mean remainder
            s = F.binarize_stochastic(_plain_bn(z, mean, invstd), seed)
        cases = [(0, 0), (1, 0), (1, 1), (1, 2)]                           # (fmt, qt_fmt)
        for fmt, qf in cases:
            name = {0: "i8", 1: "fp4", 2: "fp4p"}[qf]
            if fmt == 0:
                want = F.sign_pack(s, want_q=True, want_qt=True)
            else:
                want = F.sign_pack_fp4(s, want_qt=True, qt_fmt=name)
            for force in ((0, 1) if (C % 256 == 0 and fmt == 1 and qf >= 1) else (0,)):
                q = torch.full_like(want[0], 0x55)
                qt = F._qt_buffer(C, M, name, "cuda")
                L.call("bnn_bn_apply_pack_stoch", L.ptr(z), M, C, L.ptr(mean), L.ptr(invstd), L.ptr(mlo), L.ptr(ga),
                       L.ptr(be), fmt, L.ptr(q), q.shape[1], L.ptr(qt), qt.shape[1], qf, seed, force, L.stream())
                assert eq(q, want[0]) and eqt(qt, want[1], C, qf), (fmt, qf, force, ga is None)
        # rows only (qt NULL)
        want = F.sign_pack_fp4(s)[0]
        q = torch.full_like(want, 0x55)
        L.call("bnn_bn_apply_pack_stoch", L.ptr(z), M, C, L.ptr(mean), L.ptr(invstd), L.ptr(mlo), L.ptr(ga), L.ptr(be),
               1, L.ptr(q), q.shape[1], None, 0, 0, seed, 0, L.stream())
        assert eq(q, want)


def _plain_bn(z, mean, invstd):
    """y = (z - mean) * invstd with no affine part and no mean remainder, each step rounded to fp32 --
    bn_y1 with lo = 0, gamma = 1, beta = 0 (fmaf(xh, 1, 0) = xh)."""
    return (z - mean) * invstd


@pytest.mark.parametrize("M", [65, 256])
@pytest.mark.parametrize("panel", [0, 1])
def test_bn_apply_pack_stoch_compact_inputs_equal_the_fp32_form(F, M, panel):
    """z16 (int16 sums + bias) and s20 (20-bit sums, scale, bias) inputs: the same draw as from the fp32 z
    they stand for, hence (previous test) as binarize_stochastic(bn(z))."""
    from bnn_amd import _lib as L
    C = 256
    g = torch.Generator(device="cuda").manual_seed(M + panel)
    gam, bet = _affine(C, 4)
    bias = torch.randn(C, generator=g, device="cuda") * 0.5
    seed = 0x5EED0000 + M
    name = "fp4p" if panel else "fp4"
    # z16
    I = torch.randint(-200, 201, (M, C), generator=g, device="cuda")
    I16 = I.to(torch.int16).contiguous()
    # s20: S in (-2^19, 2^19), low 16 bits + nibble plane (column 2j in the low nibble of byte j)
    S = torch.randint(-(1 << 19) + 1, 1 << 19, (M, C), generator=g, device="cuda")
    S[0, :8] = torch.tensor([0, 1, -1, (1 << 19) - 1, -(1 << 19) + 1, 65535, 65536, -65536], device="cuda")
    scale = float(np.float32(1.0 / 255.0))
    forms = {"z16": I.float() + bias, "s20": (S.float() * scale) + bias}
    for form, z in forms.items():
        z = z.contiguous()
        mean, invstd, lo, y = _bn_fp32(F, z, gam, bet)
        s = F.binarize_stochastic(y, seed)
        want = F.sign_pack_fp4(s, want_qt=True, qt_fmt=name)
        q = torch.full_like(want[0], 0x55)
        qt = F._qt_buffer(C, M, name, "cuda")
        if form == "z16":
            L.call("bnn_bn_apply_pack_stoch_i16", L.ptr(I16), L.ptr(bias), M, C, L.ptr(mean),
                   L.ptr(invstd), L.ptr(lo), L.ptr(gam), L.ptr(bet), L.ptr(q), q.shape[1], L.ptr(qt), qt.shape[1],
                   panel, seed, L.stream())
        else:
            lo16 = (S & 0xFFFF).to(torch.int32)
            lo16 = torch.where(lo16 >= 32768, lo16 - 65536, lo16).to(torch.int16).contiguous()
            nib = ((S >> 16) & 15).to(torch.uint8)
            hi = (nib[:, 0::2] | (nib[:, 1::2] << 4)).contiguous()
            L.call("bnn_bn_apply_pack_stoch_s20", L.ptr(lo16), L.ptr(hi), L.ptr(bias), scale, M, C, L.ptr(mean),
                   L.ptr(invstd), L.ptr(lo), L.ptr(gam), L.ptr(bet), L.ptr(q), q.shape[1], L.ptr(qt), qt.shape[1],
                   panel, seed, L.stream())
        assert eq(q, want[0]) and eqt(qt, want[1], C, name), form


# ------------------------------------------------------------------ 4. layer equivalence
def _seed_of(F, salt, k):
    """The seed a layer with this salt draws right after torch.manual_seed(k)."""
    torch.manual_seed(k)
    seed = F.stochastic_seed(salt)
    torch.manual_seed(k)
    return seed


@pytest.mark.parametrize("backend", ["fp4", "mfma", "xnor"])
@pytest.mark.parametrize("dropin", [True, False])
def test_stochastic_linear_equals_the_deterministic_layer_fed_the_draw(F, backend, dropin):
    from bnn_amd.nn import BinarizeLinear
    torch.manual_seed(3)
    a = BinarizeLinear(192, 192).cuda().train()
    a.backend, a.org_protocol, a.mutate_input = backend, dropin, dropin
    a.quant_mode, a.stoch_salt = "stoch", 5
    b = copy.deepcopy(a)
    b.quant_mode = "det"
    g = torch.Generator(device="cuda").manual_seed(4)
    h0 = torch.rand(64, 192, generator=g, device="cuda") * 2.6 - 1.3
    dy = torch.randn(64, 192, generator=g, device="cuda")
    S = _seed_of(F, 5, 21)
    hs = F.binarize_stochastic(h0, S)
    assert float((hs != torch.sign(h0)).float().mean()) > 0.05
    h = h0.clone().requires_grad_(True)
    ya = a(h)
    ya.backward(dy)
    hb = hs.clone().requires_grad_(True)
    yb = b(hb)
    yb.backward(dy)
    assert eq(ya, yb)
    assert eq(a.weight.grad, b.weight.grad) and eq(a.bias.grad, b.bias.grad) and eq(h.grad, hb.grad)
    if dropin:
        assert eq(h.data, hs)                                     # the input write-back holds the draw
    else:
        assert eq(h.data, h0)
    # a second training forward draws another mask; eval mode is the deterministic layer
    assert not eq(a(h0.clone()), ya)
    a.eval(), b.eval()
    assert eq(a(h0.clone()), b(h0.clone()))


@pytest.mark.parametrize("backend", ["fp4", "mfma"])
def test_fused_stochastic_op_equals_the_unfused_layers(F, backend):
    from bnn_amd.nn import BinarizeLinear
    torch.manual_seed(5)
    fc = BinarizeLinear(192, 192).cuda().train()
    fc.backend, fc.org_protocol, fc.mutate_input = backend, False, False
    bn = torch.nn.BatchNorm1d(192).cuda().train()
    with torch.no_grad():
        bn.weight.uniform_(0.3, 1.1)
        bn.bias.normal_(0.0, 0.2)
    fc2, bn2 = copy.deepcopy(fc), copy.deepcopy(bn)
    g = torch.Generator(device="cuda").manual_seed(6)
    z0 = torch.randint(-30, 31, (64, 192), generator=g, device="cuda").float() + torch.randn(192, generator=g,
                                                                                             device="cuda")
    dy = torch.randn(64, 192, generator=g, device="cuda")
    S = 0x0DDBA11 << 20
    z = z0.clone().requires_grad_(True)
    ya = F.bn_hardtanh_binary_linear(z, bn, fc, backend, stochastic=S)
    ya.backward(dy)
    zb = z0.clone().requires_grad_(True)
    hb = F.batch_norm_hardtanh(zb, bn2)                           # hardtanh(bn(z)) in fp32
    yb = F.binary_linear(hb, fc2.weight, fc2.bias, True, backend, cache=True, stochastic=S)
    yb.backward(dy)
    yd = F.bn_hardtanh_binary_linear(z0.clone(), copy.deepcopy(bn2), fc2, backend)
    assert not eq(ya.detach(), yd.detach())                       # the draw differs from the deterministic op
    assert eq(ya, yb)
    for u, v in ((z.grad, zb.grad), (bn.weight.grad, bn2.weight.grad), (bn.bias.grad, bn2.bias.grad),
                 (fc.weight.grad, fc2.weight.grad), (fc.bias.grad, fc2.bias.grad)):
        assert eq(u, v)
    assert eq(bn.running_mean, bn2.running_mean) and eq(bn.running_var, bn2.running_var)


@pytest.mark.parametrize("mutate", [True, False])
def test_stochastic_conv_equals_the_deterministic_layer_fed_the_draw(F, mutate):
    from bnn_amd.nn import BinarizeConv2d
    torch.manual_seed(7)
    a = BinarizeConv2d(16, 32, kernel_size=5, stride=1, padding=2).cuda().train()
    a.org_protocol, a.mutate_input = mutate, mutate
    a.quant_mode, a.stoch_salt = "stoch", 2
    b = copy.deepcopy(a)
    b.quant_mode = "det"
    g = torch.Generator(device="cuda").manual_seed(8)
    x0 = torch.rand(8, 16, 14, 14, generator=g, device="cuda") * 2.6 - 1.3
    dy = torch.randn(8, 32, 14, 14, generator=g, device="cuda")
    S = _seed_of(F, 2, 33)
    xs = F.binarize_stochastic(x0, S)
    x = x0.clone().requires_grad_(True)
    ya = a(x)
    ya.backward(dy)
    xb = xs.clone().requires_grad_(True)
    yb = b(xb)
    yb.backward(dy)
    assert eq(ya, yb) and eq(a.weight.grad, b.weight.grad) and eq(a.bias.grad, b.bias.grad) and eq(x.grad, xb.grad)
    assert eq(x.data, xs if mutate else x0)
    a.eval(), b.eval()
    assert eq(a(x0.clone()), b(x0.clone()))


def test_binarize_stoch_on_a_cuda_tensor_runs_in_place(F):
    from bnn_amd.nn import Binarize
    g = torch.Generator(device="cuda").manual_seed(9)
    t0 = torch.rand(65, 192, generator=g, device="cuda") * 2.6 - 1.3
    S = _seed_of(F, 1, 44)
    t = t0.clone()
    r = Binarize(t, "stoch")
    assert r is t and eq(t, F.binarize_stochastic(t0, S))


# ------------------------------------------------------------------ 5. statistics
N_STAT = 1 << 16


@pytest.mark.parametrize("c", [-0.75, 0.0, 0.25, 0.9])
def test_frequency_within_five_sigma(F, c):
    x = torch.full((256, 256), c, device="cuda")
    p = float(R.threshold(np.float32(c))) / 2 ** 24
    assert abs(p - (c + 1) / 2) <= 2.0 ** -24
    frac = float((F.binarize_stochastic(x, 0xC0FFEE) > 0).double().mean())
    sigma = np.sqrt(p * (1 - p) / N_STAT)
    print(f"c={c}: +1 fraction {frac:.5f}, p {p:.5f}, {abs(frac - p) / sigma:.2f} sigma")
    assert abs(frac - p) <= 5 * sigma


def test_salts_and_counter_values_give_unrelated_masks(F):
    z = torch.zeros((256, 256), device="cuda")
    bound = 5 / (2 * np.sqrt(N_STAT))
    base = 0x1DEA5EED
    a = F.binarize_stochastic(z, R.site_seed(base, 2))
    b = F.binarize_stochastic(z, R.site_seed(base, 3))
    agree = float((a == b).double().mean())
    print(f"two salts agree on {agree:.5f}")
    assert abs(agree - 0.5) <= bound
    ds = F.DeviceStep("cuda").activate()
    try:
        m0 = F.binarize_stochastic(z, base)
        ds.advance()
        m1 = F.binarize_stochastic(z, base)
        torch.cuda.synchronize()
    finally:
        ds.deactivate()
    agree = float((m0 == m1).double().mean())
    print(f"two counter values agree on {agree:.5f}")
    assert abs(agree - 0.5) <= bound
    assert np.array_equal(host(m0), R.binarize(host(z), base, ctr=0))
    assert np.array_equal(host(m1), R.binarize(host(z), base, ctr=1))


# ------------------------------------------------------------------ 6. graph
def test_captured_forward_draws_afresh_per_replay(F, drawn):
    x, _, _ = drawn[(65, 192)]
    ds = F.DeviceStep("cuda").activate()
    try:
        seed = F.stochastic_seed(2)
        assert seed == R.site_seed(ds.base_seed, 2)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            F.binarize_stochastic(x, seed)
            F.stoch_pack(x, seed)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            s = F.binarize_stochastic(x, seed)
            q = F.stoch_pack(x, seed)[0]
        masks = []
        for _ in range(2):
            graph.replay()
            masks.append((s.clone(), q.clone()))
            ds.advance()
        torch.cuda.synchronize()
    finally:
        ds.deactivate()
    assert not eq(masks[0][0], masks[1][0])
    for ctr, (m, q) in enumerate(masks):
        assert np.array_equal(host(m), R.binarize(host(x), seed, ctr=ctr)), ctr
        assert eq(q, F.sign_pack(m)[0])


# ------------------------------------------------------------------ 7. nets
def test_small_net_trains_and_freezes_deterministically(F):
    from bnn_amd import freeze, nets
    from bnn_amd.data import synthetic_mnist
    from bnn_amd.optim import LatentAdam
    torch.manual_seed(0)
    kw = dict(p_drop=0, org_protocol=False, mutate_input=False, fused_bn=True)
    model = nets.SmallNet(stochastic=True, **kw).cuda().train()
    u, y = synthetic_mnist(4096, device="cuda", as_u8=True)
    opt = LatentAdam(model.parameters(), lr=0.01, clamp_params=nets.binary_params(model))
    losses = []
    for step in range(40):
        lo = (step % 16) * 256
        opt.zero_grad(set_to_none=True)
        loss = torch.nn.functional.nll_loss(model(u[lo:lo + 256]), y[lo:lo + 256])
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    losses = torch.stack(losses).cpu()
    print("stochastic SmallNet losses: first 4", losses[:4].tolist(), "last 4", losses[-4:].tolist())
    assert torch.isfinite(losses).all()
    assert float(losses[-4:].mean()) < float(losses[:4].mean())
    # training forwards draw (two differ); eval and the frozen model are deterministic and agree bit for bit
    with torch.no_grad():
        assert not eq(model(u[:300]), model(u[:300]))
        model.eval()
        old = model(u[:300])
        assert eq(model(u[:300]), old)
    twin = nets.SmallNet(**kw).cuda()
    twin.load_state_dict(model.state_dict())
    twin.eval()
    with torch.no_grad():
        assert eq(twin(u[:300]), old)                             # the deterministic net with these weights
    new = freeze(model)(u[:300])
    print("frozen vs eval: max |diff|", float((new - old).abs().max()))
    assert eq(new, freeze(twin)(u[:300]))
    assert eq(new, old)


def test_compact_handoffs_carry_the_same_draw(F, monkeypatch):
    """MLP(256 x 3) on u8 pixels: fc2's stochastic operand is drawn from the s20 form of z1 and fc3's from
    the z16 form of z2 (its tile threshold lowered through the module's constant); with both hand-offs off the
    same seeds give the same loss bit for bit."""
    from bnn_amd import nets
    from bnn_amd.data import synthetic_mnist
    u, y = synthetic_mnist(64, seed=3, device="cuda", as_u8=True)
    torch.manual_seed(1)
    model = nets.MLP(256, 256, 256, p_drop=0, org_protocol=False, mutate_input=False, fused_bn=True,
                     stochastic=True).cuda().train()
    state = copy.deepcopy(model.state_dict())
    monkeypatch.setattr(F, "Z16_MIN_TILES", 1)
    out = []
    for compact in (True, False):
        monkeypatch.setattr(F, "Z16", compact)
        monkeypatch.setattr(F, "S20", compact)
        model.load_state_dict(state)
        n16, n20 = F.Z16_HANDOFFS, F.S20_HANDOFFS
        torch.manual_seed(2)
        for p in model.parameters():
            p.grad = None
        loss = torch.nn.functional.nll_loss(model(u), y)
        loss.backward()
        assert (F.Z16_HANDOFFS > n16) == compact and (F.S20_HANDOFFS > n20) == compact
        grads = [p.grad.clone() for p in model.parameters()]
        assert all(torch.isfinite(gr).all() for gr in grads)
        out.append(loss.detach().clone())
    assert eq(out[0], out[1])


def test_bincnn_takes_a_stochastic_training_step(F):
    from bnn_amd import nets
    from bnn_amd.data import synthetic_mnist
    from bnn_amd.optim import LatentAdam
    torch.manual_seed(2)
    model = nets.BinCNN(org_protocol=False, mutate_input=False, fused_bn=True, stochastic=True).cuda().train()
    x, y = synthetic_mnist(64, seed=9, device="cuda")
    opt = LatentAdam(model.parameters(), lr=0.01, clamp_params=nets.binary_params(model))
    opt.zero_grad(set_to_none=True)
    out = model(x)
    loss = torch.nn.functional.nll_loss(out, y)
    loss.backward()
    for name, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
    assert float(model.layer2[0].weight.grad.abs().sum()) > 0
    opt.step()
    with torch.no_grad():
        assert not eq(model(x), out.detach())                     # another draw (and another weight)
        model.eval()
        assert eq(model(x), model(x))
