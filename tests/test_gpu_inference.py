"""GPU checks of frozen-model inference (bnn_amd.inference).

* The BN-sign GEMMs (bnn_gemm_fp4_bnsign, bnn_gemm_i8_affine_bnsign) against the pair they replace,
  GEMM + bnn_bn_apply_pack(fmt 1, qt NULL), on the same packed operands: the whole [M][ldq4] buffer
  byte for byte, pad included.  Both tile shapes of each entry run (the 128 x 128 one at the small
  shapes, the 256 x 256 one at a shape past its 512-tile threshold).
* The eval-mode head (functional.bn_hardtanh_linear_eval) and the whole frozen network against the
  existing ``model.eval()`` path, both measured against a float64 evaluation L64 from the exact z3:
  err_new <= max(2 err_old, one fp32 ulp of max|L64|) -- the two differ in fp32 summation order and
  at most an ulp of invstd.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def F():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from bnn_amd import functional
    return functional


def _bn_vectors(z, g):
    """Eval-mode BatchNorm vectors for the columns of z, with rigged columns: 1 has gamma < 0, 2 has
    gamma = beta = 0 (code 0x0 everywhere), 3 has mean = its own z at row 0 and beta = 0 (y == 0)."""
    N = z.shape[1]
    sd = float(z.std()) if z.numel() > 1 else 1.0
    mean = torch.randn(N, generator=g, device="cuda") * 0.3 * sd
    invstd = (torch.rand(N, generator=g, device="cuda") + 0.5) / max(sd, 1e-3)
    gamma = torch.rand(N, generator=g, device="cuda") + 0.5
    beta = torch.randn(N, generator=g, device="cuda") * 0.2
    gamma[1] = -0.75
    gamma[2] = 0.0
    beta[2] = 0.0
    mean[3] = z[0, 3]
    beta[3] = 0.0
    return mean, invstd, gamma, beta


def _apply_pack_ref(F, z, mean, invstd, gamma, beta, ldq4):
    from bnn_amd import _lib as L
    M, N = z.shape
    q = torch.full((M, ldq4), 0xEE, dtype=torch.uint8, device="cuda")
    L.call("bnn_bn_apply_pack", L.ptr(z), M, N, L.ptr(mean), L.ptr(invstd), None, L.ptr(gamma), L.ptr(beta), 1,
           L.ptr(q), ldq4, None, 0, 0, L.stream())
    return q


def _nibble(q, col):
    return (q[:, col // 2] >> (4 * (col % 2))) & 15


def _check_rigged(q, z, mean, invstd, gamma, beta):
    assert int(_nibble(q, 2).max()) == 0                       # gamma = beta = 0: code 0x0
    assert int(_nibble(q, 3)[0]) == 0                          # y exactly zero at row 0
    y1 = ((z[:, 1] - mean[1]) * invstd[1]) * gamma[1] + beta[1]
    far = y1.abs() > 1e-3
    want = torch.where(y1 > 0, 2, 10).to(torch.uint8)          # negative gamma flips the sign
    assert torch.equal(_nibble(q, 1)[far], want[far])


FP4_SHAPES = [(1, 256, 256), (33, 192, 192), (300, 512, 512), (257, 768, 64),
              (8100, 256, 4092)]     # the last: past the 512-tile threshold of the 256 x 256 kernel, ragged both ways


@pytest.mark.parametrize("M,K,N", FP4_SHAPES)
def test_gemm_fp4_bnsign_matches_gemm_then_apply_pack(F, M, K, N):
    g = torch.Generator(device="cuda").manual_seed(M + K + N)
    x = torch.randint(-1, 2, (M, K), generator=g, device="cuda").float()
    w = torch.randint(0, 2, (N, K), generator=g, device="cuda").float() * 2 - 1
    bias = torch.randn(N, generator=g, device="cuda") * 0.5
    A4, _ = F.sign_pack_fp4(x)
    B4, _ = F.sign_pack_fp4(w)
    z = F.gemm_fp4(A4, B4, M, N, bias=bias, k_true=K)
    mean, invstd, gamma, beta = _bn_vectors(z, g)
    ldq4 = F.round_up(N, 256) // 2
    for ga, be in ((gamma, beta), (None, None)):
        want = _apply_pack_ref(F, z, mean, invstd, ga, be, ldq4)
        got = torch.full((M, ldq4), 0x77, dtype=torch.uint8, device="cuda")
        F.gemm_fp4_bnsign(A4, B4, M, N, bias, mean, invstd, ga, be, k_true=K, out=got)
        assert torch.equal(got, want), (M, K, N, ga is None)
    _check_rigged(F.gemm_fp4_bnsign(A4, B4, M, N, bias, mean, invstd, gamma, beta), z, mean, invstd, gamma, beta)
    if M == 33:
        # a row longer than the tiles reach (2 ldq4 = 512 > 256 covered): the rest of the pad is cleared too
        want = _apply_pack_ref(F, z, mean, invstd, gamma, beta, 256)
        got = torch.full((M, 256), 0x77, dtype=torch.uint8, device="cuda")
        F.gemm_fp4_bnsign(A4, B4, M, N, bias, mean, invstd, gamma, beta, out=got)
        assert torch.equal(got, want)
        # no bias
        z0 = F.gemm_fp4(A4, B4, M, N, bias=None, k_true=K)
        want = _apply_pack_ref(F, z0, mean, invstd, gamma, beta, ldq4)
        assert torch.equal(F.gemm_fp4_bnsign(A4, B4, M, N, None, mean, invstd, gamma, beta), want)


I8_SHAPES = [(37, 192), (300, 512), (8100, 4092)]     # the last: the 256 x 256 kernel


@pytest.mark.parametrize("normalize", [None, (0.1307, 0.3081)])
@pytest.mark.parametrize("M,N", I8_SHAPES)
def test_gemm_i8_affine_bnsign_matches_gemm_then_apply_pack(F, M, N, normalize):
    K = 784
    g = torch.Generator(device="cuda").manual_seed(M + N)
    u = torch.randint(0, 256, (M, K), generator=g, device="cuda")
    u = torch.where(torch.rand((M, K), generator=g, device="cuda") < 0.8, torch.zeros_like(u), u).to(torch.uint8)
    w = torch.randint(0, 2, (N, K), generator=g, device="cuda").float() * 2 - 1
    bias = torch.randn(N, generator=g, device="cuda") * 0.5
    q, _ = F.pixels_pack(u)
    wq, _ = F.sign_pack(w)
    R = F.row_sums(wq, K)
    a, s0 = F.pixel_affine(normalize)
    bscale = F._const_vec(a, N, u.device)
    z = F.gemm_i8_affine(q, 1, wq, 1, M, N, b_scale=bscale, bias=bias, col_off=R, off_mul=s0, k_true=K)
    mean, invstd, gamma, beta = _bn_vectors(z, g)
    ldq4 = F.round_up(N, 256) // 2
    for ga, be in ((gamma, beta), (None, None)):
        want = _apply_pack_ref(F, z, mean, invstd, ga, be, ldq4)
        got = torch.full((M, ldq4), 0x77, dtype=torch.uint8, device="cuda")
        F.gemm_i8_affine_bnsign(q, wq, M, N, bscale, bias, R, s0, mean, invstd, ga, be, k_true=K, out=got)
        assert torch.equal(got, want), (M, N, normalize, ga is None)
    _check_rigged(F.gemm_i8_affine_bnsign(q, wq, M, N, bscale, bias, R, s0, mean, invstd, gamma, beta), z, mean,
                  invstd, gamma, beta)


# ----------------------------------------------------------------------------- head
def _ulp32(v):
    return float(np.spacing(np.float32(v)))


def _head_modules(C, seed):
    torch.manual_seed(seed)
    bn = torch.nn.BatchNorm1d(C).cuda()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.2, 0.2)
        bn.running_mean.normal_(0.0, 4.0)
        bn.running_var.uniform_(100.0, 300.0)
    return bn.eval(), torch.nn.Linear(C, 10).cuda()


def _logits64(z, bn, fc):
    """float64 evaluation of bn -> hardtanh -> fc from the exact z."""
    d = torch.float64
    y = (z.to(d) - bn.running_mean.to(d)) / (bn.running_var.to(d) + bn.eps).sqrt() * bn.weight.to(d) + bn.bias.to(d)
    return y.clamp(-1.0, 1.0) @ fc.weight.to(d).t() + fc.bias.to(d)


@pytest.mark.parametrize("C", [256, 192])
def test_eval_head_against_float64(F, C):
    """bn_hardtanh_linear_eval (C = 256: the fused head on running statistics; C = 192: its fallback)
    against the existing eval path (bnn_bn_fwd_eval + F.linear).  Both figures are printed; the
    measured ones are recorded in DESIGN.md §11."""
    M = 300
    g = torch.Generator(device="cuda").manual_seed(C)
    I = torch.randint(-40, 41, (M, C), generator=g, device="cuda")
    bias = torch.randn(C, generator=g, device="cuda") * 0.5
    z = I.float() + bias                                      # an exact z3: integer sums + bias, one rounding
    bn, fc = _head_modules(C, 5)
    L64 = _logits64(z, bn, fc)
    with torch.no_grad():
        old = fc(F.batch_norm_hardtanh(z, bn))
        new = F.bn_hardtanh_linear_eval(z, bn, fc)
    err_old = float((old.double() - L64).abs().max())
    err_new = float((new.double() - L64).abs().max())
    bound = max(2 * err_old, _ulp32(float(L64.abs().max())))
    print(f"eval head C={C}: err_new {err_new:.3e} err_old {err_old:.3e} bound {bound:.3e}")
    assert new.shape == (M, 10) and not new.requires_grad
    assert err_new <= bound, (err_new, err_old, bound)
    if C == 256:
        # the int16 form of the same z (gemm_fp4_i16's output + bias) is the same head bit for bit
        new16 = F.bn_hardtanh_linear_eval((I.to(torch.int16), bias), bn, fc)
        assert torch.equal(new16, new)
    else:
        assert torch.equal(new, old)                          # the fallback is the existing path


# ----------------------------------------------------------------------------- whole net
@pytest.fixture(scope="module")
def trained(F):
    """MLP(256 x 3) and MLP(192 x 3) after 3 training steps on a u8 batch of 300, in eval mode, with
    the existing path's log-probabilities, the frozen model's, and the float64 ones from the exact z3."""
    from bnn_amd import freeze, nets
    from bnn_amd.data import synthetic_mnist
    from bnn_amd.optim import LatentAdam
    out = {}
    u, y = synthetic_mnist(300, seed=11, device="cuda", as_u8=True)
    for h in (256, 192):
        torch.manual_seed(h)
        model = nets.MLP(h, h, h, org_protocol=False, mutate_input=False, fused_bn=True).cuda().train()
        opt = LatentAdam(model.parameters(), lr=0.01, clamp_params=nets.binary_params(model))
        for _ in range(3):
            opt.zero_grad(set_to_none=True)
            torch.nn.functional.nll_loss(model(u), y).backward()
            opt.step()
        model.eval()
        with torch.no_grad():
            old = model(u)
        fz = freeze(model)
        new = fz(u)
        b = fz._buffers(300, u.device)
        z3 = F.gemm_fp4(b["a2"], fz.t["fc3.q4"], 300, h, bias=fz.t["fc3.bias"], k_true=h)
        lp64 = torch.log_softmax(_logits64(z3, model.bn3, model.fc4), dim=1)
        out[h] = {"model": model, "fz": fz, "u": u, "old": old, "new": new.clone(), "lp64": lp64}
    return out


@pytest.mark.parametrize("h", [256, 192])
def test_frozen_net_matches_model_eval(trained, h):
    """Frozen log-probabilities against model.eval()'s with the head's bound, and the labels wherever
    the float64 top-2 margin exceeds it.  Both errors are printed (recorded in DESIGN.md §11)."""
    t = trained[h]
    old, new, lp64 = t["old"], t["new"], t["lp64"]
    assert new.shape == (300, 10) and torch.isfinite(new).all()
    err_old = float((old.double() - lp64).abs().max())
    err_new = float((new.double() - lp64).abs().max())
    bound = max(2 * err_old, _ulp32(float(lp64.abs().max())))
    print(f"frozen net h={h}: err_new {err_new:.3e} err_old {err_old:.3e} bound {bound:.3e}")
    assert err_new <= bound, (err_new, err_old, bound)
    top2 = lp64.topk(2, dim=1).values
    sure = (top2[:, 0] - top2[:, 1]) > bound
    assert int((~sure).sum()) <= 3                       # at most 1 % of the 300 rows are too close to call
    assert torch.equal(t["fz"].predict(t["u"])[sure], old.argmax(1)[sure])
    assert t["fz"].predict(t["u"]).dtype == torch.int64


def test_frozen_two_pass_form_is_bit_identical(trained):
    """The per-layer fall-back (GEMM + bn_apply_pack) gives the same operands, so the same output."""
    t = trained[192]
    fz = t["fz"]
    fz.two_pass = True
    try:
        assert torch.equal(fz(t["u"]), t["new"])
    finally:
        fz.two_pass = False


def test_frozen_mixed_widths_fused_two_pass_refresh_and_state(F):
    """Widths (192, 256, 128) at M = 37: h1 % 128 != 0 puts fc1 on the small BN-sign tile and h3 = 128 is the
    fused head's minimum width.  The fused forward equals its two-pass form bit for bit, hidden signs
    included; refresh() keeps two_pass and the output; a state round trip onto the GPU gives the same bits."""
    from bnn_amd import freeze, inference, nets
    from bnn_amd.data import synthetic_mnist
    torch.manual_seed(7)
    model = nets.MLP(192, 256, 128, org_protocol=False, mutate_input=False, fused_bn=True).cuda().eval()
    g = torch.Generator(device="cuda").manual_seed(8)
    with torch.no_grad():
        for bn, scale in ((model.bn1, 30.0), (model.bn2, 12.0), (model.bn3, 12.0)):
            n = bn.num_features
            bn.running_mean.copy_(torch.randn(n, generator=g, device="cuda") * 0.3 * scale)
            bn.running_var.copy_((torch.rand(n, generator=g, device="cuda") + 0.5) * scale * scale)
            bn.weight.copy_(torch.rand(n, generator=g, device="cuda") + 0.5)
            bn.weight[5] = -0.75
    u, _ = synthetic_mnist(37, seed=12, device="cuda", as_u8=True)
    fz = freeze(model)
    assert F.head_eval_fusable(128, 128, 10) and fz.widths == (192, 256, 128)
    want = fz(u).clone()
    signs = fz.hidden_signs(u)
    assert want.shape == (37, 10) and torch.isfinite(want).all()
    assert [tuple(s.shape) for s in signs] == [(37, 192), (37, 256)] and all((s != 0).any() for s in signs)
    fz.two_pass = True
    assert torch.equal(fz(u), want)
    assert all(torch.equal(a, b) for a, b in zip(fz.hidden_signs(u), signs))
    fz.refresh()
    assert fz.two_pass is True and fz._buf == {} and torch.equal(fz(u), want)
    fz.two_pass = False
    assert torch.equal(fz(u), want)
    again = inference.from_state(fz.state_dict(), device="cuda")
    assert again.device == u.device and torch.equal(again(u), want)
    with pytest.raises(RuntimeError, match=r"FrozenMLP on cpu got an input on cuda:0; call \.to\(device\)"):
        again.to("cpu")(u)


def test_frozen_fp32_images_give_the_same_labels(F, trained):
    t = trained[256]
    x = F.pixels_to_float(t["u"])                        # ToTensor's images of the same pixels
    assert torch.equal(t["fz"].predict(x), t["fz"].predict(t["u"]))
    # floats that are not ToTensor bytes take fc1's digit GEMM + apply-pack.  Scaling the images by
    # 1 + 2^-20 moves z1 (|z1| < 100) by < 1e-4, so a layer-1 sign can differ only where |BN1(z1)| <
    # 1e-4 * invstd * |gamma| -- under 1e-4 of the elements at these statistics; 1e-3 is asserted
    s_u8 = t["fz"].hidden_signs(t["u"])[0]
    xs = x * (1.0 + 2.0 ** -20)
    s_f32 = t["fz"].hidden_signs(xs)[0]
    assert float((s_u8 != s_f32).float().mean()) <= 1e-3
    assert torch.isfinite(t["fz"](xs)).all()


def test_frozen_accuracy_and_reload(trained, tmp_path):
    from bnn_amd.checkpoint import load_frozen, save_frozen
    t = trained[192]
    labels = t["new"].argmax(1)
    assert t["fz"].accuracy(t["u"], labels, batch=128) == 1.0
    path = str(tmp_path / "fz.pt")
    save_frozen(path, t["fz"])
    again = load_frozen(path, map_location="cuda")
    assert torch.equal(again(t["u"]), t["new"])


def test_frozen_forward_captures_in_a_graph(trained):
    t = trained[256]
    fz = t["fz"]
    static_u = t["u"][:64].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fz(static_u)                                      # warm-up: buffers and constants exist
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fz(static_u)
    static_u.copy_(t["u"][100:164])
    graph.replay()
    torch.cuda.synchronize()
    got = out.clone()
    assert torch.equal(got, fz(t["u"][100:164]))


def test_trainer_eval_prints_accuracy(F, capsys):
    from bnn_amd import trainer
    trainer.main(["--model", "small", "--epochs", "1", "--eval", "256", "--dataset-size", "512", "--batch-size", "128",
                  "--log-interval", "100"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Eval 1 : accuracy ")]
    assert len(lines) == 1 and "256 held-out samples" in lines[0]
    assert 0.0 <= float(lines[0].split()[4]) <= 1.0
