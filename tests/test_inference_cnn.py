"""Frozen BinCNN inference without a GPU: the snapshot of bnn_amd.inference.freeze(BinCNN) and its
plain-torch forward against a restatement of ``model.eval()`` written here (BinCNN itself has no CPU
forward), the weight packs, the pixel sign table, the state round-trips and the argument checks of the
new C entries."""
import ctypes

import pytest
import torch
import torch.nn.functional as tF

from bnn_amd import functional as BF
from bnn_amd import nets

NORM = (0.1307, 0.3081)


def _model(seed=0):
    torch.manual_seed(seed)
    m = nets.BinCNN(org_protocol=False, mutate_input=False)
    g = torch.Generator().manual_seed(seed + 1)
    for bn, scale in ((m.layer1[1], 3.0), (m.layer2[1], 14.0)):
        n = bn.num_features
        bn.running_mean.copy_(torch.randn(n, generator=g) * 0.3 * scale)
        bn.running_var.copy_((torch.rand(n, generator=g) + 0.5) * scale * scale)
        with torch.no_grad():
            bn.weight.copy_(torch.rand(n, generator=g) + 0.5)
            bn.bias.copy_(torch.randn(n, generator=g) * 0.2)
    with torch.no_grad():
        m.layer1[1].weight[5] = -0.75          # one negative gamma per BatchNorm
        m.layer2[1].weight[17] = -1.25
    return m.eval()


def _pixels(n, seed=3):
    g = torch.Generator().manual_seed(seed)
    u = torch.randint(0, 256, (n, 1, 28, 28), generator=g)
    return torch.where(torch.rand((n, 1, 28, 28), generator=g) < 0.8, torch.zeros_like(u), u).to(torch.uint8)


def _eval_restated(m, x, dtype):
    """model.eval() in plain torch: F.conv2d on signs, F.batch_norm on the running statistics, hardtanh,
    max_pool2d, linear -- evaluated in ``dtype`` -- and layer 1's pooled output."""
    h = x.to(dtype)
    pooled = []
    for seq in (m.layer1, m.layer2):
        conv, bn = seq[0], seq[1]
        z = tF.conv2d(h.sign(), conv.weight.detach().sign().to(dtype), conv.bias.detach().to(dtype), 1, conv.padding)
        y = tF.batch_norm(z, bn.running_mean.to(dtype), bn.running_var.to(dtype), bn.weight.detach().to(dtype),
                          bn.bias.detach().to(dtype), False, 0.0, bn.eps)
        h = tF.max_pool2d(tF.hardtanh(y), 2, 2)
        pooled.append(h)
    logits = tF.linear(h.reshape(h.shape[0], -1), m.fc.weight.detach().to(dtype), m.fc.bias.detach().to(dtype))
    return tF.log_softmax(logits, dim=1), pooled[0]


@pytest.mark.parametrize("normalize", [None, NORM])
def test_frozen_cnn_cpu_forward_matches_the_restated_eval(normalize):
    from bnn_amd import FrozenCNN, freeze
    m = _model()
    u = _pixels(41)
    fz = freeze(m, normalize=normalize)
    assert isinstance(fz, FrozenCNN)
    logp = fz.forward(u)
    ref, pooled1 = _eval_restated(m, BF.pixels_to_float(u, normalize), torch.float64)
    assert logp.shape == (41, 10) and logp.dtype == torch.float32
    # float32 bound: the classifier sums 1568 products of |f| <= 1 in fp32 (the hidden layers are exact
    # integer sums and signs); 2^-24 * 1568 * max|w| * a few, far below the 1e-4 used for the MLP's head
    assert float((logp.double() - ref).abs().max()) < 1e-4
    top2 = ref.topk(2, dim=1).values
    sure = (top2[:, 0] - top2[:, 1]) > 1e-4
    assert int(sure.sum()) >= 38
    assert torch.equal(logp.argmax(1)[sure], ref.argmax(1)[sure])
    assert torch.equal(fz.predict(u), logp.argmax(1))
    hs = fz.hidden_signs(u)
    assert hs.shape == (41, 16, 14, 14) and hs.dtype == torch.int8
    far = pooled1.abs() > 1e-9
    assert torch.equal(hs.double()[far], pooled1.sign()[far])
    assert torch.equal(fz.forward(u.reshape(41, 784)), logp)
    # fp32 images of the same bytes binarise to the same signs
    assert torch.equal(fz.forward(BF.pixels_to_float(u, normalize)), logp)


def test_weight_packs_unpack_to_tsign_with_zero_pads():
    from bnn_amd import inference as I
    g = torch.Generator().manual_seed(5)
    for Co, C, K in ((32, 16, 5), (20, 32, 5), (48, 16, 3)):
        w = torch.randn(Co, C, K, K, generator=g)
        w[0, 0, 0, 0] = 0.0
        w[1, 2, 1, 1] = float("nan")
        q = I._pack_conv_rows(w)
        kc = K * K * C // 16
        assert q.dtype == torch.int8 and q.shape == ((Co + 15) // 16 * 16, (kc + 3) // 4 * 4 * 16)
        assert torch.equal(I._unpack_conv_rows(q, Co, C, K, K), I._tsign(w))
        assert int(q[Co:].abs().sum()) == 0 and int(q[:, K * K * C:].abs().sum()) == 0
        # K order (tap, channel): byte (kh K + kw) C + c
        assert int(q[3, (1 * K + 2) * C + 7]) == int(I._tsign(w)[3, 7, 1, 2])
    for Co, K in ((16, 5), (8, 3), (20, 5)):
        w = torch.randn(Co, 1, K, K, generator=g)
        w[0, 0, 0, 0] = 0.0
        q = I._pack_conv_c1(w)
        CO = 8 if Co <= 8 else 16 if Co <= 16 else 32
        assert q.dtype == torch.int8 and q.shape == (K, 1 if K <= 4 else 2, CO, 4)
        assert torch.equal(I._unpack_conv_c1(q, Co, K), I._tsign(w))
        assert int(q[:, :, Co:].abs().sum()) == 0
        flat = q.permute(0, 1, 3, 2).reshape(K, -1, CO)
        assert int(flat[:, K:].abs().sum()) == 0
        assert int(q[2, 0, 3, 1]) == int(I._tsign(w)[3, 0, 2, 1])


@pytest.mark.parametrize("normalize", [None, NORM])
def test_pixel_table_is_the_sign_of_the_float_pipeline(normalize):
    from bnn_amd import freeze
    table = freeze(_model(), normalize=normalize).t["pixel.table"]
    x = torch.arange(256).float() / 255
    if normalize is not None:
        x = (x - normalize[0]) / normalize[1]
    assert table.dtype == torch.int8 and table.shape == (256,)
    assert torch.equal(table.float(), x.sign())
    assert int(table[0]) == (0 if normalize is None else -1)


def test_invstd_is_the_kernels_double_expression():
    from bnn_amd import freeze
    m = _model()
    fz = freeze(m)
    for i, bn in ((1, m.layer1[1]), (2, m.layer2[1])):
        eps32 = float(torch.tensor(bn.eps, dtype=torch.float32))
        want = torch.tensor([float(1.0 / (float(v) + eps32) ** 0.5) for v in bn.running_var.double()]).float()
        assert torch.equal(fz.t[f"bn{i}.invstd"], want)


def test_frozen_cnn_state_round_trips(tmp_path):
    from bnn_amd import FrozenCNN, FrozenMLP, freeze
    from bnn_amd.checkpoint import load_frozen, save_frozen
    m = _model(seed=4)
    u = _pixels(19, seed=8)
    fz = freeze(m, normalize=NORM)
    want = fz.forward(u)
    again = FrozenCNN.from_state(fz.state_dict())
    assert again.normalize == NORM and again.layers == [(1, 16, 5, 5, 2), (16, 32, 5, 5, 2)]
    assert torch.equal(again.forward(u), want)
    path = str(tmp_path / "frozen_cnn.pt")
    save_frozen(path, fz)
    assert torch.load(path, weights_only=True)["format"] == "bnn_amd.frozen_cnn/1"
    del m
    loaded = load_frozen(path)
    assert isinstance(loaded, FrozenCNN)
    assert torch.equal(loaded.forward(u), want)
    with pytest.raises(RuntimeError, match="refresh"):
        loaded.refresh()
    with pytest.raises(ValueError, match="frozen_cnn"):
        FrozenCNN.from_state({"format": "bnn_amd.frozen/1"})
    # a FrozenMLP file still loads as a FrozenMLP
    torch.manual_seed(1)
    mlp = nets.MLP(64, 64, 64, org_protocol=False, mutate_input=False).eval()
    fm = freeze(mlp)
    p2 = str(tmp_path / "frozen_mlp.pt")
    save_frozen(p2, fm)
    lm = load_frozen(p2)
    assert isinstance(lm, FrozenMLP) and not isinstance(lm, FrozenCNN)
    assert torch.equal(lm.forward(u), fm.forward(u))


def test_refresh_and_the_latent_org_weight():
    from bnn_amd import freeze
    from bnn_amd.inference import _unpack_conv_rows
    m = _model()
    latent = torch.randn_like(m.layer2[0].weight)
    m.layer2[0].weight.org = latent.clone()
    m.layer2[0].weight.data = torch.zeros_like(latent)      # what .data holds does not matter
    fz = freeze(m)
    assert torch.equal(_unpack_conv_rows(fz.t["conv2.wq"], 32, 16, 5, 5).float(), latent.sign())
    m.layer2[0].weight.org = -latent
    fz.refresh()
    assert torch.equal(_unpack_conv_rows(fz.t["conv2.wq"], 32, 16, 5, 5).float(), (-latent).sign())


def test_refresh_keeps_two_pass_and_drops_the_buffers():
    from bnn_amd import freeze
    from bnn_amd.inference import _unpack_conv_rows
    m = _model()
    fz = freeze(m, normalize=NORM)
    fz.two_pass = True
    fz._buffers(3, torch.device("cpu"))
    assert fz._buf
    with torch.no_grad():
        m.layer2[0].weight.neg_()
    want = m.layer2[0].weight.detach().sign()
    assert fz.refresh() is fz
    assert fz.two_pass is True and fz.normalize == NORM
    assert torch.equal(_unpack_conv_rows(fz.t["conv2.wq"], 32, 16, 5, 5).float(), want)
    assert fz._buf == {}


def test_a_state_written_by_the_parent_format_loads(tmp_path):
    from bnn_amd import freeze
    from test_inference import check_parent_state_loads, parent_state
    fz = freeze(_model(seed=4), normalize=NORM)
    state = parent_state(fz, ["bnn_amd.frozen_cnn/1", ("layers", [[1, 16, 5, 5, 2], [16, 32, 5, 5, 2]]),
                              ("in_hw", [28, 28]), ("normalize", [0.1307, 0.3081]), ("eps", [1e-05, 1e-05])])
    assert sorted(state["tensors"]) == sorted(
        [f"{p}{i}.{k}" for i in (1, 2) for p, ks in (("conv", ("sign", "wq", "bias")),
                                                     ("bn", ("mean", "var", "invstd", "gamma", "beta"))) for k in ks]
        + ["fc.weight", "fc.bias", "pixel.table"])
    check_parent_state_loads(fz, state, ["format", "layers", "in_hw", "normalize", "eps", "tensors"],
                             _pixels(19, seed=8), tmp_path)


def test_freeze_refuses_what_the_sign_identity_does_not_cover():
    from bnn_amd import freeze
    m = _model()
    m.layer2[1] = torch.nn.BatchNorm2d(32, track_running_stats=False)
    with pytest.raises(ValueError, match="running statistics"):
        freeze(m)
    for bad in (torch.nn.ReLU(), torch.nn.Hardtanh(-2.0, 2.0)):
        m = _model()
        m.layer1[2] = bad
        with pytest.raises(ValueError, match="Hardtanh"):
            freeze(m)
    for bad in (torch.nn.MaxPool2d(2, 2, ceil_mode=True), torch.nn.MaxPool2d(3, 2, padding=1), torch.nn.AvgPool2d(2, 2)):
        m = _model()
        m.layer2[3] = bad
        with pytest.raises(ValueError, match="MaxPool2d"):
            freeze(m)
    m = _model()
    m.layer1 = torch.nn.Sequential(m.layer1[0], m.layer1[2], m.layer1[1], m.layer1[3])     # wrong order
    with pytest.raises(ValueError, match="layer1"):
        freeze(m)
    with pytest.raises(TypeError):
        freeze(torch.nn.Linear(4, 4))
    with pytest.raises(TypeError):
        freeze(torch.nn.Sequential(torch.nn.Conv2d(1, 4, 3)))


def test_conv_infer_entries_reject_bad_arguments_without_a_gpu():
    from bnn_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(4096)

    def sign(x=p, xfmt=2, table=None, wq=p, mean=p, invstd=p, out=p, N=4, C=16, H=14, W=14, Co=32, K=5, stride=1,
             pad=2, dil=1, groups=1):
        return L.bnn_conv2d_fwd_bnsign_pool(x, xfmt, table, wq, None, mean, invstd, None, None, out, N, C, H, W, Co,
                                            K, K, stride, pad, dil, groups, None)

    def head(x=p, wq=p, mean=p, invstd=p, fcw=p, out=p, n_out=10, N=4, C=16, H=14, W=14, Co=32, K=5, stride=1, pad=2,
             dil=1, groups=1):
        return L.bnn_conv2d_fwd_bn_pool_linear(x, wq, None, mean, invstd, None, None, fcw, None, n_out, out, N, C, H,
                                               W, Co, K, K, stride, pad, dil, groups, None)

    for call in (sign, head):
        assert call(out=None) == -1                        # null output
        assert b"bad arguments" in L.bnn_last_error()
        assert call(H=13, W=13) == -1                      # odd OH
        assert call(C=8) == -1                             # C neither 1 nor a multiple of 16
        assert call(stride=2) == -1
        assert call(dil=2) == -1 and call(groups=2) == -1
        assert call(Co=65) == -1 and call(pad=5) == -1
        assert call(C=80) == -1
        assert call(H=20, W=20) == -1                      # more than 256 output pixels on the MFMA kernels
        assert call(wq=None) == -1 and call(mean=None) == -1 and call(invstd=None) == -1 and call(x=None) == -1
        assert call(wq=ctypes.c_void_p(4104)) == -1        # wq not 16-B aligned
        assert call(x=ctypes.c_void_p(4104)) == -1         # 16-B row copies need an aligned image
        assert call(N=-1) == -1
        assert call(N=0) == 0                              # nothing to do, nothing launched
    assert sign(out=ctypes.c_void_p(4104)) == -1           # misaligned output
    assert head(out=ctypes.c_void_p(4098)) == -1
    assert sign(xfmt=3) == -1
    assert sign(xfmt=1) == -1                              # u8 pixels: one channel only
    assert sign(xfmt=1, C=1, H=28, W=28, Co=16, table=None) == -1       # ... and they need the table
    assert sign(xfmt=1, C=1, H=28, W=28, Co=16, table=p, N=0) == 0
    assert sign(xfmt=0, C=1, H=27, W=27, Co=16) == -1      # odd OH on the single-channel kernel
    assert sign(xfmt=0, C=1, H=28, W=28, Co=16, K=9, pad=4) == -1       # KW > 8
    assert head(n_out=9) == -1
    assert head(fcw=None) == -1
    assert head(C=1, H=28, W=28, Co=16) == -1              # the head takes the int8-MFMA geometry only
    assert head(C=64, H=16, W=16, Co=64, K=3, pad=1) == -1     # 64 x 64 x 10 classifier: beyond one workgroup's LDS
    ok = L.bnn_conv2d_fwd_bnsign_pool_ok
    assert ok(1, 9, 1, 28, 28, 16, 5, 5, 1, 2, 1, 1) == 1 and ok(2, 9, 16, 14, 14, 32, 5, 5, 1, 2, 1, 1) == 1
    assert ok(0, 9, 32, 8, 8, 20, 5, 5, 1, 2, 1, 1) == 1 and ok(0, 9, 1, 10, 10, 8, 3, 3, 1, 1, 1, 1) == 1
    assert ok(2, 9, 16, 13, 13, 32, 5, 5, 1, 2, 1, 1) == 0 and ok(2, 9, 8, 14, 14, 32, 5, 5, 1, 2, 1, 1) == 0
    hk = L.bnn_conv2d_fwd_bn_pool_linear_ok
    assert hk(9, 16, 14, 14, 32, 5, 5, 1, 2, 1, 1, 10) == 1 and hk(9, 16, 14, 14, 32, 5, 5, 1, 2, 1, 1, 9) == 0
    assert hk(9, 16, 14, 14, 32, 5, 5, 2, 2, 1, 1, 10) == 0
    with pytest.raises(_lib.BnnError):
        _lib.call("bnn_conv2d_fwd_bn_pool_linear", None, None, None, None, None, None, None, None, None, 10, None, 4,
                  16, 14, 14, 32, 5, 5, 1, 2, 1, 1, None)

