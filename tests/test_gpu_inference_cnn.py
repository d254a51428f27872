"""GPU checks of frozen BinCNN inference (bnn_amd.inference.FrozenCNN).

* bnn_conv2d_fwd_bnsign_pool against the two-pass form it replaces -- bnn_conv2d_fwd +
  bnn_bn2d_fwd_eval(hardtanh, pool 2), then tsign, channels innermost -- byte for byte, pad channels and
  guard bytes included, for every input form, at the BinCNN's two geometries and three others.
* bnn_conv2d_fwd_bn_pool_linear and the whole frozen network against a float64 evaluation from the
  exact integer sums, with the rule of §11: err_new <= max(2 err_old, one fp32 ulp of max|L64|), err_old
  being the existing eval path's error on the same input, measured in the same test.

One thing the two forms do NOT share, found while writing this: a NaN BatchNorm output.  The existing
pass clamps with fminf(fmaxf(y, -1), 1), which returns -1 for a NaN y, so its pooled value is -1.0 and
its sign -1; the new kernel gives 0 (tsign(NaN), what torch's Hardtanh -> MaxPool2d -> sign gives with
tsign's NaN rule).  The rigged beta = NaN channel is therefore asserted to be all 0 in the new kernel's
output and left out of the byte comparison; the two-pass value is printed.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NORM = (0.1307, 0.3081)
GUARD = 0x5A


@pytest.fixture(scope="module")
def F():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from bnn_amd import functional
    return functional


def _ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


def _tsign(x):
    return (x > 0).to(torch.int8) - (x < 0).to(torch.int8)


def _conv_f32(x, w, bias, pad):
    """bnn_conv2d_fwd on a binarised input: exact integer sums + bias, fp32 NCHW."""
    from bnn_amd import _lib as L
    N, C, H, W = x.shape
    Co, _, K, _ = w.shape
    OH = H + 2 * pad - K + 1
    y = torch.empty((N, Co, OH, OH), dtype=torch.float32, device="cuda")
    L.call("bnn_conv2d_fwd", L.ptr(x), 1, L.ptr(w), L.ptr(bias), L.ptr(y), N, C, H, W, Co, K, K, 1, pad, 1, 1,
           L.stream())
    return y


def _bn_eval_pool(z, mean, var, eps, gamma, beta):
    """bnn_bn2d_fwd_eval(hardtanh = 1, pool = 2): the pooled fp32 map of the existing eval path."""
    from bnn_amd import _lib as L
    N, C, H, W = z.shape
    y = torch.empty((N, C, H // 2, W // 2), dtype=torch.float32, device="cuda")
    ws = torch.empty((L.lib().bnn_bn2d_workspace(N, C),), dtype=torch.uint8, device="cuda")
    L.call("bnn_bn2d_fwd_eval", L.ptr(z), N, C, H, W, L.ptr(gamma), L.ptr(beta), L.ptr(mean), L.ptr(var), float(eps),
           L.ptr(y), 1, 2, L.ptr(ws), L.stream())
    return y


def _nhwc_signs(y):
    N, C, H, W = y.shape
    a = torch.zeros((N, H, W, (C + 15) // 16 * 16), dtype=torch.int8, device=y.device)
    a[..., :C] = _tsign(y).permute(0, 2, 3, 1)
    return a


def _pack(w):
    from bnn_amd import inference as I
    return I._pack_conv_c1(w) if w.shape[1] == 1 else I._pack_conv_rows(w)


def _bnsign_pool(x, xfmt, table, w, bias, mean, invstd, gamma, beta, geo):
    """The new entry on a guarded output: (signs [N][PH][PW][Cop], untouched-guard flag)."""
    from bnn_amd import _lib as L
    N, C, H, Wd, Co, K, pad = geo
    PH = (H + 2 * pad - K + 1) // 2
    Cop = (Co + 15) // 16 * 16
    n = N * PH * PH * Cop
    buf = torch.full((n + 4096,), GUARD, dtype=torch.uint8, device="cuda").view(torch.int8)
    L.call("bnn_conv2d_fwd_bnsign_pool", L.ptr(x), xfmt, L.ptr(table), L.ptr(_pack(w)), L.ptr(bias), L.ptr(mean),
           L.ptr(invstd), L.ptr(gamma), L.ptr(beta), L.ptr(buf), N, C, H, Wd, Co, K, K, 1, pad, 1, 1, L.stream())
    tail_ok = bool((buf[n:].view(torch.uint8) == GUARD).all())
    return buf[:n].view(N, PH, PH, Cop).clone(), tail_ok


def _layer_case(N, C, H, Co, K, pad, seed):
    """Random layer with rigged BatchNorm channels: 0 has y == 0 exactly at the channel's largest sum (mean =
    fl(k + bias), gamma 1, beta 0), 1 has beta = NaN, 2 a negative gamma."""
    from bnn_amd import inference as I
    g = torch.Generator(device="cuda").manual_seed(seed)
    if C == 1:
        u = torch.randint(0, 256, (N, 1, H, H), generator=g, device="cuda")
        u = torch.where(torch.rand((N, 1, H, H), generator=g, device="cuda") < 0.6, torch.zeros_like(u), u)
        x = u.to(torch.uint8)
    else:
        x = torch.randint(-1, 2, (N, C, H, H), generator=g, device="cuda").float()
        x = x * (torch.rand((N, C, H, H), generator=g, device="cuda") + 0.25)
    w = torch.randn((Co, C, K, K), generator=g, device="cuda")
    w[0, 0, 0, 0] = 0.0
    bias = torch.randn(Co, generator=g, device="cuda") * 0.5
    sd = float(C * K * K) ** 0.5 * (0.5 if C == 1 else 1.0)
    mean = torch.randn(Co, generator=g, device="cuda") * 0.3 * sd
    var = (torch.rand(Co, generator=g, device="cuda") + 0.5) * sd * sd
    gamma = torch.rand(Co, generator=g, device="cuda") + 0.5
    beta = torch.randn(Co, generator=g, device="cuda") * 0.2
    eps = 1e-5
    return {"x": x, "w": w, "bias": bias, "mean": mean, "var": var, "gamma": gamma, "beta": beta, "eps": eps,
            "invstd": I._invstd(var, eps), "geo": (N, C, H, H, Co, K, pad)}


def _rig(c, xf):
    """Rig channels 0..2 from the layer's own sums (xf: its fp32 NCHW input)."""
    z = _conv_f32(xf, c["w"], c["bias"], c["geo"][6])
    k = (z[:, 0] - c["bias"][0]).round().max()                   # an integer sum that occurs in channel 0
    c["mean"][0] = k + c["bias"][0]                              # fl(k + bias): y == 0 exactly there
    c["gamma"][0], c["beta"][0] = 1.0, 0.0
    c["beta"][1] = float("nan")
    c["gamma"][2] = -0.75
    return z


def _check_layer(c, x, xfmt, table, z, label):
    Co = c["geo"][4]
    want = _nhwc_signs(_bn_eval_pool(z, c["mean"], c["var"], c["eps"], c["gamma"], c["beta"]))
    got, tail_ok = _bnsign_pool(x, xfmt, table, c["w"], c["bias"], c["mean"], c["invstd"], c["gamma"], c["beta"], c["geo"])
    assert tail_ok, f"{label}: bytes beyond sample N were written"
    keep = [ch for ch in range(got.shape[3]) if ch != 1]
    assert torch.equal(got[..., keep], want[..., keep]), label          # pad channels (0) included
    assert int(got[..., Co:].abs().sum()) == 0, label
    assert int(got[..., 1].abs().sum()) == 0, label                     # beta = NaN: all 0
    assert int((got[..., 0] == 0).sum()) > 0, label                     # the exact zero shows as code 0
    assert set(got[..., 2:Co].unique().tolist()) >= {-1, 1}, label
    return got, want


@pytest.mark.parametrize("N", [1, 9])
@pytest.mark.parametrize("normalize", [None, NORM])
def test_bnsign_pool_conv1_geometry_all_input_forms(F, N, normalize):
    """C 1 -> 16, 5 x 5 pad 2, 28 x 28; N = 9 leaves a ragged last group of samples.  u8 pixels through the
    sign table, the fp32 images (u / 255 - m) / s binarised in the kernel and the int8 signs give
    identical bytes, equal to the two-pass form's."""
    from bnn_amd import inference as I
    c = _layer_case(N, 1, 28, 16, 5, 2, seed=100 + N)
    xf = F.pixels_to_float(c["x"], normalize).contiguous()
    z = _rig(c, xf)
    table = I.pixel_sign_table(normalize).cuda()
    got_u8, want = _check_layer(c, c["x"], 1, table, z, "u8")
    got_f32, _ = _check_layer(c, xf, 0, None, z, "fp32")
    s8 = _tsign(xf).permute(0, 2, 3, 1).contiguous()
    got_s8, _ = _check_layer(c, s8, 2, None, z, "int8")
    assert torch.equal(got_u8, got_f32) and torch.equal(got_u8, got_s8)
    print(f"conv1 N={N} normalize={normalize}: two-pass sign in the beta = NaN channel: "
          f"{want[..., 1].unique().tolist()}, new kernel: {got_u8[..., 1].unique().tolist()}")


GEOMETRIES = [(1, 16, 14, 32, 5, 2), (9, 16, 14, 32, 5, 2),      # conv2 of the BinCNN
              (5, 16, 12, 48, 3, 1),                              # three channel tiles run as four
              (5, 32, 8, 20, 5, 2),                               # pad channels 20..31
              (5, 1, 10, 8, 3, 1)]                                # odd pooled size 5 x 5, one dot4 group


@pytest.mark.parametrize("N,C,H,Co,K,pad", GEOMETRIES)
def test_bnsign_pool_matches_the_two_pass_form(F, N, C, H, Co, K, pad):
    c = _layer_case(N, C, H, Co, K, pad, seed=N + C + H + Co)
    xf = F.pixels_to_float(c["x"]).contiguous() if C == 1 else c["x"]
    z = _rig(c, xf)
    got_f32, _ = _check_layer(c, xf, 0, None, z, "fp32")
    s8 = _tsign(xf).permute(0, 2, 3, 1).contiguous()
    got_s8, _ = _check_layer(c, s8, 2, None, z, "int8")
    assert torch.equal(got_f32, got_s8)
    # no bias, no affine
    c2 = dict(c, bias=None, gamma=None, beta=None)
    z0 = _conv_f32(xf, c["w"], None, pad)
    want = _nhwc_signs(_bn_eval_pool(z0, c["mean"], c["var"], c["eps"], None, None))
    got, tail_ok = _bnsign_pool(s8, 2, None, c["w"], None, c["mean"], c["invstd"], None, None, c2["geo"])
    assert tail_ok and torch.equal(got, want)


def _head_case(N, C, H, Co, K, pad, seed):
    c = _layer_case(N, C, H, Co, K, pad, seed)
    g = torch.Generator(device="cuda").manual_seed(seed + 1)
    PH = (H + 2 * pad - K + 1) // 2
    feat = Co * PH * PH
    c["fcw"] = (torch.rand((10, feat), generator=g, device="cuda") * 2 - 1) / feat ** 0.5
    c["fcb"] = torch.randn(10, generator=g, device="cuda") * 0.1
    c["s8"] = _tsign(c["x"]).permute(0, 2, 3, 1).contiguous()
    return c


def _head(c, rows=None):
    from bnn_amd import _lib as L
    N, C, H, Wd, Co, K, pad = c["geo"]
    s8 = c["s8"] if rows is None else c["s8"][rows].contiguous()
    n = s8.shape[0]
    y = torch.empty((n, 10), dtype=torch.float32, device="cuda")
    L.call("bnn_conv2d_fwd_bn_pool_linear", L.ptr(s8), L.ptr(_pack(c["w"])), L.ptr(c["bias"]), L.ptr(c["mean"]),
           L.ptr(c["invstd"]), L.ptr(c["gamma"]), L.ptr(c["beta"]), L.ptr(c["fcw"]), L.ptr(c["fcb"]), 10, L.ptr(y), n, C,
           H, Wd, Co, K, K, 1, pad, 1, 1, L.stream())
    return y


def _head64(c):
    """float64 from the exact integer sums: conv on signs in double, one fp32 rounding of I + bias,
    everything after in double."""
    d = torch.float64
    pad = c["geo"][6]
    I = torch.nn.functional.conv2d(c["x"].sign().to(d), c["w"].sign().to(d), None, 1, pad)
    x = (I.float() + c["bias"].view(1, -1, 1, 1)).to(d)
    v = lambda t: t.to(d).view(1, -1, 1, 1)
    y = (x - v(c["mean"])) / (v(c["var"]) + c["eps"]).sqrt() * v(c["gamma"]) + v(c["beta"])
    p = torch.nn.functional.max_pool2d(y.clamp(-1.0, 1.0), 2, 2)
    return p.reshape(p.shape[0], -1) @ c["fcw"].to(d).t() + c["fcb"].to(d)


@pytest.mark.parametrize("C,H,Co,K,pad", [(16, 14, 32, 5, 2), (32, 8, 20, 3, 1)])
def test_bn_pool_linear_against_float64(F, C, H, Co, K, pad):
    """The fused head against float64, with the existing eval path (bnn_conv2d_fwd + bnn_bn2d_fwd_eval +
    linear_nsmall) measured on the same input.  Both figures are printed (recorded in DESIGN.md §12).
    Deterministic, and a sample's logits do not depend on the batch it sits in."""
    N = 300
    c = _head_case(N, C, H, Co, K, pad, seed=C + H)
    L64 = _head64(c)
    new = _head(c)
    pooled = _bn_eval_pool(_conv_f32(c["x"], c["w"], c["bias"], pad), c["mean"], c["var"], c["eps"], c["gamma"],
                           c["beta"])
    old = F.linear_nsmall(pooled.reshape(N, -1), c["fcw"], c["fcb"])
    err_old = float((old.double() - L64).abs().max())
    err_new = float((new.double() - L64).abs().max())
    bound = max(2 * err_old, _ulp32(float(L64.abs().max())))
    print(f"bn_pool_linear C={C} Co={Co} {H}x{H}: err_new {err_new:.3e} err_old {err_old:.3e} bound {bound:.3e} "
          f"max|L64| {float(L64.abs().max()):.3f}")
    assert new.shape == (N, 10) and torch.isfinite(new).all()
    assert err_new <= bound, (err_new, err_old, bound)
    assert torch.equal(_head(c), new)                                  # two runs: identical bits
    rows = torch.tensor([0, 7, 15, 16, 17, 150, 290, 298, 299], device="cuda")
    assert torch.equal(_head(c, rows), new[rows])                      # N = 9 call = the same rows of N = 300


# ----------------------------------------------------------------------------- whole net
@pytest.fixture(scope="module")
def trained(F):
    """BinCNN(fused_bn=True) after 3 training steps on 300 synthetic u8-derived samples, in eval mode, without
    and with Normalize: the existing path's log-probabilities and pooled layer-1 map, the frozen model's,
    and the float64 ones from layer 2's exact integer sums."""
    from bnn_amd import freeze, nets
    from bnn_amd.data import synthetic_mnist
    from bnn_amd.optim import LatentAdam
    out = {}
    u, y = synthetic_mnist(300, seed=11, device="cuda", as_u8=True)
    for key, normalize in (("plain", None), ("norm", NORM)):
        torch.manual_seed(7)
        xf = F.pixels_to_float(u, normalize).contiguous()
        model = nets.BinCNN(org_protocol=False, mutate_input=False, fused_bn=True).cuda().train()
        opt = LatentAdam(model.parameters(), lr=0.01, clamp_params=nets.binary_params(model))
        for _ in range(3):
            opt.zero_grad(set_to_none=True)
            torch.nn.functional.nll_loss(model(xf), y).backward()
            opt.step()
        model.eval()
        taps = {}
        hook = model.layer1.register_forward_hook(lambda mod, i, o: taps.__setitem__(1, o.detach().clone()))
        with torch.no_grad():
            old = model(xf)
        hook.remove()
        if 1 not in taps:          # the fused layer does not go through the Sequential's forward
            with torch.no_grad():
                taps[1] = model._layer(model.layer1, xf)
        fz = freeze(model, normalize=normalize)
        new = fz(u).clone()
        # float64 from layer 2's exact sums on the model's own layer-1 signs
        d = torch.float64
        conv, bn = model.layer2[0], model.layer2[1]
        I2 = torch.nn.functional.conv2d(taps[1].sign().to(d), conv.weight.detach().sign().to(d), None, 1, 2)
        x2 = (I2.float() + conv.bias.detach().view(1, -1, 1, 1)).to(d)
        v = lambda t: t.detach().to(d).view(1, -1, 1, 1)
        y2 = (x2 - v(bn.running_mean)) / (v(bn.running_var) + bn.eps).sqrt() * v(bn.weight) + v(bn.bias)
        p2 = torch.nn.functional.max_pool2d(y2.clamp(-1.0, 1.0), 2, 2).reshape(300, -1)
        lp64 = torch.log_softmax(p2 @ model.fc.weight.detach().to(d).t() + model.fc.bias.detach().to(d), dim=1)
        out[key] = {"model": model, "fz": fz, "u": u, "xf": xf, "y": y, "old": old, "new": new, "lp64": lp64,
                    "pooled1": taps[1]}
    return out


@pytest.mark.parametrize("key", ["plain", "norm"])
def test_frozen_cnn_matches_model_eval(trained, key):
    """Frozen log-probabilities against float64 with the head's rule, the labels wherever the float64 top-2
    margin exceeds the bound, layer 1's signs exactly.  Both errors are printed."""
    t = trained[key]
    old, new, lp64, fz = t["old"], t["new"], t["lp64"], t["fz"]
    assert new.shape == (300, 10) and torch.isfinite(new).all()
    err_old = float((old.double() - lp64).abs().max())
    err_new = float((new.double() - lp64).abs().max())
    bound = max(2 * err_old, _ulp32(float(lp64.abs().max())))
    top2 = lp64.topk(2, dim=1).values
    margin = top2[:, 0] - top2[:, 1]
    print(f"frozen cnn {key}: err_new {err_new:.3e} err_old {err_old:.3e} bound {bound:.3e} "
          f"min margin {float(margin.min()):.3e}")
    assert err_new <= bound, (err_new, err_old, bound)
    sure = margin > bound
    assert int((~sure).sum()) <= 3
    assert torch.equal(fz.predict(t["u"])[sure], old.argmax(1)[sure])
    hs = fz.hidden_signs(t["u"])
    assert hs.dtype == torch.int8 and torch.equal(hs, _tsign(t["pooled1"]))
    # fp32 images take the in-kernel binarisation: same signs, same output
    assert torch.equal(fz(t["xf"]), new)
    assert torch.equal(fz(t["u"].reshape(300, 784)), new)


@pytest.mark.parametrize("key", ["plain", "norm"])
def test_frozen_cnn_two_pass_form(trained, key):
    """two_pass = True runs the layers as model.eval() does (conv + bnn_bn2d_fwd_eval, linear_nsmall): layer 1's
    signs are the fused form's bit for bit and its output is model.eval()'s bit for bit; the classifier
    sums in fp32 there and in double in the fused head, so the log-probabilities are held to the same
    float64 rule rather than to equality."""
    t = trained[key]
    fz = t["fz"]
    hs = fz.hidden_signs(t["u"])
    fz.two_pass = True
    try:
        two = fz(t["u"]).clone()
        hs2 = fz.hidden_signs(t["u"])
    finally:
        fz.two_pass = False
    assert torch.equal(hs2, hs)
    assert torch.equal(two, t["old"])
    lp64 = t["lp64"]
    bound = max(2 * float((two.double() - lp64).abs().max()), _ulp32(float(lp64.abs().max())))
    assert float((t["new"].double() - lp64).abs().max()) <= bound
    top2 = lp64.topk(2, dim=1).values
    sure = (top2[:, 0] - top2[:, 1]) > bound
    assert torch.equal(two.argmax(1)[sure], t["new"].argmax(1)[sure])


def test_frozen_cnn_graph_capture_replays(trained):
    t = trained["norm"]
    fz = t["fz"]
    static_u = t["u"][:64].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fz(static_u)                                      # warm-up: buffers exist
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fz(static_u)
    static_u.copy_(t["u"][100:164])
    graph.replay()
    torch.cuda.synchronize()
    got = out.clone()
    assert torch.equal(got, fz(t["u"][100:164]))


def test_frozen_cnn_accuracy_and_reload(trained, tmp_path):
    from bnn_amd import FrozenCNN
    from bnn_amd.checkpoint import load_frozen, save_frozen
    t = trained["norm"]
    fz = t["fz"]
    acc = fz.accuracy(t["u"], t["y"], batch=128)          # 128 + 128 + 44: a short last batch
    assert round(acc * 300) == int((t["new"].argmax(1) == t["y"]).sum()) and 0.0 <= acc <= 1.0
    path = str(tmp_path / "cnn.pt")
    save_frozen(path, fz)
    loaded = load_frozen(path, map_location="cuda")
    assert isinstance(loaded, FrozenCNN) and loaded.device.type == "cuda"
    assert torch.equal(loaded(t["u"]), t["new"])
    cpu = load_frozen(path, map_location="cpu")
    sure = t["lp64"].topk(2, dim=1).values
    sure = (sure[:, 0] - sure[:, 1]) > 1e-4
    assert torch.equal(cpu.predict(t["u"].cpu())[sure.cpu()], t["new"].argmax(1).cpu()[sure.cpu()])


def test_trainer_eval_prints_accuracy_for_the_cnn(F, capsys):
    from bnn_amd import trainer
    trainer.main(["--model", "cnn", "--epochs", "1", "--eval", "256", "--dataset-size", "512", "--batch-size", "128",
                  "--log-interval", "100"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Eval 1 : accuracy ")]
    assert len(lines) == 1 and "256 held-out samples" in lines[0]
    assert 0.0 <= float(lines[0].split()[4]) <= 1.0
