"""Frozen-model inference without a GPU: the snapshot of bnn_amd.inference.freeze and its plain-torch
forward against ``model.eval()``, the state round-trips, and the argument checks of the new C entries."""
import ctypes

import pytest
import torch
import torch.nn.functional as tF

from bnn_amd import functional as BF
from bnn_amd import nets


def _cpu_binary_linear(x, weight, bias=None, binarize_input=True, backend="fp4", cache=False, xpack=None):
    """BinarizeLinear's forward value in plain torch (binarized_modules.py:73-85), in the dtype of x."""
    y = tF.linear(x.sign() if binarize_input else x, weight.sign())
    return y if bias is None else y + bias


def _model(seed=0, **kw):
    torch.manual_seed(seed)
    m = nets.MLP(192, 192, 192, org_protocol=False, mutate_input=False, **kw)
    g = torch.Generator().manual_seed(seed + 1)
    for bn, scale in ((m.bn1, 30.0), (m.bn2, 12.0), (m.bn3, 12.0)):
        bn.running_mean.copy_(torch.randn(bn.num_features, generator=g) * 0.3 * scale)
        bn.running_var.copy_((torch.rand(bn.num_features, generator=g) + 0.5) * scale * scale)
        with torch.no_grad():
            bn.weight.copy_(torch.rand(bn.num_features, generator=g) + 0.5)
            bn.bias.copy_(torch.randn(bn.num_features, generator=g) * 0.2)
    with torch.no_grad():
        m.bn1.weight[5] = -0.75          # one negative gamma per hidden BatchNorm
        m.bn2.weight[17] = -1.25
    return m.eval()


def _pixels(n, seed=3):
    g = torch.Generator().manual_seed(seed)
    u = torch.randint(0, 256, (n, 1, 28, 28), generator=g)
    return torch.where(torch.rand((n, 1, 28, 28), generator=g) < 0.8, torch.zeros_like(u), u).to(torch.uint8)


def test_frozen_cpu_forward_matches_model_eval_signs(monkeypatch):
    from bnn_amd import freeze
    m = _model()
    u = _pixels(37)
    fz = freeze(m)
    logp = fz.forward(u)
    s1, s2 = fz.hidden_signs(u)
    # model.eval() in plain torch, evaluated in float64 so the reference's own summation order plays
    # no part: the hidden GEMMs are integer sums either way
    monkeypatch.setattr(BF, "binary_linear", _cpu_binary_linear)
    md = _model().double()
    taps = {}
    hooks = [md.htanh1.register_forward_hook(lambda mod, i, o: taps.__setitem__(1, o.detach().sign())),
             md.htanh2.register_forward_hook(lambda mod, i, o: taps.__setitem__(2, o.detach().sign()))]
    with torch.no_grad():
        ref = md(BF.pixels_to_float(u).double())
    for h in hooks:
        h.remove()
    assert s1.shape == (37, 192) and s2.shape == (37, 192)
    assert torch.equal(s1.double(), taps[1]) and torch.equal(s2.double(), taps[2])
    assert (s1[:, 5] != 0).any() and (s2 != 0).any()
    assert logp.shape == (37, 10) and logp.dtype == torch.float32
    assert float((logp.double() - ref).abs().max()) < 1e-4      # fp32 head against the float64 one
    assert torch.equal(logp.argmax(1), fz.predict(u))


def test_frozen_uses_the_latent_org_weight():
    from bnn_amd import freeze
    m = _model()
    latent = torch.randn_like(m.fc2.weight)
    m.fc2.weight.org = latent.clone()
    m.fc2.weight.data = torch.zeros_like(latent)         # what .data holds does not matter
    fz = freeze(m)
    from bnn_amd.inference import _unpack_fp4_rows
    assert torch.equal(_unpack_fp4_rows(fz.t["fc2.q4"], 192).float(), latent.sign())
    # refresh() picks up further training
    m.fc2.weight.org = -latent
    fz.refresh()
    assert torch.equal(_unpack_fp4_rows(fz.t["fc2.q4"], 192).float(), (-latent).sign())


def test_frozen_state_round_trips(tmp_path):
    from bnn_amd import FrozenMLP, freeze
    from bnn_amd.checkpoint import load_frozen, save_frozen
    m = _model(seed=4, normalize=(0.1307, 0.3081))
    u = _pixels(19, seed=8)
    fz = freeze(m)
    want = fz.forward(u)
    again = FrozenMLP.from_state(fz.state_dict())
    assert again.widths == (192, 192, 192) and again.normalize == (0.1307, 0.3081)
    assert torch.equal(again.forward(u), want)
    path = str(tmp_path / "frozen.pt")
    save_frozen(path, fz)
    del m
    loaded = load_frozen(path)
    assert torch.equal(loaded.forward(u), want)
    assert torch.equal(loaded.forward(u.reshape(19, 784)), want)
    with pytest.raises(RuntimeError, match="refresh"):
        loaded.refresh()


def test_refresh_keeps_two_pass_and_drops_the_buffers():
    from bnn_amd import freeze
    from bnn_amd.inference import _unpack_fp4_rows
    m = _model()
    fz = freeze(m)
    fz.two_pass = True
    fz._buffers(3, torch.device("cpu"))
    assert fz._buf
    with torch.no_grad():
        m.fc3.weight.neg_()
    want = m.fc3.weight.detach().sign()
    assert fz.refresh() is fz
    assert fz.two_pass is True
    assert torch.equal(_unpack_fp4_rows(fz.t["fc3.q4"], 192).float(), want)
    assert fz._buf == {}


def parent_state(fz, meta):
    """The dictionary the state_dict() of the commit that introduced the formats wrote, rebuilt by hand:
    ``meta`` is that commit's literal list of (key, value) pairs after "format"."""
    return {"format": meta[0], **dict(meta[1:]), "tensors": {k: v.clone() for k, v in fz.t.items()}}


def check_parent_state_loads(fz, state, keys, u, tmp_path):
    from bnn_amd import inference
    from bnn_amd.checkpoint import load_frozen
    assert list(state) == keys
    path = str(tmp_path / "parent.pt")
    torch.save(state, path)
    want = fz.forward(u)
    for got in (inference.from_state(state), load_frozen(path)):
        assert type(got) is type(fz)
        again = got.state_dict()
        assert list(again) == keys
        assert all(again[k] == state[k] for k in keys[:-1])
        assert list(again["tensors"]) == list(state["tensors"])
        assert all(torch.equal(again["tensors"][k], v) and again["tensors"][k].dtype == v.dtype
                   for k, v in state["tensors"].items())
        assert torch.equal(got.forward(u), want)


def test_a_state_written_by_the_parent_format_loads(tmp_path):
    from bnn_amd import freeze, inference
    fz = freeze(_model(seed=4, normalize=(0.1307, 0.3081)))
    state = parent_state(fz, ["bnn_amd.frozen/1", ("widths", [192, 192, 192]), ("normalize", [0.1307, 0.3081]),
                              ("eps", [1e-05, 1e-05, 1e-05])])
    assert sorted(state["tensors"]) == sorted(
        [f"bn{i}.{k}" for i in (1, 2, 3) for k in ("mean", "var", "invstd", "gamma", "beta")]
        + ["fc1.q", "fc1.rowsum", "fc2.q4", "fc3.q4", "fc1.bias", "fc2.bias", "fc3.bias", "fc4.weight", "fc4.bias"])
    check_parent_state_loads(fz, state, ["format", "widths", "normalize", "eps", "tensors"], _pixels(19, seed=8),
                             tmp_path)
    with pytest.raises(ValueError, match=r"bnn_amd\.frozen/1.*bnn_amd\.frozen_cnn/1"):
        inference.from_state({"format": "x"})


def test_tensor_level_eval_head_checks_its_arguments():
    """The argument errors of bn_hardtanh_linear_eval, raised by the tensor-level functions it wraps
    (before any device check, so a CPU tensor shows them)."""
    z = torch.zeros(4, 192)
    v = torch.ones(192)
    w4 = torch.zeros(10, 192)
    pair = (torch.zeros(4, 192, dtype=torch.int16), v)
    no_stats = "bn_hardtanh_linear_eval needs a BatchNorm with running statistics"
    needs_fused = r"bn_hardtanh_linear_eval: an int16 pre-activation needs the fused head \(head_eval_fusable\)"
    with pytest.raises(ValueError, match=needs_fused):
        BF.bn_linear_eval(pair, v, v, 1e-5, None, None, w4, None)
    with pytest.raises(ValueError, match=no_stats):
        BF.bn_linear_eval(z, v, None, 1e-5, None, None, w4, None)
    with pytest.raises(ValueError, match=needs_fused):       # 192 is no width of the fused head
        BF.bn_head_eval(pair, v, v, None, None, w4, None)
    with pytest.raises(ValueError, match=no_stats):
        BF.bn_head_eval(z, v, None, None, None, w4, None)
    assert BF.head_eval_fusable(256, 256, 10) and not BF.head_eval_fusable(192, 192, 10)
    assert not BF.head_eval_fusable(256, 256, 12) and not BF.head_eval_fusable(256, 128, 10)


def test_freeze_needs_running_statistics():
    from bnn_amd import freeze
    m = _model()
    m.bn2 = torch.nn.BatchNorm1d(192, track_running_stats=False)
    with pytest.raises(ValueError, match="running statistics"):
        freeze(m)
    with pytest.raises(TypeError):
        freeze(torch.nn.Linear(4, 4))


def test_bnsign_entries_reject_bad_arguments_without_a_gpu():
    from bnn_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(16)

    def fp4(K=64, N=8, ldq4=128, q4=p, mean=p, lda=64):
        return L.bnn_gemm_fp4_bnsign(p, lda, p, 64, None, mean, p, None, None, q4, ldq4, 8, N, K, None)

    def i8(K=64, N=8, ldq4=128, q4=p, invstd=p):
        return L.bnn_gemm_i8_affine_bnsign(p, 64, p, 64, None, None, None, 0.0, p, invstd, None, None, q4, ldq4,
                                           8, N, K, None)

    for call in (fp4, i8):
        assert call(K=63) == -1                    # K not a multiple of 64
        assert b"bad arguments" in L.bnn_last_error()
        assert call(N=6) == -1                     # N % 4 != 0
        assert call(ldq4=64) == -1                 # ldq4 not a multiple of 128
        assert call(N=260, ldq4=128) == -1         # 2 ldq4 < round_up(N, 256)
        assert call(q4=None) == -1
        assert call(q4=ctypes.c_void_p(24)) == -1  # q4 not 16-B aligned
    assert fp4(mean=None) == -1 and i8(invstd=None) == -1
    assert fp4(lda=32) == -1                       # lda < K
    # the eval head: exactly one of x / x16, C % 128 == 0
    assert L.bnn_bn_head_eval(None, None, None, 8, 128, p, p, None, None, p, 10, None, p, None) == -1
    assert L.bnn_bn_head_eval(p, p, p, 8, 128, p, p, None, None, p, 10, None, p, None) == -1
    assert L.bnn_bn_head_eval(p, None, None, 8, 192, p, p, None, None, p, 10, None, p, None) == -1
    with pytest.raises(_lib.BnnError):
        _lib.call("bnn_gemm_fp4_bnsign", None, 64, None, 64, None, None, None, None, None, None, 128, 8, 8, 64, None)
