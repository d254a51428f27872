"""Host logic of the autograd hand-offs (functional._placeholder / _q6_key): every gradient
placeholder is a stride-0 view of one cached zero per device, so they all share data_ptr and the
version counter; each carries a unique token that the hand-offs' staleness key includes, so two
placeholders of the same shape never key alike.  Also the pre-activation descriptor
(functional.PreAct: suffix, arguments, save / restore, exact decode, entry names against bnn.h) and the
one attach / take helper of the gradient hand-offs (stale and lost payloads).  All on CPU tensors."""
import numpy as np
import pytest
import torch

from bnn_amd import functional as F


def test_placeholders_key_apart():
    a = F._placeholder((4, 5), "cpu")
    b = F._placeholder((4, 5), "cpu")
    assert a.data_ptr() == b.data_ptr() and a.stride() == (0, 0)
    assert F._q6_key(a) != F._q6_key(b)
    assert F._q6_key(a) == F._q6_key(a)


def test_stale_handoff_refused():
    """A hand-off attached to one placeholder is not taken through another of the same shape."""
    a = F._placeholder((3, 64), "cpu")
    b = F._placeholder((3, 64), "cpu")
    setattr(b, F._Q6_ATTR, (F._q6_key(a), "rows", "cols", "cs"))      # a key that is not b's
    assert F._q6_take(b) is None
    setattr(a, F._Q6_ATTR, (F._q6_key(a), "rows", "cols", "cs"))
    assert F._q6_take(a) == ("rows", "cols", "cs")
    assert isinstance(torch.zeros(1), torch.Tensor)


# ---- the pre-activation descriptor (functional.PreAct) and the attach / take helper
def _preacts(with_bias):
    """One descriptor of each kind at its smallest shape: (kind, descriptor, suffix, bytes per element)."""
    b2 = torch.tensor([0.5, -1.25]) if with_bias else None
    x = torch.zeros(1, 2)
    x16 = torch.tensor([[3, -4]], dtype=torch.int16)
    hi = torch.tensor([[0x21]], dtype=torch.uint8)
    xq = torch.ones((1, 1, 2, 2), dtype=torch.int16)
    xq8 = xq.to(torch.int8)
    bq = torch.tensor([0.5]) if with_bias else None
    return [(F.PreAct("f32", x), (x,), "", 4), (F.PreAct("z16", x16, b2), (x16, b2), "_i16", 2),
            (F.PreAct("s20", x16, hi, b2, 0.25), (x16, hi, b2, 0.25), "_s20", 2.5),
            (F.PreAct("zq", xq, bq, 2), (xq, bq, 2), "_q", 2),
            (F.PreAct("zq", xq8, bq, 1), (xq8, bq, 1), "_q", 1)]


@pytest.mark.parametrize("with_bias", [True, False])
def test_preact_suffix_arguments_bytes_and_round_trip(with_bias):
    for d, args, suffix, nbytes in _preacts(with_bias):
        assert d.suffix == suffix and d.nbytes == nbytes and d.compact == (d.kind != "f32")
        assert len(d.args) == len(args) and all(a is b for a, b in zip(d.args, args))
        assert d.shape == args[0].shape and d.device == args[0].device
        saved, meta = d.saved(), d.meta()
        assert len(saved) == 3 and all(t is None or isinstance(t, torch.Tensor) for t in saved)
        assert not any(isinstance(m, torch.Tensor) for m in meta)
        r = F.PreAct.restored(meta, saved)
        assert r.kind == d.kind and len(r.args) == len(args) and all(a is b for a, b in zip(r.args, args))


def test_preact_of_a_plain_tensor_and_of_a_placeholder():
    x = torch.zeros(3, 4)
    d = F._preact_of(x)
    assert d.kind == "f32" and d.args[0] is x
    z = F.PreAct("z16", torch.zeros((1, 2), dtype=torch.int16), None)
    n0 = F.Z16_HANDOFFS
    ph = F._preact_carrier(z)
    assert F.Z16_HANDOFFS == n0 + 1 and ph.shape == (1, 2) and ph.stride() == (0, 0)
    assert F._preact_of(ph, ("z16",)) is z and F.dense_preact(x) is x
    s = F.PreAct("s20", torch.zeros((1, 2), dtype=torch.int16), torch.zeros((1, 1), dtype=torch.uint8), None, 0.25)
    assert F._s20_of(F._preact_carrier(s)) is s.args and F._s20_of(ph) is None and F._s20_of(x) is None


def test_s20_dense_is_the_two_rounding_decode():
    S = np.array([[-2 ** 19, -65536, -1, 0], [32768, 65535, 65536, 2 ** 19 - 1]], dtype=np.int64)
    u = S & 0xFFFFF                                   # the 20-bit two's complement pattern
    lo = torch.from_numpy((u & 0xFFFF).astype(np.uint16).view(np.int16))
    nib = (u >> 16).astype(np.uint8)
    hi = torch.from_numpy(nib[:, 0::2] | (nib[:, 1::2] << 4))          # even column in the low nibble
    bias = np.array([0.3, -1.7, 1e-3, 123.456], dtype=np.float32)
    want = (S.astype(np.float32) * np.float32(0.25)).astype(np.float32)
    assert np.array_equal(F.PreAct("s20", lo, hi, None, 0.25).dense().numpy(), want)
    got = F.PreAct("s20", lo, hi, torch.from_numpy(bias), 0.25).dense()
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), (want + bias).astype(np.float32))
    ph = F._preact_carrier(F.PreAct("s20", lo, hi, torch.from_numpy(bias), 0.25))
    assert np.array_equal(F.dense_preact(ph).numpy(), (want + bias).astype(np.float32))


def test_z16_dense_at_the_int16_bounds():
    x = np.array([[32767, -32767, -32768, 0]], dtype=np.int16)
    bias = np.array([0.3, -1.7, 1e-3, 0.5], dtype=np.float32)
    assert np.array_equal(F.PreAct("z16", torch.from_numpy(x), None).dense().numpy(), x.astype(np.float32))
    got = F.PreAct("z16", torch.from_numpy(x), torch.from_numpy(bias)).dense()
    assert np.array_equal(got.numpy(), (x.astype(np.float32) + bias).astype(np.float32))


def test_c2d_refuses_every_compact_placeholder():
    for d, *_ in _preacts(True):
        if d.compact:
            with pytest.raises(RuntimeError, match="reads fp32 values"):
                F._c2d(F._preact_carrier(d))
            with pytest.raises(RuntimeError, match="reads fp32 values"):      # a kind the caller's entries lack
                F._preact_of(F._preact_carrier(d), tuple({"z16", "s20", "zq"} - {d.kind}))
    x = torch.zeros(3, 4)
    assert F._c2d(x) is x
    t = torch.zeros(4, 3).t()
    assert torch.equal(F._c2d(t), t) and F._c2d(t).is_contiguous()


def test_every_entry_name_is_in_the_header():
    from bnn_amd import _lib
    sigs = _lib.signatures()
    assert len(F._ENTRIES) == 27
    for (base, kind, mod), name in F._ENTRIES.items():
        assert name in sigs, (base, kind, mod, name)
        assert F._entry(base, F.PreAct(kind, None), mod) == name
    assert F._entry("bnn_bn_apply_pack", F.PreAct("s20", None), "_stoch") == "bnn_bn_apply_pack_stoch_s20"
    assert F._entry("bnn_bn_bwd_q6", F.PreAct("z16", None), "_pre") == "bnn_bn_bwd_q6_i16_pre"
    assert F._entry("bnn_bn_fwd_train", F.PreAct("f32", None), "_dropout") == "bnn_bn_dropout_fwd_train"
    assert F._entry("bnn_bn_fwd_train", F.PreAct("z16", None), "_dropout") == "bnn_bn_fwd_train_i16"
    assert F._entry("bnn_bn2d_bwd_stats", F.PreAct("zq", None)) == "bnn_bn2d_bwd_stats_q"


def test_take_semantics():
    a, b = F._placeholder((3, 64), "cpu"), F._placeholder((3, 64), "cpu")
    for attr in (F._Q6_ATTR, F._I8C_ATTR, F._C1BN_ATTR):
        F._attach(a, attr, 1, 2)
        assert getattr(a, attr) == (F._q6_key(a), 1, 2)               # the stored layout: (key, *payload)
        assert F._take(a, attr) == (1, 2) and F._take(a, attr) is None      # taken once
    n0 = F.Q6_HANDOFFS
    setattr(b, F._Q6_ATTR, (F._q6_key(a), "rows", "cols", "cs"))      # stale: keyed for another placeholder
    assert F._q6_take(b) is None and F.Q6_HANDOFFS == n0
    setattr(b, F._I8C_ATTR, (F._q6_key(a), "dg", "sc", "cs", "ds"))
    with pytest.raises(RuntimeError, match="stale int8 column-digit hand-off"):
        F._i8c_take(b)
    c = F._placeholder((2, 1, 4, 4), "cpu")
    setattr(c, F._C1BN_ATTR, (F._q6_key(a),) + tuple(range(12)))
    with pytest.raises(RuntimeError, match="stale conv1 / BatchNorm2d hand-off"):
        F._c1bn_take(c)
    F._attach(c, F._C1BN_ATTR, *range(12))
    bn = F._c1bn_take(c)
    assert (bn.zq, bn.zb, bn.zf, bn.dyp, bn.inv_n, bn.ht) == (0, 1, 2, 3, 10, 11) and tuple(bn) == tuple(range(12))


def test_take_required_mode():
    ph = F._placeholder((3, 64), "cpu")
    with pytest.raises(RuntimeError, match="lost its FP6 hand-off"):
        F._q6_take_required(ph)
    with pytest.raises(RuntimeError, match="lost its int8 column-digit hand-off"):
        F._i8c_take(ph)
    with pytest.raises(RuntimeError, match="lost its BatchNorm2d hand-off"):
        F._c1bn_take(F._placeholder((2, 1, 4, 4), "cpu"))
    with pytest.raises(RuntimeError, match="lost"):
        F._take(ph, "_bnn_test", lost="lost")
    assert F._take(ph, "_bnn_test") is None and F._q6_take(ph) is None           # not required: no payload, None
    setattr(ph, F._Q6_ATTR, (F._q6_key(F._placeholder((3, 64), "cpu")), "rows", "cols", "cs"))
    with pytest.raises(RuntimeError, match="lost its FP6 hand-off"):              # stale, and nothing to fall back on
        F._q6_take_required(ph)
    dense = torch.ones(1).expand(3, 4)              # stride 0, but a legitimate dense-valued gradient
    assert F._q6_take_required(dense) is None and F._i8c_take(dense) is None
    assert F._c1bn_take(torch.ones(1).expand(2, 1, 4, 4)) is None
    assert F._take(torch.ones(3, 4), "_bnn_test", lost="lost") is None
