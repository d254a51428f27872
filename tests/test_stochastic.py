"""CPU-side checks of stochastic binarization: the numpy restatement of the rule
(stoch_ref.py) is self-consistent, the C ABI declares and binds the stochastic entries and they reject
bad arguments before any launch, and the module-level plumbing that needs no GPU (seeds, attributes,
the CPU path of ``Binarize(t, 'stoch')``)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import stoch_ref as R
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "bnn.h")
ENTRIES = ["bnn_binarize_stoch_f32", "bnn_stoch_pack_i8", "bnn_stoch_pack_fp4", "bnn_stoch_pack_fp4_out",
           "bnn_bn_apply_pack_stoch", "bnn_bn_apply_pack_stoch_i16", "bnn_bn_apply_pack_stoch_s20"]


# ------------------------------------------------------------------ the rule
def test_rule_saturates_and_is_never_zero_except_nan():
    x = np.array([1.0, 1.5, np.inf, 3e38, -1.0, -1.5, -np.inf, -3e38], np.float32)
    for seed in (0, 1, 2 ** 63 + 12345, R.M64):
        s = R.binarize(np.tile(x, 4096), seed)
        assert np.array_equal(s.reshape(-1, 8), np.tile(np.sign(x), (4096, 1)))
    rng = np.random.default_rng(0)
    x = rng.uniform(-1.3, 1.3, 1 << 16).astype(np.float32)
    x[::97] = 0.0
    x[5::101] = -0.0
    x[7::103] = np.nan
    s = R.binarize(x, 99)
    assert np.array_equal(s == 0, np.isnan(x))
    assert set(np.unique(s[~np.isnan(x)])) == {-1.0, 1.0}


def test_rule_thresholds():
    # t = floor(p * 2^24) with p = fl((x + 1) / 2): 0 at x <= -1, 2^24 at x >= 1, 2^23 at +-0
    # (1 - 2^-24 already rounds to p = 1: the tie goes to the even mantissa)
    x = np.array([-2.0, -1.0, -0.0, 0.0, 0.5, 1.0, 2.0, np.nan, -1 + 2.0 ** -23, 1 - 2.0 ** -23, 1 - 2.0 ** -24],
                 np.float32)
    t = R.threshold(x)
    assert list(t) == [0, 0, 1 << 23, 1 << 23, 3 << 22, 1 << 24, 1 << 24, 0, 1, (1 << 24) - 1, 1 << 24]


def test_rule_at_zero_takes_exactly_half_the_hash_values():
    # x = 0: +1 iff (h >> 8) < 2^23, i.e. iff the top bit of h is clear -- exactly half of all 2^32
    # hash values; fmix32 is a bijection of the 32-bit words, so over a full period of the element
    # index each value occurs once.  Checked on the hash's own definition over a 2^20 window:
    h = R.hash32(1234, 1 << 20)
    s = R.binarize(np.zeros(1 << 20, np.float32), 1234)
    assert np.array_equal(s > 0, (h >> 31) == 0)
    # and fmix32's two multipliers are odd (each step is invertible)
    assert 0x85EBCA6B % 2 == 1 and 0xC2B2AE35 % 2 == 1 and 0x9E3779B1 % 2 == 1
    # 5 sigma on this window (sigma of the +1 fraction = 1 / (2 sqrt n))
    assert abs(float((s > 0).mean()) - 0.5) < 5 / (2 * np.sqrt(1 << 20))


def test_rule_counter_and_salt_change_the_mask():
    z = np.zeros(1 << 16, np.float32)
    a, b, c = R.binarize(z, 77), R.binarize(z, 77, ctr=1), R.binarize(z, R.site_seed(77, 1))
    for u, v in ((a, b), (a, c), (b, c)):
        assert abs(float((u == v).mean()) - 0.5) < 5 / (2 * np.sqrt(z.size))
    assert np.array_equal(R.binarize(z, 77, ctr=3), R.binarize(z, (77 + 3 * R.CTR_GOLDEN) & R.M64))


# ------------------------------------------------------------------ C ABI
def test_header_and_binding_declare_the_entries():
    from bnn_amd import _lib
    text = open(HEADER).read()
    declared = set(re.findall(r"^\s*int\s+(bnn_\w+)\(", text, re.M))
    for name in ENTRIES:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert ctypes.c_uint64 in _lib.SIGNATURES[name][1], name       # each takes the 64-bit seed
        assert hasattr(_lib.lib(), name), name


def test_entries_reject_bad_arguments_without_a_gpu():
    from bnn_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(256)
    assert L.bnn_binarize_stoch_f32(None, p, 4, 1, None) == -1
    assert b"bnn_binarize_stoch_f32" in L.bnn_last_error()
    assert L.bnn_binarize_stoch_f32(p, p, -1, 1, None) == -1
    assert L.bnn_stoch_pack_i8(p, 4, 100, 100, p, 100, None, 0, 1, None) == -1      # ldq not a multiple of 64
    assert b"bnn_stoch_pack_i8" in L.bnn_last_error()
    assert L.bnn_stoch_pack_i8(p, 4, 100, 100, None, 0, None, 0, 1, None) == -1      # neither output
    assert L.bnn_stoch_pack_fp4(p, 4, 100, 100, p, 64, None, 0, 0, 1, 0, None) == -1  # ldq4 not a multiple of 128
    assert L.bnn_stoch_pack_fp4(p, 4, 256, 256, p, 128, p, 64, 3, 1, 1, None) == -1   # qt_fmt out of range
    assert L.bnn_stoch_pack_fp4_out(p, 4, 256, p, 128, None, 0, 2, None, 1, 0, None) == -1   # no sout
    assert L.bnn_stoch_pack_fp4_out(p, 4, 256, p, 100, None, 0, 2, p, 1, 1, None) == -1      # bad ldq4
    assert L.bnn_bn_apply_pack_stoch(p, 4, 256, None, p, None, None, None, 1, p, 128, None, 0, 0, 1, 0, None) == -1
    assert b"bnn_bn_apply_pack_stoch" in L.bnn_last_error()
    assert L.bnn_bn_apply_pack_stoch(p, 4, 256, p, p, None, None, None, 2, p, 128, None, 0, 0, 1, 0, None) == -1
    assert L.bnn_bn_apply_pack_stoch_i16(p, None, 4, 192, p, p, None, None, None, p, 128, p, 128, 0, 1, None) == -1
    assert b"bnn_bn_apply_pack_stoch_i16" in L.bnn_last_error()
    assert L.bnn_bn_apply_pack_stoch_s20(p, None, None, 1.0, 4, 256, p, p, None, None, None, p, 128, p, 128, 0, 1,
                                         None) == -1
    assert b"bnn_bn_apply_pack_stoch_s20" in L.bnn_last_error()
    # empty inputs are accepted without a launch, as the deterministic entries accept them
    assert L.bnn_binarize_stoch_f32(p, p, 0, 1, None) == 0
    assert L.bnn_stoch_pack_i8(p, 0, 64, 64, p, 64, None, 0, 1, None) == 0


def test_functional_ops_refuse_cpu_tensors():
    from bnn_amd import functional as F
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.binarize_stochastic(torch.zeros(4), 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.stoch_pack(torch.zeros(2, 8), 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.stoch_pack_fp4(torch.zeros(2, 8), 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.binary_linear(torch.zeros(2, 8), torch.zeros(3, 8), stochastic=1)


# ------------------------------------------------------------------ seeds and modules
def test_stochastic_seed_scheme():
    from bnn_amd import functional as F
    torch.manual_seed(5)
    base = int(torch.randint(0, 2 ** 62, (1,)).item())
    torch.manual_seed(5)
    assert F.stochastic_seed(3) == R.site_seed(base, 3)
    torch.manual_seed(5)
    assert F.dropout_seed() == base                     # the dropout keeps the unsalted base
    a, b = F.stochastic_seed(1), F.stochastic_seed(1)   # one draw of the CPU generator per call
    assert a != b and 0 <= a < 2 ** 64
    with pytest.raises(ValueError):
        F.stochastic_seed(0)


def test_binarize_stoch_on_cpu_mutates_in_place():
    from bnn_amd.nn import Binarize
    torch.manual_seed(0)
    t = torch.rand(64, 33) * 2.6 - 1.3
    t[0, 0], t[0, 1] = 2.0, -2.0
    before = t.clone()
    r = Binarize(t, "stoch")
    # the CPU path keeps the reference's torch ops: the argument is overwritten in place (it ends as the
    # clamped probability, :15's add_/div_/add_/clamp_) and the +-1 draw is returned
    assert not torch.equal(t, before) and float(t.min()) >= 0.0 and float(t.max()) <= 1.0
    assert r.shape == t.shape and set(r.unique().tolist()) == {-1.0, 1.0}
    assert r[0, 0] == 1.0 and r[0, 1] == -1.0


def test_layers_and_nets_carry_the_mode():
    from bnn_amd import nets
    from bnn_amd.nn import BinarizeConv2d, BinarizeLinear
    assert BinarizeLinear.quant_mode == "det" and BinarizeConv2d.quant_mode == "det"
    assert BinarizeLinear.stoch_salt >= 1 and BinarizeConv2d.stoch_salt >= 1
    m = nets.SmallNet()
    assert [fc.quant_mode for fc in (m.fc1, m.fc2, m.fc3)] == ["det"] * 3
    m = nets.SmallNet(stochastic=True)
    assert [fc.quant_mode for fc in (m.fc1, m.fc2, m.fc3)] == ["det", "stoch", "stoch"]
    assert (m.fc2.stoch_salt, m.fc3.stoch_salt) == (2, 3)
    c = nets.BinCNN(stochastic=True)
    assert c.layer1[0].quant_mode == "det" and c.layer2[0].quant_mode == "stoch" and c.layer2[0].stoch_salt == 2
    assert nets.BinCNN().layer2[0].quant_mode == "det"
    fc = BinarizeLinear(8, 4)
    fc.quant_mode = "sometimes"
    with pytest.raises(ValueError, match="quant_mode"):
        fc(torch.zeros(2, 8))


def test_trainer_flag():
    from bnn_amd import trainer
    assert trainer.parse([]).stochastic is False
    assert trainer.parse(["--stochastic"]).stochastic is True
