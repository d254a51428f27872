"""CPU-side checks of the C-ABI library: it loads, exports every symbol include/bnn.h declares,
and rejects bad arguments without launching anything (no GPU needed for these)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "bnn.h")


def declared_symbols():
    text = open(HEADER).read()
    return sorted(set(re.findall(r"^\s*(?:int|int64_t|const char\*)\s+(bnn_\w+)\(", text, re.M)))


@pytest.fixture(scope="module")
def L():
    from bnn_amd import _lib
    return _lib.lib()


def test_header_declares_the_bound_signatures(L):
    """The binding is parsed from the header, and the parse is total: every ``bnn_*(`` left after the
    comments are stripped is a parsed declaration, and the library exports each of them."""
    from bnn_amd import _lib
    assert declared_symbols() == sorted(_lib.SIGNATURES)
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert len(re.findall(r"\bbnn_\w+\s*\(", text)) == len(_lib.SIGNATURES) == len(_lib.parse_header(text))
    for name in _lib.SIGNATURES:
        assert hasattr(L, name), name


@pytest.mark.parametrize("decl, what", [
    ("int bnn_f(const float* x, size_t n);", "unknown parameter type"),       # a scalar type the map lacks
    ("int bnn_f(const half* x, int64_t n);", "unknown pointee type"),
    ("int bnn_f(const float* x);\nvoid bnn_g(int32_t v);", "2 bnn_\\*\\( declarations, 1 parsed"),   # skipped
    ("int bnn_f(const float* x);\nint bnn_f(float* y);", "2 bnn_\\*\\( declarations, 1 parsed"),      # shadowed
])
def test_parser_raises_rather_than_skip(decl, what):
    from bnn_amd import _lib
    with pytest.raises(ValueError, match=what):
        _lib.parse_header(decl)


def test_missing_header_is_a_clear_error(monkeypatch, tmp_path):
    from bnn_amd import _lib
    monkeypatch.setattr(_lib, "_signatures", None)
    monkeypatch.setenv("BNN_HEADER", str(tmp_path / "nowhere.h"))
    with pytest.raises(RuntimeError, match="bnn.h not found at .*nowhere.h"):
        _lib.signatures()


def _kinds(name):
    """(restype, argument kinds) of a bound entry: scalars as their ctypes type, pointers as the tensor
    element they take ("f32*", "i8*" -- the sign is not part of the rule --, "any*")."""
    import torch
    from bnn_amd import _lib
    labels = {torch.float32: "f32*", torch.float64: "f64*", torch.int8: "i8*", torch.int16: "i16*",
              torch.int32: "i32*", torch.int64: "i64*"}
    res, args = _lib.SIGNATURES[name]
    out = []
    for a in args:
        if isinstance(a, _lib.Pointer):
            hit = [v for k, v in labels.items() if a.dtypes is not None and k in a.dtypes]
            assert len(hit) == (a.dtypes is not None), (name, a)
            out.append(hit[0] if hit else "any*")
        else:
            out.append(a)
    return res, out


I32, I64, U64, F32, F64, STREAM = (ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_float, ctypes.c_double,
                                   ctypes.c_void_p)

# written from include/bnn.h by hand; between them every kind of restype and parameter
ANCHORS = {
    "bnn_version": (I32, []),
    "bnn_last_error": (ctypes.c_char_p, []),
    "bnn_gemm_i8_kernel": (ctypes.c_char_p, [I32, I32, I64, I64, I64]),
    "bnn_bn_workspace": (I64, [I64, I64]),
    "bnn_bn_plan": (I32, [I64, I64, "i64*"]),
    "bnn_gemm_i8_affine": (I32, ["i8*", I64, I64, I32, "i8*", I64, I64, I32, "f32*", "f32*", "f32*", "i64*", "i64*",
                                 F64, "f32*", I64, I64, I64, I64, STREAM]),
    "bnn_stoch_pack_fp4": (I32, ["f32*", I64, I64, I64, "i8*", I64, "i8*", I64, I32, U64, I32, STREAM]),
    "bnn_sign_pack_bits": (I32, ["f32*", I64, I64, I64, "i32*", "i32*", I64, STREAM]),
    "bnn_gemm_fp4_bnstats": (I32, ["i8*", I64, "i8*", I64, "f32*", "f32*", "i16*", I64, "f32*", I64, I64, I64, F32,
                                   U64, "f64*", I64, STREAM]),
    "bnn_hinge_fwd": (I32, ["f32*", "i64*", "f32*", I64, I64, F32, I32, "f32*", "any*", I64, STREAM]),
    "bnn_adam_clamp_multi": (I32, [I32, "any*", "any*", "any*", "any*", "i64*", "i64*", "i32*", F32, F32, F32, F32,
                                   "f32*", "i64*", F32, STREAM]),
    "bnn_gemm_fp6_set_half": (I32, [I32, F64]),
}


@pytest.mark.parametrize("name", sorted(ANCHORS))
def test_parsed_signature_matches_the_handwritten_anchor(name):
    assert _kinds(name) == ANCHORS[name]


# every call below is bnn_sign_pack_i8 with ldq = 100: libbnn answers BNN_EINVAL before any launch, so a
# host tensor's address is never used
def _sign_pack(L, x, q, qt=None):
    return L.bnn_sign_pack_i8(x, 4, 100, 100, q, 100, qt, 0, None)


def test_wrong_dtype_tensor_is_refused_before_the_call(L):
    import torch
    x, q = torch.zeros(400), torch.zeros(400, dtype=torch.int8)
    with pytest.raises(ctypes.ArgumentError, match=r"bnn_sign_pack_i8.*`const float\* x`.*float32.*int16"):
        _sign_pack(L, x.to(torch.int16), q)
    with pytest.raises(ctypes.ArgumentError, match=r"bnn_sign_pack_i8.*`const float\* x`.*float32.*float64"):
        _sign_pack(L, x.double(), q)
    with pytest.raises(ctypes.ArgumentError, match=r"bnn_sign_pack_i8.*`int8_t\* q`.*int8.*float32"):
        _sign_pack(L, x, x)
    with pytest.raises(ctypes.ArgumentError, match=r"bnn_sign_pack_i8.*`int8_t\* qt`.*int8.*int16"):
        _sign_pack(L, x, q, q.to(torch.int16))
    # K = 63 is refused likewise (the existing bad-argument test's call)
    with pytest.raises(ctypes.ArgumentError, match=r"bnn_gemm_i8_affine.*`const int64_t\* row_off`.*int64.*int32"):
        L.bnn_gemm_i8_affine(q, 64, 0, 1, q, 64, 0, 1, None, None, None, torch.zeros(8, dtype=torch.int32), None, 0.0,
                             x, 8, 8, 8, 63, None)


def test_right_dtype_tensor_reaches_the_library(L):
    import torch
    x, q = torch.zeros(400), torch.zeros(400, dtype=torch.int8)
    for xx, qq in ((x, q), (torch.nn.Parameter(x), q), (x, q.view(torch.uint8))):    # the sign is not checked
        assert _sign_pack(L, xx, qq) == -1
        assert b"bnn_sign_pack_i8" in L.bnn_last_error()


def test_none_ptr_and_c_void_p_still_pass(L):
    import torch
    from bnn_amd import _lib
    x, q = torch.zeros(400), torch.zeros(400, dtype=torch.int8)
    buf = (ctypes.c_float * 400)()
    for xx in (_lib.ptr(x), ctypes.c_void_p(16), x.data_ptr(), buf, ctypes.byref(buf)):
        assert _sign_pack(L, xx, _lib.ptr(q), None) == -1
        assert b"bnn_sign_pack_i8" in L.bnn_last_error()
    assert _lib.ptr(None) is None
    assert _sign_pack(L, None, None) == -1


def test_library_exports_every_declared_symbol(L):
    for name in declared_symbols():
        assert hasattr(L, name), name


def test_version_and_error_string(L):
    assert L.bnn_version() >= 1
    assert isinstance(L.bnn_last_error(), bytes)


def test_bad_arguments_are_rejected_without_a_gpu(L):
    from bnn_amd import _lib
    # K not a multiple of 64 -> BNN_EINVAL before any launch
    rc = L.bnn_gemm_i8(ctypes.c_void_p(16), 64, 0, 1, ctypes.c_void_p(16), 64, 0, 1, None, None, None,
                       ctypes.c_void_p(16), 8, 8, 8, 63, None)
    assert rc == -1
    assert b"bad arguments" in L.bnn_last_error()
    # unsupported digit combination (1,3)
    rc = L.bnn_gemm_i8(ctypes.c_void_p(16), 64, 0, 1, ctypes.c_void_p(16), 64, 64 * 8, 3, None, None, None,
                       ctypes.c_void_p(16), 8, 8, 8, 64, None)
    assert rc == -1
    rc = L.bnn_sign_pack_i8(ctypes.c_void_p(16), 4, 100, 100, ctypes.c_void_p(16), 100, None, 0, None)
    assert rc == -1  # ldq must be a multiple of 64
    with pytest.raises(_lib.BnnError):
        _lib.call("bnn_quant_rows", None, 1, 1, 1, None, 64, 64, None, None)


def test_workspace_queries(L):
    assert L.bnn_quant_cols_workspace(65536, 8192) > 0
    assert L.bnn_conv2d_bwd_filter_workspace(4096, 16, 32, 5, 5, 1) > 0


def test_ops_refuse_cpu_tensors():
    import torch
    from bnn_amd import functional as F
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.sign(torch.zeros(4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.binary_linear(torch.zeros(2, 8), torch.zeros(3, 8))


def test_conv_bf3_plans_are_bank_conflict_free(L):
    """The bf16x3 conv backward kernels' LDS layouts for the BinCNN's conv2 (host-only plan query):
    the data kernel's pixel / weight pitches are 16 (mod 32) bf16 with one image row per pixel
    tile, the filter kernel's dY pitch likewise, and its shifted input copies are padded so the
    modelled B-fragment ds_read_b128 is conflict-free (4 LDS cycles; the plain layout put all five
    kw copies of a combo row on the same banks)."""
    out = (ctypes.c_int64 * 9)()
    assert L.bnn_conv_bf3_plan(4096, 16, 14, 14, 32, 5, 5, 1, 2, 1, 1, out) == 0
    ps, ws, rowt, lds_d, kd, cs, xl, lds_f, cyc = list(out)
    assert ps % 32 == 16 and ws % 32 == 16 and rowt == 1 and lds_d <= 160 * 1024
    assert kd % 32 == 16 and cs % 8 == 0 and xl % 8 == 0 and lds_f <= 160 * 1024
    assert cyc == 400
    # shapes neither kernel takes report -1
    assert L.bnn_conv_bf3_plan(4, 8, 9, 9, 8, 3, 3, 2, 1, 1, 1, out) == 0 and out[0] == -1 and out[4] == -1


def test_bn_dropin_rejects_cpu_and_non_2d_inputs():
    """bnn_amd.nn.BatchNorm1d raises for what it does not run on the GPU (no silent torch fallback)."""
    import pytest
    import torch
    from bnn_amd.nn import BatchNorm1d
    bn = BatchNorm1d(8)
    assert isinstance(bn, torch.nn.BatchNorm1d) and set(bn.state_dict()) == set(torch.nn.BatchNorm1d(8).state_dict())
    with pytest.raises(TypeError, match="float32 CUDA"):
        bn(torch.randn(4, 8))
