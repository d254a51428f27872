"""ctypes binding of libbnn.so, derived from the C ABI's one declaration, include/bnn.h.

The library is the product: there is no CPU fallback.  Loading fails loudly when the .so or the
header is missing, and every op raises when handed a non-ROCm tensor.  Pointer parameters take
tensors directly and check their dtype against the pointee type the header declares.
"""
import ctypes
import os
import re

import torch  # load torch's HIP runtime first so libbnn binds to the same one

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libbnn.so")
DEFAULT_HEADER = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "bnn.h")

_RESTYPES = {"int": ctypes.c_int32, "int64_t": ctypes.c_int64, "const char*": ctypes.c_char_p}
_SCALARS = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
            "float": ctypes.c_float, "double": ctypes.c_double, "bnn_stream_t": ctypes.c_void_p}


def _ints(size):
    """The integer dtypes of one element size: the sign is not checked (uint32_t keep-bit planes are
    int32 tensors, FP4 bytes travel through int8_t* and uint8_t*)."""
    names = {1: ("int8", "uint8"), 2: ("int16", "uint16"), 4: ("int32", "uint32"), 8: ("int64", "uint64")}[size]
    return frozenset(getattr(torch, n) for n in names if hasattr(torch, n))


# pointee -> tensor dtypes a pointer to it takes (None: anything)
_POINTEES = {"float": frozenset({torch.float32}), "double": frozenset({torch.float64}),
             "int8_t": _ints(1), "uint8_t": _ints(1), "int16_t": _ints(2), "int32_t": _ints(4),
             "uint32_t": _ints(4), "int64_t": _ints(8), "void": None}


class Pointer:
    """argtype of one pointer parameter.  ctypes calls from_param per argument: a tensor is checked
    against the header's pointee type and passed as its data_ptr(); anything else (None, an int, a
    c_void_p, a ctypes array or byref) goes through c_void_p.from_param as before.  Host and device
    pointers are not told apart here (functional._check is the device check)."""
    __slots__ = ("entry", "decl", "dtypes")

    def __init__(self, entry, decl, dtypes):
        self.entry, self.decl, self.dtypes = entry, decl, dtypes

    def from_param(self, v):
        if isinstance(v, torch.Tensor):
            if self.dtypes is not None and v.dtype not in self.dtypes:
                raise TypeError(f"{self.entry}: parameter `{self.decl}` takes "
                                f"{' / '.join(sorted(str(d) for d in self.dtypes))}, got a {v.dtype} tensor")
            # a c_void_p, never the bare int: ctypes would marshal that as a 32-bit C int
            return ctypes.c_void_p(v.data_ptr())
        return ctypes.c_void_p.from_param(v)

    def __repr__(self):
        return f"Pointer({self.entry}: {self.decl})"


def _argtype(entry, decl):
    ctype, _name = re.fullmatch(r"(.*?)\s*(\w+)", decl).groups()
    if "*" not in ctype:
        if ctype not in _SCALARS:
            raise ValueError(f"bnn.h: {entry}: unknown parameter type in `{decl}`")
        return _SCALARS[ctype]
    pointee = ctype.replace("const", "").replace(" ", "")
    if pointee.count("*") > 1:          # arrays of pointers (the multi-tensor entries)
        return Pointer(entry, decl, None)
    if pointee[:-1] not in _POINTEES:
        raise ValueError(f"bnn.h: {entry}: unknown pointee type in `{decl}`")
    return Pointer(entry, decl, _POINTEES[pointee[:-1]])


def parse_header(text):
    """name -> (restype, [argtypes]) of every bnn_* declaration in the header's text.  Total: an
    unknown type or a declaration this did not parse raises."""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    sigs = {}
    for res, name, params in re.findall(r"\b(int|int64_t|const char\*)\s+(bnn_\w+)\s*\(([^)]*)\)\s*;", text):
        params = [" ".join(p.split()) for p in params.split(",")]
        sigs[name] = (_RESTYPES[res], [] if params == ["void"] else [_argtype(name, p) for p in params])
    seen = len(re.findall(r"\bbnn_\w+\s*\(", text))
    if seen != len(sigs):
        raise ValueError(f"bnn.h: {seen} bnn_*( declarations, {len(sigs)} parsed")
    return sigs


_lib = None
_signatures = None


def library_path():
    return os.environ.get("BNN_LIB", DEFAULT_PATH)


def header_path():
    return os.environ.get("BNN_HEADER", DEFAULT_HEADER)


def signatures():
    """The header's prototypes as ctypes signatures, parsed once."""
    global _signatures
    if _signatures is None:
        path = header_path()
        if not os.path.exists(path):
            raise RuntimeError(f"bnn.h not found at {path}: the binding is derived from it "
                               "(set BNN_HEADER if it lives elsewhere)")
        with open(path) as f:
            _signatures = parse_header(f.read())
    return _signatures


def __getattr__(name):
    if name == "SIGNATURES":
        return signatures()
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def lib():
    """Load libbnn.so once.  Raises RuntimeError (no fallback) if it is missing."""
    global _lib
    if _lib is None:
        path = library_path()
        if not os.path.exists(path):
            raise RuntimeError(
                f"libbnn.so not found at {path}: build it with "
                "`make -C distributed-mnist-bnns_amd/csrc` (or __graft_entry__.build()). "
                "The BNN hot path has no CPU fallback.")
        L = ctypes.CDLL(path)
        for name, (res, args) in signatures().items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


class BnnError(RuntimeError):
    pass


def call(name, *args):
    rc = getattr(lib(), name)(*args)
    if rc != 0:
        msg = lib().bnn_last_error().decode(errors="replace")
        raise BnnError(f"{name} failed (code {rc}): {msg}")
    return rc


def ptr(t):
    """Device pointer of a tensor (or NULL for None)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
