"""GPU check of the binding's two calling forms: a tensor passed directly (the header-derived pointer
argtype takes its data_ptr()) and the same tensor through ptr() give the kernel the same pointers.  The
kernel is not under test, the marshalling is: bnn_sign_f32 on 1,024 floats."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_tensor_and_ptr_forms_launch_the_same_call():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from bnn_amd import _lib
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1024, generator=g)
    x[:8] = torch.tensor([0.0, -0.0, float("nan"), -float("nan"), 1.0, -1.0, float("inf"), -float("inf")])
    x = x.cuda()
    direct, wrapped = torch.full_like(x, 7.0), torch.full_like(x, 7.0)
    _lib.call("bnn_sign_f32", x, direct, x.numel(), _lib.stream())
    _lib.call("bnn_sign_f32", _lib.ptr(x), _lib.ptr(wrapped), x.numel(), _lib.stream())
    torch.cuda.synchronize()
    assert torch.equal(direct.view(torch.int32), wrapped.view(torch.int32))       # bit for bit
    # sign(0) = 0 (include/bnn.h), and a NaN gives 0 where Tensor.sign() would propagate it
    want = torch.sign(torch.nan_to_num(x, nan=0.0, posinf=float("inf"), neginf=-float("inf")))
    assert torch.equal(direct, want)
    with pytest.raises(ctypes.ArgumentError, match="const float\\* x"):
        _lib.call("bnn_sign_f32", x.view(torch.int32), direct, x.numel(), _lib.stream())
