"""The hinge criteria (bnn_hinge_*, bnn_amd.nn.HingeLoss / SqrtHingeLoss / SqrtHingeLossFunction, the
trainer's --loss) as far as they can be checked without a GPU: the C ABI is declared, exported and
rejects bad arguments before any launch; functional.hinge_loss has no CPU fallback; on CPU tensors the
modules run the torch restatement of models/binarized_modules.py:20-54 -- mean(max(0, 1 - x*t)) and its
square, a tie (x*t == margin) counting as 0 with a zero gradient."""
import ctypes
import os

import pytest
import torch

from conftest import ROOT

NAMES = ("bnn_hinge_ok", "bnn_hinge_workspace", "bnn_hinge_fwd", "bnn_hinge_bwd")
M, C = 37, 10
TIES = ((0, 0), (5, 3), (17, 9), (36, 4))


@pytest.fixture(scope="module")
def L():
    from bnn_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def case():
    """(x, y, T): logits randn * 3, labels, and their +-1 one-vs-all target, with x = margin * T (an exact
    tie at margin 1) at TIES."""
    g = torch.Generator().manual_seed(11)
    x = torch.randn(M, C, generator=g) * 3.0
    y = torch.randint(0, C, (M,), generator=g)
    T = torch.where(y.unsqueeze(1) == torch.arange(C), 1.0, -1.0)
    for i, j in TIES:
        x[i, j] = T[i, j]
    return x, y, T


def test_header_declares_and_library_exports_the_hinge_entries(L):
    text = open(os.path.join(ROOT, "include", "bnn.h")).read()
    for name in NAMES:
        assert name + "(" in text, name
        assert hasattr(L, name), name


def test_workspace_and_class_counts(L):
    assert L.bnn_hinge_workspace(65536, 10) > 0
    assert L.bnn_hinge_ok(10) == 1
    assert L.bnn_hinge_ok(7) == 0


def test_bad_arguments_are_rejected_without_a_gpu(L):
    p = ctypes.c_void_p(16)           # fake non-null pointers: nothing may be launched or read
    big = 1 << 20

    def fwd(y, t, M, C, work_bytes):
        return L.bnn_hinge_fwd(p, y, t, M, C, 1.0, 0, p, p, work_bytes, None)

    for args in ((p, None, 64, 7, big),       # C = 7
                 (p, None, 0, 10, big),       # M = 0
                 (None, None, 64, 10, big),   # both targets null
                 (p, p, 64, 10, big),         # both targets set
                 (p, None, 64, 10, 0)):       # work_bytes = 0
        assert fwd(*args) == -1, args
        assert b"bnn_hinge_fwd: bad arguments" in L.bnn_last_error()
    assert L.bnn_hinge_fwd(p, p, None, 64, 10, 1.0, 2, p, p, big, None) == -1      # squared not 0 / 1
    assert L.bnn_hinge_bwd(p, None, None, 64, 10, 1.0, 0, p, p, None) == -1
    assert b"bnn_hinge_bwd: bad arguments" in L.bnn_last_error()


def test_functional_hinge_loss_refuses_cpu_tensors(case):
    from bnn_amd import functional as F
    x, y, T = case
    assert not F.hinge_loss_ok(x, y) and not F.hinge_loss_ok(x, T)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.hinge_loss(x, y)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.hinge_loss(x, T, squared=True)


def test_sqrt_hinge_forms_agree_on_cpu(case):
    from bnn_amd.nn import SqrtHingeLoss, SqrtHingeLossFunction
    from models.binarized_modules import SqrtHingeLoss as dropin
    assert dropin is SqrtHingeLoss
    x, y, T = case
    ref = float(torch.relu(1.0 - x.double() * T.double()).pow(2).mean())
    for got in (SqrtHingeLoss()(x, T), SqrtHingeLossFunction.apply(x, T), SqrtHingeLoss()(x, y)):
        assert abs(float(got) - ref) <= 1e-6 * abs(ref)


def test_hinge_labels_equal_the_one_vs_all_target_on_cpu(case):
    from bnn_amd.nn import HingeLoss
    x, y, T = case
    assert torch.equal(HingeLoss()(x, y), HingeLoss()(x, T))
    ref = float(torch.relu(1.0 - x.double() * T.double()).mean())
    assert abs(float(HingeLoss()(x, T)) - ref) <= 1e-6 * abs(ref)


def test_torch_path_takes_every_target_input_mul_takes(case):
    """Only int64 [M] against [M, C] logits is read as labels.  An int64 dense +-1 target (what
    F.one_hot builds) and the 1-D binary hinge go to ``input * target`` as they always did."""
    from bnn_amd.nn import HingeLoss, SqrtHingeLoss, SqrtHingeLossFunction
    x, y, T = case
    Ti = 2 * torch.nn.functional.one_hot(y, C) - 1
    assert Ti.dtype == torch.int64 and torch.equal(Ti.float(), T)
    assert torch.equal(HingeLoss()(x, Ti), torch.relu(1.0 - x * T).mean())
    assert torch.equal(HingeLoss()(x, Ti), HingeLoss()(x, T))
    assert torch.equal(SqrtHingeLoss()(x, Ti), SqrtHingeLoss()(x, T))
    a, b = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    SqrtHingeLossFunction.apply(a, Ti).backward()
    SqrtHingeLossFunction.apply(b, T).backward()
    assert torch.equal(a.grad, b.grad)
    x1, t1 = x[:, 0].contiguous(), Ti[:, 0].contiguous()              # 1-D binary hinge, int64 +-1 [M]
    assert torch.equal(HingeLoss()(x1, t1), torch.relu(1.0 - x1 * t1).mean())
    assert torch.equal(SqrtHingeLoss()(x1, t1), torch.relu(1.0 - x1 * t1).pow(2).mean())
    xd = x.double()                                                    # other dtypes too
    assert torch.equal(HingeLoss()(xd, T.double()), torch.relu(1.0 - xd * T.double()).mean())


@pytest.mark.parametrize("scale", [1.0, 3.0])
def test_sqrt_hinge_function_gradient_on_cpu(case, scale):
    from bnn_amd.nn import SqrtHingeLossFunction
    x, y, T = case
    h = torch.relu(1.0 - x.double() * T.double())
    ref = scale * (-2.0 * T.double() * h / x.numel())
    a = x.clone().requires_grad_(True)
    loss = SqrtHingeLossFunction.apply(a, T)
    (loss if scale == 1.0 else scale * loss).backward()
    assert (a.grad.double() - ref).abs().max().item() <= 1e-6 * ref.abs().max().item()
    for i, j in TIES:
        assert a.grad[i, j].item() == 0.0
    assert int((a.grad != 0).sum()) > 0


def test_trainer_loss_flag():
    from bnn_amd import trainer
    assert trainer.parse([]).loss == "ce"
    assert trainer.parse(["--loss", "sqhinge"]).loss == "sqhinge"
    assert trainer.parse(["--loss", "hinge"]).loss == "hinge"
    with pytest.raises(SystemExit):
        trainer.parse(["--loss", "nope"])
