"""The flat and multi-tensor latent updates run one span (update_span, csrc/bnn_update.hip) for every
optimizer: float4 runs and a scalar tail when the weight and every state stream are 16-B aligned, scalar
throughout when one is not.  Both forms go through the same element, so the results must not depend on
alignment, on where the vector body ends, or on which kernel -- flat, multi-tensor, fused with the re-pack
-- ran the element:

* flat Adam: p, m, v bit-equal between aligned tensors and views one float past alignment (all of them, only
  p, only a state tensor), and bit-equal to one bnn_adam_clamp_pack of the same data as a 2-D weight; the
  per-launch form and the device-step (sched / ctr) form;
* flat SGD: p, buf bit-equal to the numpy restatement (tests/sgd_ref.py) at the same alignments, a first step
  (buffer pre-filled with NaN, written only) and a second;
* one multi-tensor launch of 16 tensors whose alignments differ: Adam bit-equal to one flat call per tensor,
  SGD to the restatement with mixed first and clamp flags.

Sizes: below, at and just above one float4, a vector body with a 3-element tail (1027), more than one pass of
the grid-stride loop's first block row (65536 + 3).  Every tensor sits between guard elements that must
survive: a run that went past an end would show.
"""
import numpy as np
import pytest
import torch

import sgd_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32
SIZES = [1, 3, 4, 5, 7, 1027, 65536 + 3]
GUARD = 4                    # floats kept on either side of every tensor
SENTINEL = -12345.0
LR, B1, B2, EPS, GSCALE = 0.01, 0.9, 0.999, 1e-8, 1.0 / 3.0
# offsets in floats past a 16-B aligned address of (p, g, first state tensor, second state tensor)
ALIGNMENTS = {"aligned": (0, 0, 0, 0), "offset": (1, 1, 1, 1), "p_only": (1, 0, 0, 0), "state_only": (0, 0, 0, 1),
              "first_state_only": (0, 0, 1, 0)}


@pytest.fixture(scope="module")
def F():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from bnn_amd import functional
    return functional


class Placed:
    """A device copy of ``a`` whose first element lies ``off`` floats past a 16-B aligned address, with GUARD
    sentinel floats before and after it."""

    def __init__(self, a, off):
        a = np.ascontiguousarray(a, F32)
        self.base = torch.full((a.size + 2 * GUARD + off,), SENTINEL, device="cuda")
        self.lo = GUARD + off
        self.t = self.base[self.lo:self.lo + a.size]
        self.t.copy_(torch.from_numpy(a))
        assert self.t.is_contiguous() and self.base.data_ptr() % 16 == 0
        assert a.size == 0 or (self.t.data_ptr() % 16 == 0) == (off % 4 == 0)

    def bits(self):
        """The values' bit patterns; asserts that the guards were left alone."""
        h = self.base.cpu().numpy()
        assert (h[:self.lo] == F32(SENTINEL)).all() and (h[self.lo + self.t.numel():] == F32(SENTINEL)).all(), \
            "written outside the tensor"
        return h[self.lo:self.lo + self.t.numel()].view(np.uint32)


def same(placed, a):
    return np.array_equal(placed.bits(), np.ascontiguousarray(a, F32).view(np.uint32))


def adam_data(n, seed):
    """p beyond +-1 in places (the clamp occurs), a state as after a few steps."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1.2, 1.2, n).astype(F32), rng.standard_normal(n).astype(F32),
            (rng.standard_normal(n) * 1e-3).astype(F32), (rng.random(n) * 1e-6).astype(F32))


def adam_flat(F, data, offs, step=3, clamp=True, **kw):
    p, g, m, v = (Placed(a, o) for a, o in zip(data, offs))
    F.adam_clamp_(p.t, g.t, m.t, v.t, step, LR, B1, B2, EPS, grad_scale=GSCALE, clamp=clamp, **kw)
    return p.bits(), m.bits(), v.bits()


def adam_pack(data, step=3):
    """One bnn_adam_clamp_pack of the same data as a [1][n] weight (int8 rows, no transpose)."""
    from bnn_amd import _lib as L
    p, g, m, v = (Placed(a, 0) for a in data)
    n = p.t.numel()
    ldq = (n + 63) // 64 * 64
    q = torch.empty((1, ldq), dtype=torch.int8, device="cuda")
    L.call("bnn_adam_clamp_pack", p.t, g.t, m.t, v.t, 1, n, LR, B1, B2, EPS, step, GSCALE, 1, 0, q, ldq, None, 0, 0,
           L.stream())
    assert np.array_equal(q[0, :n].cpu().numpy(), np.sign(p.t.cpu().numpy()).astype(np.int8))
    return p.bits(), m.bits(), v.bits()


@pytest.mark.parametrize("n", SIZES)
def test_flat_adam_does_not_depend_on_alignment_and_equals_the_pack(F, n):
    data = adam_data(n, 100 + n)
    want = adam_pack(data)
    assert not np.array_equal(want[0], data[0].view(np.uint32))           # the step moved p
    for name, offs in ALIGNMENTS.items():
        got = adam_flat(F, data, offs)
        for x, y, what in zip(got, want, "pmv"):
            assert np.array_equal(x, y), (name, what)
    if n >= 1027:
        assert (np.abs(want[0].view(F32)) == 1).any()                      # the clamp occurred


def test_flat_adam_device_step_form(F):
    """sched / ctr: the bias corrections of step 3 read from the device table equal the per-launch ones."""
    n = 1027
    data = adam_data(n, 5)
    want = adam_flat(F, data, ALIGNMENTS["aligned"], step=3)
    sched = F.adam_schedule(LR, B1, B2, 1, 8, "cuda")
    ctr = torch.tensor([2], dtype=torch.int64, device="cuda")              # table row 2 = step 3
    for name in ("aligned", "offset", "state_only"):
        got = adam_flat(F, data, ALIGNMENTS[name], step=999, sched=sched, ctr=ctr)
        for x, y, what in zip(got, want, "pmv"):
            assert np.array_equal(x, y), (name, what)


@pytest.fixture(scope="module")
def sgd_cases():
    """{(setting, n): (p0, g1, g2, (p1, buf1), (p2, buf2))}: the restatement's first and second step, once."""
    out = {}
    for si, setting in enumerate(R.SETTINGS):
        mu, damp, wd, nest = setting
        for n in SIZES:
            rng = np.random.default_rng(1000 * si + n)
            p0, g1, g2 = R.make_p0(n, rng), R.make_grad(n, rng), R.make_grad(n, rng)
            s1 = R.sgd_step(p0, g1, None, LR, mu, damp, wd, nest, True, GSCALE, True)
            s2 = R.sgd_step(s1[0], g2, s1[1], LR, mu, damp, wd, nest, False, GSCALE, True)
            out[setting, n] = (p0, g1, g2, s1, s2)
    return out


@pytest.mark.parametrize("setting", R.SETTINGS)
def test_flat_sgd_equals_restatement_at_every_alignment(F, sgd_cases, setting):
    mu, damp, wd, nest = setting
    for n in SIZES:
        p0, g1, g2, s1, s2 = sgd_cases[setting, n]
        for name, (po, go, bo, _) in ALIGNMENTS.items():
            p = Placed(p0, po)
            buf = Placed(np.full(n, np.nan, F32), bo) if mu != 0 else None      # first: never read
            for first, g, (p_ref, buf_ref) in ((True, g1, s1), (False, g2, s2)):
                F.sgd_clamp_(p.t, Placed(g, go).t, None if buf is None else buf.t, LR, mu, damp, wd, nest,
                             first=first, grad_scale=GSCALE, clamp=True)
                assert same(p, p_ref), (n, name, first)
                if mu != 0:
                    assert same(buf, buf_ref), (n, name, first)


# ------------------------------------------------------------------ one multi-tensor launch, mixed alignments
MULTI_SIZES = [1027, 4, 5, 255, 256, 257, 1023, 1024, 1025, 0, 7, 260, 3, 1, 252, 1028]
MULTI_OFFS = [(0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0), (2, 0, 0, 0), (0, 3, 0, 0), (0, 0, 0, 0), (0, 0, 1, 0),
              (0, 0, 0, 2)]


def test_multi_adam_equals_flat_per_tensor(F):
    assert len(MULTI_SIZES) == F.ADAM_MULTI_MAX
    items, placed, want = [], [], []
    for j, n in enumerate(MULTI_SIZES):
        data, step, clamp = adam_data(n, 40 + j), 1 + j % 5, j % 3 != 0
        want.append(adam_flat(F, data, ALIGNMENTS["aligned"], step=step, clamp=clamp))
        ts = [Placed(a, o) for a, o in zip(data, MULTI_OFFS[j % len(MULTI_OFFS)])]
        placed.append(ts)
        items.append((*[t.t for t in ts], step, clamp))
    F.adam_clamp_multi_(items, LR, B1, B2, EPS, grad_scale=GSCALE)
    for j, (ts, w) in enumerate(zip(placed, want)):
        for i, k, what in ((0, 0, "p"), (2, 1, "m"), (3, 2, "v")):
            assert np.array_equal(ts[i].bits(), w[k]), (j, what)
        assert np.array_equal(ts[1].bits(), adam_data(MULTI_SIZES[j], 40 + j)[1].view(np.uint32))     # g is only read


@pytest.mark.parametrize("setting", R.SETTINGS)
def test_multi_sgd_equals_restatement(F, setting):
    mu, damp, wd, nest = setting
    rng = np.random.default_rng(31)
    items, placed, want = [], [], []
    for j, n in enumerate(MULTI_SIZES):
        first, clamp = j % 3 == 0, j % 2 == 0
        po, go, bo, _ = MULTI_OFFS[j % len(MULTI_OFFS)]
        p0, g, b0 = R.make_p0(n, rng), R.make_grad(n, rng), (0.5 * R.make_grad(n, rng)).astype(F32)
        p, buf = Placed(p0, po), None
        if mu != 0:
            buf = Placed(np.full(n, np.nan, F32) if first else b0, bo)
        placed.append((p, buf))
        items.append((p.t, Placed(g, go).t, None if buf is None else buf.t, first, clamp))
        want.append(R.sgd_step(p0, g, b0, LR, mu, damp, wd, nest, first, GSCALE, clamp))
    F.sgd_clamp_multi_(items, LR, mu, damp, wd, nest, grad_scale=GSCALE)
    for j, ((p, buf), (p_ref, buf_ref)) in enumerate(zip(placed, want)):
        assert same(p, p_ref), j
        if mu != 0:
            assert same(buf, buf_ref), j
