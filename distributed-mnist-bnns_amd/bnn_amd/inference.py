"""Frozen-model inference for the binarized MLPs (nets.MLP and its Net / SmallNet / WideNet widths) and the
binarized CNN (nets.BinCNN -> FrozenCNN, described at that class).  ``_Frozen`` holds what the two share: the
state file, the device, the CPU / GPU dispatch with its buffer cache, refresh and the inference API.

``freeze(model)`` snapshots a trained network once -- fc1's int8 weight rows and their row sums, fc2
and fc3's FP4 weight rows, every bias, each BatchNorm's running mean / invstd / gamma / beta, fc4 --
and ``FrozenMLP.forward`` runs it without the float model or autograd:

    u8 pixels -> pixels_pack -> fc1 GEMM [BN1-sign epilogue] -> fc2 GEMM [BN2-sign epilogue]
              -> fc3 GEMM -> BN3 + Hardtanh + fc4 head on the running statistics -> log-softmax

In eval mode BatchNorm -> Hardtanh -> Binarize of the next layer is a per-column function of the
GEMM's sum (Hardtanh keeps the sign), so the hidden GEMMs write the next layer's FP4 operand from
their epilogue (bnn_gemm_i8_affine_bnsign, bnn_gemm_fp4_bnsign): 0.5 B per hidden activation and no
fp32 hidden activation at all.  The operands are bit-identical to ``model.eval()``'s GEMM +
bn_apply_pack pair; the head accumulates its logits in double.

The forward has no host synchronisation and keeps its buffers per batch size, so it can be captured
in ``torch.cuda.graph``.  On CPU tensors it runs a plain-torch restatement of the same layer math
(for checking a snapshot without a GPU; it is not a serving path).
"""
import torch
import torch.nn.functional as tF

from . import _lib as L
from . import functional as BF
from . import nets
from .metrics import Meter

__all__ = ["freeze", "from_state", "FrozenMLP", "FrozenCNN"]

FORMAT = "bnn_amd.frozen/1"
FORMAT_CNN = "bnn_amd.frozen_cnn/1"
_K1 = 28 * 28


def _tsign(w):
    """Ternary sign as libbnn's tsign(): int8 +1 / -1 / 0 (NaN -> 0)."""
    return (w > 0).to(torch.int8) - (w < 0).to(torch.int8)


def _pack_i8_rows(w):
    """[N, K] fp32 -> int8 sign rows [N, round_up(K, 64)] (the layout of bnn_sign_pack_i8)."""
    N, K = w.shape
    q = torch.zeros((N, BF.round_up(K)), dtype=torch.int8, device=w.device)
    q[:, :K] = _tsign(w)
    return q


def _pack_fp4_rows(w):
    """[N, K] fp32 -> FP4 sign rows [N, round_up(K, 256) / 2] (the layout of bnn_sign_pack_fp4: code
    0x2 / 0xA / 0x0, element k in byte k / 2, low nibble for even k)."""
    N, K = w.shape
    s = _tsign(w)
    code = torch.zeros((N, BF.round_up(K, 256)), dtype=torch.uint8, device=w.device)
    code[:, :K] = torch.where(s > 0, 2, torch.where(s < 0, 10, 0)).to(torch.uint8)
    return (code[:, 0::2] | (code[:, 1::2] << 4)).contiguous()


def _unpack_fp4_rows(q4, K):
    """FP4 sign rows -> int8 signs [rows, K]."""
    code = torch.stack((q4 & 15, q4 >> 4), dim=2).reshape(q4.shape[0], -1)[:, :K]
    return (code == 2).to(torch.int8) - (code == 10).to(torch.int8)


def _latent(p):
    """The latent value of a binarized layer's parameter: ``.org`` when the layer carries one."""
    return getattr(p, "org", p.data).detach()


def _pick_co(co):
    return 8 if co <= 8 else 16 if co <= 16 else 32 if co <= 32 else 64


def _pack_conv_rows(w):
    """[Co, C, KH, KW] (C % 16 == 0) -> int8 [round_up(Co, 16), KCp * 16]: the LDS image of libbnn's int8-MFMA
    conv, byte (kh KW + kw) C + c of row co = tsign(w[co, c, kh, kw]), KCp = round_up(KH KW C / 16, 4), zeros
    in every pad."""
    Co, C, KH, KW = w.shape
    kc = KH * KW * C // 16
    q = torch.zeros((BF.round_up(Co, 16), BF.round_up(kc, 4) * 16), dtype=torch.int8, device=w.device)
    q[:Co, :KH * KW * C] = _tsign(w).permute(0, 2, 3, 1).reshape(Co, KH * KW * C)
    return q


def _unpack_conv_rows(q, Co, C, KH, KW):
    return q[:Co, :KH * KW * C].reshape(Co, KH, KW, C).permute(0, 3, 1, 2).contiguous()


def _pack_conv_c1(w):
    """[Co, 1, KH, KW] (KW <= 8) -> int8 [KH, KWG, CO, 4] (KWG = 1 for KW <= 4 else 2, CO = 8 / 16 / 32 / 64):
    byte j of word (kh, g, co) = tsign(w[co, 0, kh, 4 g + j]), zero for 4 g + j >= KW and co >= Co -- the
    dot4 words of libbnn's single-channel conv."""
    Co, _, KH, KW = w.shape
    kwg = 1 if KW <= 4 else 2
    q = torch.zeros((KH, kwg * 4, _pick_co(Co)), dtype=torch.int8, device=w.device)
    q[:, :KW, :Co] = _tsign(w)[:, 0].permute(1, 2, 0)
    return q.reshape(KH, kwg, 4, -1).permute(0, 1, 3, 2).contiguous()


def _unpack_conv_c1(q, Co, KW):
    KH, kwg, CO, _ = q.shape
    return q.permute(0, 1, 3, 2).reshape(KH, kwg * 4, CO)[:, :KW, :Co].permute(2, 0, 1).unsqueeze(1).contiguous()


def pixel_sign_table(normalize=None):
    """int8 [256]: tsign of the fp32 value the data pipeline makes of each byte (ToTensor, then Normalize)."""
    return _tsign(BF.pixels_to_float(torch.arange(256, dtype=torch.uint8), normalize))


def _plain(v):
    """Tuples as lists, all the way down (what a state file holds)."""
    return [_plain(e) for e in v] if isinstance(v, (tuple, list)) else v


# The two networks take invstd from the running variance differently, and each is pinned bit for bit by
# tests: model.eval()'s BatchNorm1d pass (bn_apply_pack on bnn_amd.nn's vectors) uses the fp32 rsqrt, the
# BatchNorm2d pass (bnn_bn2d_fwd_eval) computes bn_invstd_k's double expression in the kernel.
def _invstd_rsqrt32(var, eps):
    """(var + eps).rsqrt() in fp32, as model.eval()'s BatchNorm1d pass."""
    return (var.detach().float() + eps).rsqrt()


def _invstd(var, eps):
    """bit-identical to libbnn's bn_invstd_k: float(1 / sqrt(double(var) + double(float32(eps))))."""
    e = float(torch.tensor(eps, dtype=torch.float32))
    return (1.0 / torch.sqrt(var.detach().double().cpu() + e)).float().to(var.device)


def _snapshot_bn(t, i, bn, invstd, name):
    """t["bn<i>.mean / var / invstd / gamma / beta"] of a BatchNorm's running statistics."""
    if bn.running_mean is None or bn.running_var is None:
        raise ValueError(f"freeze: {name} keeps no running statistics (track_running_stats=False); "
                         "a frozen network needs them")
    t[f"bn{i}.mean"] = bn.running_mean.detach().float().clone()
    t[f"bn{i}.var"] = bn.running_var.detach().float().clone()
    t[f"bn{i}.invstd"] = invstd(bn.running_var, bn.eps)
    if bn.weight is not None:
        t[f"bn{i}.gamma"] = bn.weight.detach().float().clone()
    if bn.bias is not None:
        t[f"bn{i}.beta"] = bn.bias.detach().float().clone()


def _bn_y_cpu(f, mean, invstd, gamma, beta):
    """fmaf((f - mean) * invstd, gamma, beta) as the kernels form it (bn_y1): the product and sum in double
    are exact, so rounding them once is the fmaf."""
    g = gamma.double() if gamma is not None else 1.0
    b = beta.double() if beta is not None else 0.0
    return (((f - mean) * invstd).double() * g + b).float()


class _Frozen:
    """What a frozen network is apart from its layers: packed tensors ``t`` plus the metadata fields META,
    their state file, the device, the CPU / GPU dispatch with per-batch buffers, and the inference API.  A
    subclass gives FORMAT, META, OUT (the classifier weight's key), _snapshot, _input, _alloc, _forward_gpu,
    _hidden_gpu and _forward_cpu."""
    _FORMS = {"widths": lambda v: tuple(int(h) for h in v),
              "layers": lambda v: [tuple(int(e) for e in l) for l in v],        # per conv (C, Co, KH, KW, pad)
              "in_hw": lambda v: (int(v[0]), int(v[1])),
              "normalize": lambda v: None if v is None else (float(v[0]), float(v[1])),
              "eps": lambda v: tuple(float(e) for e in v)}

    def __init__(self, meta, tensors, model=None):
        self._load(meta, tensors)
        self._model = model
        self.two_pass = False     # True: every layer as GEMM / conv + its BatchNorm pass (A/B and cross-checks)

    def _load(self, meta, tensors):
        for k in self.META:
            setattr(self, k, self._FORMS[k](meta[k]))
        self.t = dict(tensors)
        self._buf = {}

    def refresh(self):
        """Re-snapshot the model this was frozen from (after more training); ``two_pass`` stays."""
        if self._model is None:
            raise RuntimeError(f"{type(self).__name__}.refresh: this snapshot was loaded from a state, "
                               "not frozen from a model")
        self._load(*self._snapshot(self._model, self.normalize))
        return self

    # ------------------------------------------------------------------ persistence
    def state_dict(self):
        """Tensors, numbers and strings only (torch.load(weights_only=True) reads it back)."""
        return {"format": self.FORMAT, **{k: _plain(getattr(self, k)) for k in self.META},
                "tensors": {k: v.detach().clone() for k, v in self.t.items()}}

    @classmethod
    def from_state(cls, state, device=None):
        if state.get("format") != cls.FORMAT:
            raise ValueError(f"{cls.__name__}.from_state: not a {cls.FORMAT} state (format={state.get('format')!r})")
        t = {k: (v.to(device) if device is not None else v.clone()) for k, v in state["tensors"].items()}
        return cls(state, t)

    def to(self, device):
        self.t = {k: v.to(device) for k, v in self.t.items()}
        self._buf = {}
        return self

    @property
    def device(self):
        return self.t[self.OUT].device

    # ------------------------------------------------------------------ forward
    def _bn(self, i):
        t = self.t
        return t[f"bn{i}.mean"], t[f"bn{i}.invstd"], t.get(f"bn{i}.gamma"), t.get(f"bn{i}.beta")

    def _buffers(self, M, device):
        key = (M, str(device))
        b = self._buf.get(key)
        if b is None:
            b = self._buf[key] = self._alloc(M, device)
        return b

    def _run(self, x):
        """(log-probabilities, the hidden layers' record) of inputs ``_input`` has checked."""
        if not x.is_cuda:
            return self._forward_cpu(x)
        if self.device != x.device:
            raise RuntimeError(f"{type(self).__name__} on {self.device} got an input on {x.device}; call .to(device)")
        return self._forward_gpu(x, self._buffers(x.shape[0], x.device))

    def forward(self, x):
        """log-probabilities [M, 10] of u8 pixels (the Normalize frozen with the model applied) or fp32 images."""
        return self._run(self._input(x))[0]

    __call__ = forward

    def hidden_signs(self, x):
        """int8 signs the hidden layers hand on (what exactly: the subclass's _hidden_gpu)."""
        x = self._input(x)
        hidden = self._run(x)[1]
        return self._hidden_gpu(hidden) if x.is_cuda else hidden

    def predict(self, x):
        """int64 class labels [M]."""
        return self.forward(x).argmax(dim=1)

    def accuracy(self, x, labels, batch=4096):
        """Fraction of ``labels`` predicted, run in batches of ``batch`` (one host read at the end)."""
        n = x.shape[0]
        if n == 0:
            return float("nan")
        hits = torch.zeros((), dtype=torch.int64, device=x.device)
        for i in range(0, n, batch):
            hits += (self.predict(x[i:i + batch]) == labels[i:i + batch].to(x.device)).sum()
        return float(hits.item()) / n

    def evaluate(self, x, labels, k=5, batch=4096):
        """The held-out metrics of a test loop over (x, labels), run in batches of ``batch``: ``forward`` and one
        metrics launch per batch into one device accumulator, one host read at the end.  Returns
        ``metrics.Meter.result()``: {"n", "loss" (mean cross-entropy), "prec1", "preck" (percent), "k" (clipped
        to the class count), "confusion" (int64 [C, C], row = label)}.  CPU tensors run the plain-torch
        restatements of both."""
        meter = Meter(self.t[self.OUT].shape[0], k=k, device=x.device)
        for i in range(0, x.shape[0], batch):
            meter.update(self.forward(x[i:i + batch]), labels[i:i + batch].to(device=x.device, dtype=torch.int64))
        return meter.result()


class FrozenMLP(_Frozen):
    """A frozen nets.MLP: packed tensors plus widths and the pixel Normalize.  See the module doc.
    ``hidden_signs``: sign(hardtanh(bn_i(z_i))) of the two hidden layers feeding fc2 / fc3, int8 [M, h_i]."""
    FORMAT = FORMAT
    META = ("widths", "normalize", "eps")
    OUT = "fc4.weight"

    # ------------------------------------------------------------------ snapshot
    @staticmethod
    def _snapshot(model, normalize=None):
        if not isinstance(model, nets.MLP):
            raise TypeError("freeze: expects a bnn_amd.nets.MLP (Net / SmallNet / WideNet)")
        t = {}
        bns = (model.bn1, model.bn2, model.bn3)
        for i, bn in enumerate(bns, 1):
            _snapshot_bn(t, i, bn, _invstd_rsqrt32, f"bn{i}")
        w1 = _latent(model.fc1.weight).float()
        if w1.shape[1] != _K1:
            raise ValueError("freeze: fc1 must take 784 pixels")
        t["fc1.q"] = _pack_i8_rows(w1)
        t["fc1.rowsum"] = t["fc1.q"][:, :_K1].sum(dim=1, dtype=torch.int64)
        t["fc2.q4"] = _pack_fp4_rows(_latent(model.fc2.weight).float())
        t["fc3.q4"] = _pack_fp4_rows(_latent(model.fc3.weight).float())
        for i, fc in enumerate((model.fc1, model.fc2, model.fc3), 1):
            if fc.bias is not None:
                # (bias.org is the reference's per-forward clone of the same value)
                t[f"fc{i}.bias"] = fc.bias.detach().float().clone()
        t["fc4.weight"] = model.fc4.weight.detach().float().contiguous().clone()
        if model.fc4.bias is not None:
            t["fc4.bias"] = model.fc4.bias.detach().float().clone()
        return {"widths": (model.fc1.out_features, model.fc2.out_features, model.fc3.out_features),
                "normalize": model.fc1.pixel_normalize, "eps": [bn.eps for bn in bns]}, t

    # ------------------------------------------------------------------ forward
    def _input(self, x):
        if x.dim() > 2:
            x = x.reshape(x.shape[0], -1)
        if x.dim() != 2 or x.shape[1] != _K1:
            raise ValueError(f"FrozenMLP: expects [M, 784] or [M, 1, 28, 28] inputs (got {tuple(x.shape)})")
        if x.dtype not in (torch.uint8, torch.float32):
            raise TypeError(f"FrozenMLP: uint8 pixels or float32 images (got {x.dtype})")
        return x

    # ---- GPU
    def _alloc(self, M, device):
        h1, h2, _ = self.widths
        return {"q": torch.empty((M, BF.round_up(_K1)), dtype=torch.int8, device=device),
                "a1": torch.empty((M, BF.round_up(h1, 256) // 2), dtype=torch.uint8, device=device),
                "a2": torch.empty((M, BF.round_up(h2, 256) // 2), dtype=torch.uint8, device=device),
                "y4": torch.empty((M, BF.HEAD_NOUT), dtype=torch.float32, device=device)}

    def _hidden_gpu(self, b):
        return [_unpack_fp4_rows(b["a1"], self.widths[0]), _unpack_fp4_rows(b["a2"], self.widths[1])]

    def _apply_pack(self, z, i, out):
        """The two-pass form's second pass: z fp32 -> FP4 rows of sign(BN_i(z)) (bnn_bn_apply_pack)."""
        mean, invstd, gamma, beta = self._bn(i)
        M, C = z.shape
        L.call("bnn_bn_apply_pack", z, M, C, mean, invstd, None, gamma, beta, 1, out, out.shape[1], None, 0, 0,
               L.stream())
        return out

    def _forward_gpu(self, x, b):
        t = self.t
        h1, h2, h3 = self.widths
        M = x.shape[0]
        w4, b4 = t["fc4.weight"], t.get("fc4.bias")
        if M == 0:
            return torch.empty((0, w4.shape[0]), dtype=torch.float32, device=x.device), b
        wq = t["fc1.q"]
        mean1, invstd1, g1, be1 = self._bn(1)
        if x.dtype == torch.float32 and self.normalize is None and not torch.cuda.is_current_stream_capturing():
            u = BF.unit_to_pixels(x)          # ToTensor images are their bytes (one host read, as fc1's)
            x = u if u is not None else x
        if x.dtype == torch.uint8:
            x = x if x.is_contiguous() else x.contiguous()
            L.call("bnn_pixels_pack", x, M, _K1, _K1, b["q"], b["q"].shape[1], None, 0, L.stream())
            a, s0 = BF.pixel_affine(self.normalize)
            bscale = BF._const_vec(a, h1, x.device)
            if BF.bnsign_ok(h1) and not self.two_pass:
                a1 = BF.gemm_i8_affine_bnsign(b["q"], wq, M, h1, bscale, t.get("fc1.bias"), t["fc1.rowsum"], s0,
                                              mean1, invstd1, g1, be1, k_true=_K1, out=b["a1"])
            else:
                z1 = BF.gemm_i8_affine(b["q"], 1, wq, 1, M, h1, b_scale=bscale, bias=t.get("fc1.bias"),
                                       col_off=t["fc1.rowsum"], off_mul=s0, k_true=_K1, label="pixels")
                a1 = self._apply_pack(z1, 1, b["a1"])
        else:
            # fp32 images that are not plain ToTensor bytes (already normalised, or arbitrary floats):
            # fc1 on the fp32 digit GEMM as BinarizeLinear runs it, then the apply-pack pass
            xd, sx = BF.quant_rows(x)
            z1 = BF.gemm_i8(xd, 3, wq, 1, M, h1, a_scale=sx, bias=t.get("fc1.bias"), k_true=_K1)
            a1 = self._apply_pack(z1, 1, b["a1"])
        mean2, invstd2, g2, be2 = self._bn(2)
        if BF.bnsign_ok(h2) and not self.two_pass:
            a2 = BF.gemm_fp4_bnsign(a1, t["fc2.q4"], M, h2, t.get("fc2.bias"), mean2, invstd2, g2, be2, k_true=h1,
                                    out=b["a2"])
        else:
            a2 = self._apply_pack(BF.gemm_fp4(a1, t["fc2.q4"], M, h2, bias=t.get("fc2.bias"), k_true=h1), 2, b["a2"])
        mean3, invstd3, g3, be3 = self._bn(3)
        fused = BF.head_eval_fusable(h3, w4.shape[1], w4.shape[0])
        if fused and "fc3.bias" in t and BF.z16_ok(M, h3, h2):
            z3 = (BF.gemm_fp4_i16(a2, t["fc3.q4"], M, h3, k_true=h2), t["fc3.bias"])
        else:
            z3 = BF.gemm_fp4(a2, t["fc3.q4"], M, h3, bias=t.get("fc3.bias"), k_true=h2)
        if fused:
            logits = BF.bn_head_eval(z3, mean3, invstd3, g3, be3, w4, b4, out=b["y4"])
        elif h3 % 4 == 0:
            logits = BF.bn_linear_eval(z3, mean3, t["bn3.var"], self.eps[2], g3, be3, w4, b4)
        else:       # a width libbnn's BatchNorm passes do not take (as nets.MLP: torch's modules)
            y = tF.batch_norm(z3, mean3, t["bn3.var"], g3, be3, False, 0.0, self.eps[2])
            logits = tF.linear(tF.hardtanh(y), w4, b4)
        return tF.log_softmax(logits, dim=1), b

    # ---- CPU restatement
    def _forward_cpu(self, x):
        t = self.t
        h1, h2, h3 = self.widths
        w1 = t["fc1.q"][:, :_K1].double()
        if x.dtype == torch.uint8:
            a, s0 = BF.pixel_affine(self.normalize)
            a32 = torch.tensor(a, dtype=torch.float32).double()
            S = (x.double() - 128.0) @ w1.t() + s0 * t["fc1.rowsum"].double()      # exact integers (+ s0 R)
            z = (S * a32).float()
        else:
            z = (x.double() @ w1.t()).float()
        signs = []
        for i, K in ((1, None), (2, h1), (3, h2)):
            if K is not None:
                z = (signs[-1].double() @ _unpack_fp4_rows(t[f"fc{i}.q4"], K).double().t()).float()
            if f"fc{i}.bias" in t:
                z = z + t[f"fc{i}.bias"]
            if i < 3:
                signs.append(_tsign(_bn_y_cpu(z, *self._bn(i))))
        mean3, invstd3, g3, be3 = self._bn(3)
        y = (z - mean3) * invstd3
        if g3 is not None:
            y = y * g3
        if be3 is not None:
            y = y + be3
        logits = tF.linear(tF.hardtanh(y), t["fc4.weight"], t.get("fc4.bias"))
        return tF.log_softmax(logits, dim=1), signs


class FrozenCNN(_Frozen):
    """A frozen nets.BinCNN: per conv layer the packed sign weights, bias and the BatchNorm2d's running
    mean / var / invstd / gamma / beta; the classifier; the 256-entry pixel sign table.

        u8 pixels -> conv1 [BN-sign-pool epilogue] -> int8 signs [N, 14, 14, 16]
                  -> conv2 [BN-pool-Linear epilogue] -> logits -> log-softmax

    Hardtanh and MaxPool2d are monotone, so the next layer's operand sign(maxpool(hardtanh(bn(z)))) is the
    window maximum of sign(bn(z)): the hidden layer writes 1 B per pooled element and no fp32 map
    (bnn_conv2d_fwd_bnsign_pool), the last one goes straight to the logits (bnn_conv2d_fwd_bn_pool_linear,
    sums in double).  ``two_pass = True`` runs every layer as conv + bnn_bn2d_fwd_eval (+ linear_nsmall /
    F.linear), the form ``model.eval()`` runs; a layer whose shape the fused kernels do not take falls back
    to it by itself.  No host synchronisation, buffers kept per batch size (graph capture works); CPU
    tensors run a plain-torch restatement (a checking path).  ``hidden_signs``: layer 1's pooled signs
    sign(maxpool(hardtanh(bn1(conv1(x))))), int8 NCHW [N, Co, H/2, W/2]."""
    FORMAT = FORMAT_CNN
    META = ("layers", "in_hw", "normalize", "eps")
    OUT = "fc.weight"

    # ------------------------------------------------------------------ snapshot
    @staticmethod
    def _snapshot(model, normalize):
        if not isinstance(model, nets.BinCNN):
            raise TypeError("freeze: expects a bnn_amd.nets.BinCNN")
        from .nn import BinarizeConv2d
        import torch.nn as tnn
        t, layers, eps = {}, [], []
        for i, seq in enumerate((model.layer1, model.layer2), 1):
            ok = (isinstance(seq, tnn.Sequential) and len(seq) == 4 and isinstance(seq[0], BinarizeConv2d)
                  and isinstance(seq[1], tnn.BatchNorm2d) and isinstance(seq[2], tnn.Hardtanh)
                  and seq[2].min_val == -1.0 and seq[2].max_val == 1.0 and isinstance(seq[3], tnn.MaxPool2d))
            if ok:
                pool = seq[3]
                pair = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)
                ok = (pair(pool.kernel_size) == (2, 2) and pair(pool.stride) == (2, 2) and pair(pool.padding) == (0, 0)
                      and pair(pool.dilation) == (1, 1) and not pool.ceil_mode)
            if not ok:
                raise ValueError(f"freeze: layer{i} must be BinarizeConv2d -> BatchNorm2d -> Hardtanh(-1, 1) -> "
                                 "MaxPool2d(2, 2) without padding or ceil_mode (the sign commutes with exactly that)")
            conv, bn = seq[0], seq[1]
            if (tuple(conv.stride) != (1, 1) or tuple(conv.dilation) != (1, 1) or conv.groups != 1
                    or conv.padding[0] != conv.padding[1] or conv.in_channels == 3):
                raise ValueError(f"freeze: layer{i}'s convolution must have stride 1, dilation 1, one group, square "
                                 "padding and a binarised input (in_channels != 3)")
            w = _latent(conv.weight).float()
            Co, C, KH, KW = w.shape
            layers.append((C, Co, KH, KW, conv.padding[0]))
            t[f"conv{i}.sign"] = _tsign(w)
            if C == 1 and KW <= 8:
                t[f"conv{i}.wq"] = _pack_conv_c1(w)
            elif C % 16 == 0:
                t[f"conv{i}.wq"] = _pack_conv_rows(w)
            if conv.bias is not None:
                t[f"conv{i}.bias"] = conv.bias.detach().float().clone()
            _snapshot_bn(t, i, bn, _invstd, f"layer{i}'s BatchNorm2d")
            eps.append(bn.eps)
        if layers[0][0] != 1:
            raise ValueError("freeze: the first convolution must take one-channel images")
        t["fc.weight"] = model.fc.weight.detach().float().contiguous().clone()
        if model.fc.bias is not None:
            t["fc.bias"] = model.fc.bias.detach().float().clone()
        t["pixel.table"] = pixel_sign_table(normalize).to(t["fc.weight"].device)
        return {"layers": layers, "in_hw": (28, 28), "normalize": normalize, "eps": eps}, t

    # ------------------------------------------------------------------ forward
    def _input(self, x):
        H, W = self.in_hw
        if x.dim() == 2 and x.shape[1] == H * W:
            x = x.reshape(x.shape[0], 1, H, W)
        if x.dim() != 4 or tuple(x.shape[1:]) != (1, H, W):
            raise ValueError(f"FrozenCNN: expects [N, {H * W}] or [N, 1, {H}, {W}] inputs (got {tuple(x.shape)})")
        if x.dtype not in (torch.uint8, torch.float32):
            raise TypeError(f"FrozenCNN: uint8 pixels or float32 images (got {x.dtype})")
        return x

    # ---- GPU
    def _shapes(self):
        """Per layer (C, Co, K.., pad, H, W, PH, PW) along the net."""
        H, W = self.in_hw
        out = []
        for C, Co, KH, KW, pad in self.layers:
            OH, OW = H + 2 * pad - KH + 1, W + 2 * pad - KW + 1
            out.append((C, Co, KH, KW, pad, H, W, OH // 2, OW // 2))
            H, W = OH // 2, OW // 2
        return out

    def _alloc(self, N, device):
        b = {"y": torch.empty((N, self.t["fc.weight"].shape[0]), dtype=torch.float32, device=device)}
        for i, (C, Co, KH, KW, pad, H, W, PH, PW) in enumerate(self._shapes()[:-1], 1):
            b[f"a{i}"] = torch.empty((N, PH, PW, BF.round_up(Co, 16)), dtype=torch.int8, device=device)
        return b

    def _hidden_gpu(self, hidden):
        cur, form, Co = hidden
        return cur[..., :Co].permute(0, 3, 1, 2).contiguous() if form == "s8" else _tsign(cur)

    def _wf(self, i):
        """fp32 sign weights of layer i for the two-pass form's conv (its kernel takes a latent fp32 weight)."""
        k = f"conv{i}.wf"
        w = self._buf.get(k)
        if w is None or w.device != self.t[f"conv{i}.sign"].device:
            w = self._buf[k] = self.t[f"conv{i}.sign"].float().contiguous()
        return w

    def _two_pass_layer(self, i, x, shp):
        """Layer i as model.eval() runs it: conv (binarising x, fp32 NCHW) -> bnn_bn2d_fwd_eval with Hardtanh and
        the 2x2 pool -> fp32 pooled map."""
        C, Co, KH, KW, pad, H, W, PH, PW = shp
        N = x.shape[0]
        z = BF.binary_conv2d(x, self._wf(i), self.t.get(f"conv{i}.bias"), True, 1, pad, 1, 1)
        y = torch.empty((N, Co, PH, PW), dtype=torch.float32, device=x.device)
        ws = torch.empty((L.lib().bnn_bn2d_workspace(N, Co),), dtype=torch.uint8, device=x.device)
        mean, _, gamma, beta = self._bn(i)
        L.call("bnn_bn2d_fwd_eval", z, N, Co, z.shape[2], z.shape[3], gamma, beta, mean, self.t[f"bn{i}.var"],
               float(self.eps[i - 1]), y, 1, 2, ws, L.stream())
        return y

    def _as_form(self, cur, form, want, C):
        """An activation of C channels from one of its three forms to another: u8 pixels, f32 (NCHW, what a
        layer binarises) and s8 (int8 signs, channels innermost and padded to a multiple of 16)."""
        if form == want:
            return cur
        if form == "u8":
            cur = BF.pixels_to_float(cur, self.normalize)
        if want == "f32":
            return cur if form == "u8" else cur[..., :C].permute(0, 3, 1, 2).float().contiguous()
        N, _, H, W = cur.shape
        a = torch.zeros((N, H, W, BF.round_up(C, 16)), dtype=torch.int8, device=cur.device)
        a[..., :C] = _tsign(cur).permute(0, 2, 3, 1)
        return a

    def _forward_gpu(self, x, b):
        t = self.t
        N = x.shape[0]
        n_out = t["fc.weight"].shape[0]
        if N == 0:
            return torch.empty((0, n_out), dtype=torch.float32, device=x.device), None
        x = x if x.is_contiguous() else x.contiguous()
        shapes = self._shapes()
        cur, form = x, ("u8" if x.dtype == torch.uint8 else "f32")
        hidden = None
        for i, shp in enumerate(shapes, 1):
            C, Co, KH, KW, pad, H, W, PH, PW = shp
            last = i == len(shapes)
            mean, invstd, gamma, beta = self._bn(i)
            wq, bias = t.get(f"conv{i}.wq"), t.get(f"conv{i}.bias")
            geo = (N, C, H, W, Co, KH, KW, 1, pad, 1, 1)
            xfmt = {"f32": 0, "u8": 1, "s8": 2}[form]
            # fused, or two-pass where the fused kernel does not take the layer (or two_pass asks for it)
            if self.two_pass or wq is None:
                fused = False
            elif last:
                fused = (C % 16 == 0 and t["fc.weight"].shape[1] == Co * PH * PW
                         and L.lib().bnn_conv2d_fwd_bn_pool_linear_ok(*geo, n_out) == 1)
            else:
                fused = L.lib().bnn_conv2d_fwd_bnsign_pool_ok(xfmt, *geo) == 1
            want = "f32" if not fused else "s8" if last else form
            cur, form = self._as_form(cur, form, want, C), want
            if fused and last:
                L.call("bnn_conv2d_fwd_bn_pool_linear", cur, wq, bias, mean, invstd, gamma, beta, t["fc.weight"],
                       t.get("fc.bias"), n_out, b["y"], *geo, L.stream())
                logits = b["y"]
            elif fused:
                L.call("bnn_conv2d_fwd_bnsign_pool", cur, xfmt, t["pixel.table"], wq, bias, mean, invstd, gamma, beta,
                       b[f"a{i}"], *geo, L.stream())
                cur, form = b[f"a{i}"], "s8"
            else:
                cur = self._two_pass_layer(i, cur, shp)
                if last:
                    flat = cur.reshape(N, -1)
                    if BF.linear_nsmall_ok(flat, t["fc.weight"]):
                        logits = BF.linear_nsmall(flat, t["fc.weight"], t.get("fc.bias"))
                    else:
                        logits = tF.linear(flat, t["fc.weight"], t.get("fc.bias"))
            if i == 1 and not last:
                hidden = (cur, form, Co)
        return tF.log_softmax(logits, dim=1), hidden

    # ---- CPU restatement
    def _forward_cpu(self, x):
        t = self.t
        if x.dtype == torch.uint8:
            s = t["pixel.table"].to(torch.int64)[x.long()].double()
        else:
            s = _tsign(x).double()
        hidden = None
        for i, (C, Co, KH, KW, pad, H, W, PH, PW) in enumerate(self._shapes(), 1):
            z = tF.conv2d(s, t[f"conv{i}.sign"].double(), None, 1, pad).float()          # exact integer sums
            if f"conv{i}.bias" in t:
                z = z + t[f"conv{i}.bias"].view(1, -1, 1, 1)
            y = _bn_y_cpu(z, *(None if v is None else v.view(1, -1, 1, 1) for v in self._bn(i)))
            p = tF.max_pool2d(tF.hardtanh(y), 2, 2)
            if i == 1:
                hidden = _tsign(p)
            s = _tsign(p).double()
        logits = tF.linear(p.reshape(p.shape[0], -1), t["fc.weight"], t.get("fc.bias"))
        return tF.log_softmax(logits, dim=1), hidden


_CLASSES = {cls.FORMAT: cls for cls in (FrozenMLP, FrozenCNN)}


def from_state(state, device=None):
    """The FrozenMLP or FrozenCNN of a ``state_dict()``; the state's format string tells which."""
    cls = _CLASSES.get(state.get("format"))
    if cls is None:
        raise ValueError(f"from_state: format {state.get('format')!r} is none of {sorted(_CLASSES)}")
    return cls.from_state(state, device)


def freeze(model, normalize=None):
    """Snapshot a trained network for inference (see the module doc): nets.MLP -> FrozenMLP, nets.BinCNN ->
    FrozenCNN.  The weight source of each binarized layer is ``weight.org`` when the layer carries one, else
    ``weight``.  ``normalize`` = (mean, std) is the Normalize the u8 pixels of a BinCNN go through (an MLP
    carries its own in ``fc1.pixel_normalize``).  Raises ValueError for a BatchNorm without running
    statistics or a CNN layer that is not conv -> BatchNorm2d -> Hardtanh(-1, 1) -> MaxPool2d(2, 2)."""
    cls = FrozenCNN if isinstance(model, nets.BinCNN) else FrozenMLP
    if cls is FrozenMLP and normalize is not None:
        raise ValueError("freeze: normalize applies to a BinCNN; an MLP carries fc1.pixel_normalize")
    return cls(*cls._snapshot(model, normalize), model)
