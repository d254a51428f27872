"""bnn_amd -- MI355X-native binarized-network training hot path.

Layers: ``functional`` (libbnn.so ops + autograd Functions), ``nn`` (BinarizeLinear /
BinarizeConv2d modules with the reference's ``weight.org`` protocol), ``parallel`` (RCCL
bucketed gradient exchange), ``optim`` (fused latent Adam / SGD + clamp, Bop), ``nets`` / ``trainer``
(the reference's training loop restated), ``data`` (synthetic MNIST + sampler), ``inference``
(``freeze(model) -> FrozenMLP / FrozenCNN``: a trained network packed once and run without the float
model), ``metrics`` (``accuracy`` / ``Meter``: held-out loss, precision@k and confusion counts on the device).
"""
__version__ = "0.1.0"


def __getattr__(name):
    if name == "metrics":
        import importlib
        return importlib.import_module(".metrics", __name__)
    # ``from bnn_amd import freeze, FrozenMLP, FrozenCNN`` (frozen-model inference) without importing torch
    # for users of the package's lighter modules
    if name in ("freeze", "FrozenMLP", "FrozenCNN"):
        from . import inference
        return getattr(inference, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
