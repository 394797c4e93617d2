"""What every layer of the package builds on: the module base class and the buffer holder."""
import torch.nn as nn


try:  # the reference subclasses pl.LightningModule; do the same when Lightning is importable
    import pytorch_lightning as pl  # type: ignore
    _Base = pl.LightningModule
    _HAVE_PL = True
except Exception:  # pragma: no cover - Lightning is not in this image
    _Base = nn.Module
    _HAVE_PL = False


class _Acts:
    """Activation / gradient buffers for one batch size (allocated once, reused every step)."""
    pass
