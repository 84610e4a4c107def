"""Drop-in for the reference's `layers.modules` (train.py: `from layers.modules import MultiBoxLoss`)."""
from yolact_amd.layers.modules import MultiBoxLoss                      # noqa: F401

__all__ = ['MultiBoxLoss']
