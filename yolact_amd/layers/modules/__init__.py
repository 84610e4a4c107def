from .multibox_loss import MultiBoxLoss  # noqa: F401

__all__ = ['MultiBoxLoss']
