from .multibox_loss import MultiBoxLoss  # noqa: F401
from .multibox_loss_plus import MultiBoxLossPlus  # noqa: F401

__all__ = ['MultiBoxLoss', 'MultiBoxLossPlus']
