"""utils/augmentations.py -> the device transforms (train.py's SSDAugmentation, eval.py's BaseTransform / FastBaseTransform).

This directory deliberately has no __init__.py: with the reference checkout on sys.path as well (the eval.py drop-in), the
reference's own `utils` package — a regular package, which eval.py also needs for utils.functions and utils.timer — keeps precedence
over this namespace portion; with shim/ alone, `from utils.augmentations import SSDAugmentation` resolves here."""
from yolact_amd.utils.augmentations import (MEANS, STD, AugmentParams, BaseTransform, FastBaseTransform,   # noqa: F401
                                            SSDAugmentation, draw_augmentation)
