"""layers/box_utils.py -> the helpers eval.py's metric code imports (eval.py:5) plus crop / sanitize_coordinates."""
from yolact_amd.layers.box_utils import (center_size, crop, encode, intersect, jaccard, mask_bits, mask_iou,   # noqa: F401
                                         mask_iou_bits, match, point_form, sanitize_coordinates)
