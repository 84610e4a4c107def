"""MultiBoxLoss for the YOLACT++ configs: B + M + C + S of multibox_loss.MultiBoxLoss, computed by the same calls, plus the mask-IoU
term 'I' (layers/modules/multibox_loss.py:180-188; layers/maskiou_loss.py).

    crit = MultiBoxLossPlus(num_classes, pos_threshold, neg_threshold, negpos_ratio)
    losses = crit(net, predictions, targets, masks, num_crowds)          # {'B', 'M', 'C', 'S', 'I'}, 0-dim tensors

`net` is anything with a .maskiou_net FastMaskIoUNet.  'I' is divided by the batch's number of positives like 'B', 'M' and 'C'
(:196-203) and is absent when cfg.discard_mask_area leaves no instance (:187, :657-658) or cfg.use_maskiou is off.  The losses are
differentiable to loc, conf, mask, proto, segm and net.maskiou_net's parameters.  The switches MultiBoxLoss refuses are refused
here too, except use_maskiou; cfg.maskious_to_train > 0 raises NotImplementedError naming the field.
"""
from __future__ import annotations

from .. import maskiou_loss as MIL
from ...config import active_cfg
from .multibox_loss import MultiBoxLoss, check_switches


class MultiBoxLossPlus(MultiBoxLoss):
    def forward(self, net, predictions, targets, masks, num_crowds):
        cfg = active_cfg()
        check_switches(cfg, allow_maskiou=True)
        if cfg.use_maskiou:
            MIL.check_switches(cfg)
        return self._losses(cfg, net, predictions, targets, masks, num_crowds, maskiou=bool(cfg.use_maskiou))
