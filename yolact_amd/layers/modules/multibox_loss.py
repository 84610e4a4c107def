"""MultiBoxLoss for the configs that train with B + M + C + S (layers/modules/multibox_loss.py:50-213): every term on the HIP
kernels, composed from match_targets (with the constructor's thresholds), box_loss, lincomb_mask_loss, ohem_conf_loss and
semantic_segmentation_loss.

    crit = MultiBoxLoss(num_classes, pos_threshold, neg_threshold, negpos_ratio)
    losses = crit(net, predictions, targets, masks, num_crowds)          # {'B', 'M', 'C', 'S'}, 0-dim tensors

predictions: dict(loc [B,P,4], conf [B,P,C], mask [B,P,32], priors [P,4], proto [B,mh,mw,32], segm [B,C-1,sh,sw]); targets, masks
and num_crowds as the reference takes them (the crowd annotations last; the caller's lists are not changed).  'B', 'M' and 'C'
are divided by the batch's number of positives as a float (a batch without positives gives the reference's inf / NaN), 'S' by
the batch size (:196-203).  The losses are differentiable through autograd to loc, conf, mask, proto and segm; `net` is not used
(it serves the mask-IoU term of YOLACT++ only).  What the kernels do not implement raises NotImplementedError naming the cfg
field: use_maskiou ('I'), mask_proto_loss ('P'), use_class_existence_loss, train_masks = False, a mask_type other than lincomb,
use_instance_coeff, and every switch the terms' own check_switches refuse.
"""
from __future__ import annotations

from torch import nn

from .. import class_loss as CL
from .. import mask_loss as ML
from .. import match as MT
from .. import segm_loss as SL
from ... import _lib as L
from ...config import active_cfg, is_lincomb


def check_switches(cfg, allow_maskiou=False):
    """NotImplementedError naming the cfg field for every loss term or switch that does not exist here (allow_maskiou: the caller,
    multibox_loss_plus.MultiBoxLossPlus, computes the term 'I')."""
    def refuse(field, why):
        raise NotImplementedError('yolact_amd MultiBoxLoss: cfg.%s = %r is not supported (%s)' % (field, getattr(cfg, field), why))
    if cfg.use_maskiou and not allow_maskiou:
        refuse('use_maskiou', "the mask-IoU term 'I' of the YOLACT++ configs is not implemented")
    if cfg.mask_proto_loss is not None:
        refuse('mask_proto_loss', "the prototype term 'P' is not implemented")
    if cfg.use_class_existence_loss:
        refuse('use_class_existence_loss', "the class existence term 'E' is not implemented")
    if not cfg.train_masks:
        refuse('train_masks', "the mask term 'M' is always trained")
    if not is_lincomb(cfg):
        refuse('mask_type', 'only the lincomb mask loss is implemented')
    if cfg.use_instance_coeff:
        refuse('use_instance_coeff', 'instance coefficients are not implemented')
    MT.check_switches(cfg)
    ML.check_switches(cfg)
    CL.check_switches(cfg)


class MultiBoxLoss(nn.Module):
    def __init__(self, num_classes, pos_threshold, neg_threshold, negpos_ratio):
        super().__init__()
        self.num_classes = num_classes
        self.pos_threshold = pos_threshold
        self.neg_threshold = neg_threshold
        self.negpos_ratio = negpos_ratio

    def forward(self, net, predictions, targets, masks, num_crowds):
        cfg = active_cfg()
        check_switches(cfg)
        return self._losses(cfg, net, predictions, targets, masks, num_crowds, maskiou=False)

    def _losses(self, cfg, net, predictions, targets, masks, num_crowds, maskiou):
        """The terms of forward(); maskiou: also 'I' (multibox_loss_plus.MultiBoxLossPlus)."""
        loc_data, conf_data, mask_data = predictions['loc'], predictions['conf'], predictions['mask']
        priors, proto_data = predictions['priors'], predictions['proto']
        for name in ('loc', 'conf', 'mask', 'priors', 'proto'):
            L.require_cuda(predictions[name], 'MultiBoxLoss predictions[%r]' % name)
        batch_size = loc_data.size(0)
        if not (len(targets) == len(masks) == len(num_crowds) == batch_size):
            raise ValueError('MultiBoxLoss: %d targets, %d masks, %d num_crowds for a batch of %d'
                             % (len(targets), len(masks), len(num_crowds), batch_size))
        if conf_data.size(2) != self.num_classes:
            raise ValueError('MultiBoxLoss: conf has %d classes, the criterion %d' % (conf_data.size(2), self.num_classes))

        # split the crowd annotations off the labels and masks (:109-117) into new lists; match_targets splits the boxes itself
        labels, obj_masks = [], []
        for tgt, msk, nc in zip(targets, masks, num_crowds):
            L.require_cuda(tgt, 'MultiBoxLoss targets')
            L.require_cuda(msk, 'MultiBoxLoss masks')
            n = tgt.size(0) - int(nc)
            labels.append(tgt[:n, 4].detach().long())
            obj_masks.append(msk[:n])

        m = MT.match_targets(priors, [t.detach() for t in targets], [int(nc) for nc in num_crowds],
                             pos_threshold=self.pos_threshold, neg_threshold=self.neg_threshold)
        conf_t, idx_t, pos = m['conf_t'], m['idx_t'], m['pos']

        losses = MT.box_loss(loc_data, m['loc_t'], pos)
        maskiou_targets = None
        if maskiou:
            from .. import maskiou_loss as MIL
            ret, maskiou_targets = MIL.lincomb_mask_loss_maskiou(pos, idx_t, mask_data, proto_data, obj_masks, m['gt_box_t'], labels)
            losses.update(ret)
        else:
            losses.update(ML.lincomb_mask_loss(pos, idx_t, mask_data, proto_data, obj_masks, m['gt_box_t']))
        losses['C'] = CL.ohem_conf_loss(conf_data, conf_t, self.negpos_ratio)
        if cfg.use_semantic_segmentation_loss:
            losses['S'] = SL.semantic_segmentation_loss(predictions['segm'], obj_masks, labels)
        if maskiou_targets is not None:                                      # :186-188
            losses['I'] = MIL.mask_iou_loss(net, maskiou_targets)

        # :196-203
        total_num_pos = m['num_pos'].sum().float()
        for k in losses:
            losses[k] = losses[k] / (batch_size if k == 'S' else total_num_pos)
        return losses
