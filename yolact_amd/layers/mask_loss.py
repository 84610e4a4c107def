"""The lincomb mask loss 'M' of MultiBoxLoss on the HIP kernel (layers/modules/multibox_loss.py:499-627,650).

    mask_loss(proto, coef, box, gt, gt_idx, img_off, weight, crop=True, roi_norm=True, alpha=6.125)
        the batch's instances already gathered (include/yolact_amd.h ymi_mask_loss_desc); a 0-dim loss, differentiable once in
        proto and coef.  One call of ymi_mask_loss_f32 computes the loss and the gradients that are needed; backward multiplies
        them by the upstream scalar.
    lincomb_mask_loss(pos, idx_t, mask_data, proto_data, masks, gt_box_t) -> {'M': loss}
        the reference method's argument subset for the switches the shipped base configs train with, read from active_cfg().
        PyTorch does the plumbing the reference does in PyTorch too: the GT masks are downsampled with F.interpolate and
        binarised under no_grad, the positives are gathered by boolean indexing, and the `masks_to_train` subsample draws
        torch.randperm(n) on the CPU from the global generator, once per image over the cap, in image order — so a seeded run
        selects the reference's subset.

`cfg.use_maskiou` is not read: the mask-IoU targets and maskiou_net_input of YOLACT++ (multibox_loss.py:629-672) are not
produced here.  `cfg.use_mask_scoring` (multibox_loss.py:560,582; False in every shipped config) must be False like the other
unsupported switches.  CPU tensors raise: there is no CPU path.
"""
from __future__ import annotations

import ctypes as C

import torch

from .. import _lib as L
from ..config import act_name, active_cfg
from . import _loss_common as LC

# cfg field -> the value the kernel implements (both shipped base configs: data/config.py coco_base_config / yolact_base_config)
SHIPPED_SWITCHES = {
    'mask_proto_crop_with_pred_box': False,
    'mask_proto_remove_empty_masks': False,
    'mask_proto_reweight_mask_loss': False,
    'mask_proto_normalize_mask_loss_by_sqrt_area': False,
    'mask_proto_double_loss': False,
    'mask_proto_coeff_diversity_loss': False,
    'mask_proto_binarize_downsampled_gt': True,
    'use_mask_scoring': False,
}


def _launch(proto, coef, box, gt, gt_idx, img_off, weight, crop, roi_norm, alpha, want_proto, want_coef, want_inst=False):
    """ymi_mask_loss_f32 on detached fp32 tensors -> (loss [1], d_proto or None, d_coef or None, loss_inst or None)."""
    for name, t in (('proto', proto), ('coef', coef), ('box', box), ('gt', gt), ('gt_idx', gt_idx), ('img_off', img_off),
                    ('weight', weight)):
        L.require_cuda(t, 'mask_loss ' + name)
    if proto.dim() != 4 or coef.dim() != 2 or coef.shape[1] != proto.shape[3]:
        raise ValueError('mask_loss: proto %s / coef %s' % (tuple(proto.shape), tuple(coef.shape)))
    B, mh, mw, K = proto.shape
    N = coef.shape[0]
    if tuple(box.shape) != (N, 4) or gt.dim() != 3 or tuple(gt.shape[1:]) != (mh, mw) or gt_idx.numel() != N \
            or img_off.numel() != B + 1 or weight.numel() != N:
        raise ValueError('mask_loss: box %s / gt %s / gt_idx %s / img_off %s / weight %s do not fit proto %s, coef %s'
                         % (tuple(box.shape), tuple(gt.shape), tuple(gt_idx.shape), tuple(img_off.shape), tuple(weight.shape),
                            tuple(proto.shape), tuple(coef.shape)))
    dev = proto.device
    with torch.cuda.device(dev), torch.no_grad():
        protod, coefd, boxd, weightd = LC.f32(proto, dev), LC.f32(coef, dev), LC.f32(box, dev), LC.f32(weight, dev)
        gtd, gidx, ioff = LC.mask_u8(gt, dev), LC.i32(gt_idx, dev), LC.i32(img_off, dev)
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        loss = new(1)
        linst = new(N) if want_inst else None
        dproto = new(B, mh, mw, K) if want_proto else None
        dcoef = new(N, K) if want_coef else None
        d = L.MaskLossDesc()
        d.proto, d.coef, d.box, d.gt = protod.data_ptr(), coefd.data_ptr(), boxd.data_ptr(), gtd.data_ptr()
        d.gt_idx, d.img_off, d.weight = gidx.data_ptr(), ioff.data_ptr(), weightd.data_ptr()
        d.loss = loss.data_ptr()
        for name, t in (('loss_inst', linst), ('d_proto', dproto), ('d_coef', dcoef)):
            setattr(d, name, None if t is None else t.data_ptr())
        d.B, d.mh, d.mw, d.K, d.N, d.G = B, mh, mw, K, N, gt.shape[0]
        d.crop, d.roi_norm, d.alpha = int(bool(crop)), int(bool(roi_norm)), float(alpha)
        ws = LC.workspace('MASK_LOSS', d, dev)
        L.check(L.lib().ymi_mask_loss_f32(C.byref(d), L.stream_ptr()), 'ymi_mask_loss_f32')
        return loss, dproto, dcoef, linst


def mask_loss(proto, coef, box, gt, gt_idx, img_off, weight, crop=True, roi_norm=True, alpha=6.125):
    """proto [B,mh,mw,32], coef [N,32], box [N,4] (relative point form), gt [G,mh,mw] 0 / 1, gt_idx [N], img_off [B+1],
    weight [N] -> the 0-dim loss alpha / mh / mw * sum_j weight_j L_j.  A gradient is computed only for the tensor (proto, coef)
    that requires it."""
    return LC.LossFunction.apply(_launch, 2, proto, coef, box, gt, gt_idx, img_off, weight, crop, roi_norm, alpha)


def mask_loss_terms(proto, coef, box, gt, gt_idx, img_off, weight, crop=True, roi_norm=True, alpha=6.125):
    """One launch with every output: (loss [1], loss_inst [N], d_proto [B,mh,mw,32], d_coef [N,32]); no autograd."""
    loss, dproto, dcoef, linst = _launch(proto, coef, box, gt, gt_idx, img_off, weight, crop, roi_norm, alpha, True, True, True)
    return loss, linst, dproto, dcoef


def check_switches(cfg):
    """NotImplementedError naming the cfg field for every switch outside what the shipped base configs train with."""
    LC.check_shipped_switches(cfg, SHIPPED_SWITCHES, 'lincomb_mask_loss',
                              'the kernel implements %r, what yolact_base_config and yolact_plus_base_config train with')
    if act_name(cfg.mask_proto_mask_activation) != 'sigmoid':
        raise NotImplementedError('yolact_amd lincomb_mask_loss: cfg.mask_proto_mask_activation must be the sigmoid')


def gather_instances(pos, idx_t, mask_data, masks, gt_box_t, mask_h, mask_w, masks_to_train):
    """The reference's per-image gathering (multibox_loss.py:516-587) for a whole batch, on whatever device the tensors live:
    -> coef [N,32] (differentiable in mask_data), box [N,4], gt uint8 [G,mh,mw], gt_idx int32 [N], img_off int32 [B+1],
    weight fp32 [N], and the list of the drawn `select` index tensors (None for images at or under the cap)."""
    dev = mask_data.device
    coefs, boxes, gts, gidx, weights, offs, selects = [], [], [], [], [], [0], []
    row0 = 0
    for idx in range(mask_data.size(0)):
        gts.append(LC.downsample_gt(masks[idx], mask_h, mask_w))
        cur_pos = pos[idx]
        pos_idx_t = idx_t[idx, cur_pos]
        pos_gt_box_t = gt_box_t[idx, cur_pos]
        proto_coef = mask_data[idx, cur_pos, :]
        old_num_pos = proto_coef.size(0)
        select = None
        if old_num_pos > masks_to_train:
            perm = torch.randperm(proto_coef.size(0))
            select = perm[:masks_to_train]
            sel = select.to(dev)
            proto_coef, pos_idx_t, pos_gt_box_t = proto_coef[sel, :], pos_idx_t[sel], pos_gt_box_t[sel, :]
        selects.append(select)
        num_pos = proto_coef.size(0)
        if num_pos > 0:
            coefs.append(proto_coef)
            boxes.append(pos_gt_box_t)
            gidx.append(pos_idx_t.to(torch.int32) + row0)
            weights.append(torch.full((num_pos,), old_num_pos / num_pos, dtype=torch.float32, device=dev))
        offs.append(offs[-1] + num_pos)
        row0 += gts[-1].size(0)
    K = mask_data.size(2)
    cat = lambda ts, empty: torch.cat(ts) if ts else empty
    coef = cat(coefs, mask_data.new_zeros(0, K))
    box = cat(boxes, gt_box_t.new_zeros(0, 4))
    gt = cat(gts, torch.zeros(0, mask_h, mask_w, dtype=torch.uint8, device=dev))
    gt_idx = cat(gidx, torch.zeros(0, dtype=torch.int32, device=dev))
    weight = cat(weights, torch.zeros(0, dtype=torch.float32, device=dev))
    img_off = torch.tensor(offs, dtype=torch.int32, device=dev)
    return coef, box, gt, gt_idx, img_off, weight, selects


def lincomb_mask_loss(pos, idx_t, mask_data, proto_data, masks, gt_box_t):
    """MultiBoxLoss.lincomb_mask_loss (multibox_loss.py:499-627,650) -> {'M': 0-dim tensor}: pos [B,P] bool, idx_t [B,P] long,
    mask_data [B,P,32], proto_data [B,mh,mw,32], masks = one [n_gt,H,W] float tensor per image, gt_box_t [B,P,4]."""
    cfg = active_cfg()
    check_switches(cfg)
    L.require_cuda(proto_data, 'lincomb_mask_loss proto_data')
    L.require_cuda(mask_data, 'lincomb_mask_loss mask_data')
    mask_h, mask_w = proto_data.size(1), proto_data.size(2)
    coef, box, gt, gt_idx, img_off, weight, _ = gather_instances(pos, idx_t, mask_data, masks, gt_box_t, mask_h, mask_w,
                                                                 int(cfg.masks_to_train))
    if gt.size(0) == 0:
        gt = torch.zeros(1, mask_h, mask_w, dtype=torch.uint8, device=proto_data.device)
    loss = mask_loss(proto_data, coef, box, gt, gt_idx, img_off, weight, crop=bool(cfg.mask_proto_crop),
                     roi_norm=bool(cfg.mask_proto_normalize_emulate_roi_pooling), alpha=float(cfg.mask_alpha))
    return {'M': loss}
