"""The semantic segmentation term 'S' of MultiBoxLoss on the HIP kernel (layers/modules/multibox_loss.py:218-239;
csrc/segm_loss.hip, include/yolact_amd.h ymi_segm_loss_desc).

    segm_loss(segm, gt, label, gt_off, alpha=1.0) -> 0-dim tensor
        prepared inputs: segm [B,K,mh,mw] logits, gt [G,mh,mw] 0 / 1 (the downsampled, binarised GT masks of the batch, image by
        image), label [G], gt_off = the B + 1 offsets of the images into gt (a Python list).  Once differentiable in segm: one
        call of ymi_segm_loss_f32 computes the loss and its gradient, backward multiplies by the upstream scalar.
    segm_terms(segm, gt, label, gt_off, alpha=1.0) -> (loss [1], d_segm [B,K,mh,mw]); no autograd.
    semantic_segmentation_loss(segment_data, mask_t, class_t) -> 0-dim tensor
        the reference method's arguments: mask_t = one [n,H,W] float tensor per image, class_t = one [n] label tensor per image.
        PyTorch does the plumbing the reference does in PyTorch too: the masks are downsampled with F.interpolate (bilinear,
        align_corners=False) and binarised with .gt(0.5) under no_grad, exactly as mask_loss.gather_instances does for 'M'.

semantic_segmentation_alpha is read from active_cfg().  CPU tensors raise: there is no CPU path.
"""
from __future__ import annotations

import ctypes as C

import torch

from .. import _lib as L
from ..config import active_cfg
from . import _loss_common as LC


def _launch(segm, gt, label, gt_off, alpha, want_grad):
    """ymi_segm_loss_f32 on detached tensors -> (loss [1], d_segm or None)."""
    for name, t in (('segm', segm), ('gt', gt), ('label', label)):
        L.require_cuda(t, 'segm_loss ' + name)
    gt_off = [int(v) for v in gt_off]
    if segm.dim() != 4 or gt.dim() != 3 or tuple(gt.shape[1:]) != tuple(segm.shape[2:]) or label.numel() != gt.size(0) \
            or len(gt_off) != segm.size(0) + 1:
        raise ValueError('segm_loss: segm %s / gt %s / label %s / %d offsets' % (tuple(segm.shape), tuple(gt.shape),
                                                                                   tuple(label.shape), len(gt_off)))
    dev = segm.device
    B, K, mh, mw = segm.shape
    G = gt.size(0)
    with torch.cuda.device(dev), torch.no_grad():
        segmd, gtd, labeld = LC.f32(segm, dev), LC.mask_u8(gt, dev), LC.i32(label, dev)
        off_h, off_d = LC.offsets(gt_off, dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        dsegm = torch.empty(B, K, mh, mw, dtype=torch.float32, device=dev) if want_grad else None
        d = L.SegmLossDesc()
        d.segm, d.gt_off, d.gt_off_host, d.loss = segmd.data_ptr(), off_d.data_ptr(), C.cast(off_h, C.c_void_p), loss.data_ptr()
        if G:
            d.gt, d.label = gtd.data_ptr(), labeld.data_ptr()
        d.d_segm = None if dsegm is None else dsegm.data_ptr()
        d.B, d.K, d.mh, d.mw, d.G, d.alpha = B, K, mh, mw, G, float(alpha)
        ws = LC.workspace('SEGM_LOSS', d, dev)
        L.check(L.lib().ymi_segm_loss_f32(C.byref(d), L.stream_ptr()), 'ymi_segm_loss_f32')
        return loss, dsegm


def segm_loss(segm, gt, label, gt_off, alpha=1.0):
    """segm [B,K,mh,mw], gt [G,mh,mw] 0 / 1, label [G], gt_off B + 1 offsets -> alpha / (mh mw) * the summed BCE with logits."""
    return LC.LossFunction.apply(_launch, 1, segm, gt, label, gt_off, float(alpha))


def segm_terms(segm, gt, label, gt_off, alpha=1.0):
    """One launch sequence with every output, no autograd: (loss [1], d_segm [B,K,mh,mw])."""
    return _launch(segm, gt, label, gt_off, float(alpha), True)


def downsample_targets(mask_t, class_t, mask_h, mask_w, device):
    """The reference's GT preparation (multibox_loss.py:227-230) for a whole batch -> gt uint8 [G,mh,mw], label long [G], offsets."""
    gts, labels, off = [], [], [0]
    with torch.no_grad():
        for m, c in zip(mask_t, class_t):
            if m.size(0):
                gts.append(LC.downsample_gt(m, mask_h, mask_w))
                labels.append(c.long())
            off.append(off[-1] + m.size(0))
    gt = torch.cat(gts) if gts else torch.zeros(0, mask_h, mask_w, dtype=torch.uint8, device=device)
    label = torch.cat(labels) if labels else torch.zeros(0, dtype=torch.long, device=device)
    return gt, label, off


def semantic_segmentation_loss(segment_data, mask_t, class_t):
    """MultiBoxLoss.semantic_segmentation_loss (multibox_loss.py:218-239) -> 0-dim tensor."""
    cfg = active_cfg()
    L.require_cuda(segment_data, 'semantic_segmentation_loss segment_data')
    if len(mask_t) != segment_data.size(0) or len(class_t) != segment_data.size(0):
        raise ValueError('semantic_segmentation_loss: %d masks, %d labels for a batch of %d' % (len(mask_t), len(class_t), segment_data.size(0)))
    for m, c in zip(mask_t, class_t):
        L.require_cuda(m, 'semantic_segmentation_loss mask_t')
        if m.size(0) != c.numel():
            raise ValueError('semantic_segmentation_loss: %d masks, %d labels in one image' % (m.size(0), c.numel()))
    gt, label, off = downsample_targets(mask_t, class_t, segment_data.size(2), segment_data.size(3), segment_data.device)
    return segm_loss(segment_data, gt, label.to(segment_data.device), off, float(cfg.semantic_segmentation_alpha))
