"""MultiBoxLoss target assignment and the box loss 'B' on the HIP kernels (layers/box_utils.py:159-265 match / encode,
layers/modules/multibox_loss.py:84-145; csrc/match.hip).

    match_targets(priors, targets, num_crowds, loc_data=None, pos_threshold=None, neg_threshold=None)
        -> dict(loc_t [B,P,4], conf_t [B,P] long, idx_t [B,P] long, gt_box_t [B,P,4], pos [B,P] bool, num_pos [B] long)
        the loop of multibox_loss.py:100-126 for the whole batch in one call of ymi_match_f32: `targets` is the reference's list of
        [n,5] tensors (x1, y1, x2, y2, label) with the crowd annotations last, `num_crowds` its list of crowd counts.  With
        loc_data [B,P,4] the same call also returns 'B' (bbox_alpha * the summed smooth-L1 at the positives, un-normalised, as
        losses['B'] is before multibox_loss.py:196-203) and 'd_loc', its gradient in loc_data.  pos, idx_t and gt_box_t are what
        lincomb_mask_loss takes.
    box_loss(loc_data, loc_t, pos) -> {'B': 0-dim}
        multibox_loss.py:141-145 for given targets, once differentiable in loc_data.
    check_switches(cfg)
        NotImplementedError naming the cfg field for what the kernels do not implement.

Thresholds and bbox_alpha are read from active_cfg().  CPU tensors raise: there is no CPU path.
"""
from __future__ import annotations

import ctypes as C

import torch

from .. import _lib as L
from ..config import active_cfg
from . import _loss_common as LC

# cfg field -> the value the kernels implement (every shipped config: data/config.py:443,553,600,620,698-701)
SHIPPED_SWITCHES = {
    'use_prediction_matching': False,
    'use_change_matching': False,
    'use_yolo_regressors': False,
    'train_boxes': True,
}


def check_switches(cfg):
    """NotImplementedError naming the cfg field for every switch outside what the shipped configs train with."""
    LC.check_shipped_switches(cfg, SHIPPED_SWITCHES, 'match_targets / box_loss')


def _launch(priors, truth, label, gt_off, crowd, crowd_off, loc_data, pos_thresh, neg_thresh, crowd_thresh, bbox_alpha,
            want_grad=True):
    """ymi_match_f32 on fp32 device tensors; gt_off / crowd_off are Python lists of B + 1 offsets (crowd None without crowds).
    -> dict of the kernel's outputs in its own dtypes (conf_t / idx_t / num_pos int32, pos uint8)."""
    for name, t in (('priors', priors), ('truth', truth), ('label', label)):
        L.require_cuda(t, 'match ' + name)
    if loc_data is not None:
        L.require_cuda(loc_data, 'match loc_data')
    if priors.dim() != 2 or priors.size(1) != 4 or truth.dim() != 2 or truth.size(1) != 4 or label.numel() != truth.size(0):
        raise ValueError('match: priors %s / truth %s / label %s' % (tuple(priors.shape), tuple(truth.shape), tuple(label.shape)))
    dev = priors.device
    B, P, G = len(gt_off) - 1, priors.size(0), truth.size(0)
    Gc = 0 if crowd is None else crowd.size(0)
    if loc_data is not None and tuple(loc_data.shape) != (B, P, 4):
        raise ValueError('match: loc_data %s is not [%d, %d, 4]' % (tuple(loc_data.shape), B, P))
    with torch.cuda.device(dev), torch.no_grad():
        priorsd, truthd, labeld = LC.f32(priors, dev), LC.f32(truth, dev), LC.i32(label, dev)
        off_h, off_d = LC.offsets(gt_off, dev)
        new = lambda dtype, *shape: torch.empty(*shape, dtype=dtype, device=dev)
        out = dict(loc_t=new(torch.float32, B, P, 4), gt_box_t=new(torch.float32, B, P, 4), conf_t=new(torch.int32, B, P),
                   idx_t=new(torch.int32, B, P), pos=new(torch.uint8, B, P), num_pos=new(torch.int32, B))
        d = L.MatchDesc()
        d.priors, d.truth, d.label, d.gt_off = priorsd.data_ptr(), truthd.data_ptr(), labeld.data_ptr(), off_d.data_ptr()
        d.gt_off_host = C.cast(off_h, C.c_void_p)
        if Gc:
            crowdd = LC.f32(crowd, dev)
            coff_h, coff_d = LC.offsets(crowd_off, dev)
            d.crowd, d.crowd_off, d.crowd_off_host = crowdd.data_ptr(), coff_d.data_ptr(), C.cast(coff_h, C.c_void_p)
        if loc_data is not None:
            locd = LC.f32(loc_data, dev)
            out['loss'] = new(torch.float32, 1)
            d.loc_data, d.loss = locd.data_ptr(), out['loss'].data_ptr()
            if want_grad:
                out['d_loc'] = new(torch.float32, B, P, 4)
                d.d_loc = out['d_loc'].data_ptr()
        for name in ('loc_t', 'gt_box_t', 'conf_t', 'idx_t', 'pos', 'num_pos'):
            setattr(d, name, out[name].data_ptr())
        d.B, d.P, d.G, d.Gc = B, P, G, Gc
        d.pos_thresh, d.neg_thresh, d.crowd_thresh, d.bbox_alpha = pos_thresh, neg_thresh, crowd_thresh, bbox_alpha
        ws = LC.workspace('MATCH', d, dev)
        L.check(L.lib().ymi_match_f32(C.byref(d), L.stream_ptr()), 'ymi_match_f32')
        return out


def match_targets(priors, targets, num_crowds, loc_data=None, pos_threshold=None, neg_threshold=None):
    """See the module docstring.  One launch sequence for the batch; nothing is read back to the host.  pos_threshold /
    neg_threshold override cfg.positive_iou_threshold / cfg.negative_iou_threshold (MultiBoxLoss passes its constructor's)."""
    cfg = active_cfg()
    check_switches(cfg)
    L.require_cuda(priors, 'match_targets priors')
    if len(targets) != len(num_crowds) or not len(targets):
        raise ValueError('match_targets: %d targets, %d num_crowds' % (len(targets), len(num_crowds)))
    truths, labels, crowds, gt_off, crowd_off = [], [], [], [0], [0]
    for tgt, nc in zip(targets, num_crowds):
        L.require_cuda(tgt, 'match_targets targets')
        nc = int(nc)
        n = tgt.size(0) - nc                            # the crowd annotations are the last nc rows (multibox_loss.py:110-117)
        truths.append(tgt[:n, :4])
        labels.append(tgt[:n, 4])
        if nc > 0:
            crowds.append(tgt[n:, :4])
        gt_off.append(gt_off[-1] + n)
        crowd_off.append(crowd_off[-1] + nc)
    out = _launch(priors, torch.cat(truths), torch.cat(labels).long(), gt_off, torch.cat(crowds) if crowds else None, crowd_off,
                  loc_data, float(cfg.positive_iou_threshold if pos_threshold is None else pos_threshold),
                  float(cfg.negative_iou_threshold if neg_threshold is None else neg_threshold),
                  float(cfg.crowd_iou_threshold), float(cfg.bbox_alpha))
    res = dict(loc_t=out['loc_t'], conf_t=out['conf_t'].long(), idx_t=out['idx_t'].long(), gt_box_t=out['gt_box_t'],
               pos=out['pos'].bool(), num_pos=out['num_pos'].long())
    if loc_data is not None:
        res['B'] = out['loss'].reshape(())
        res['d_loc'] = out['d_loc']
    return res


def _box_loss_launch(loc_data, loc_t, pos, bbox_alpha, want_grad):
    for name, t in (('loc_data', loc_data), ('loc_t', loc_t), ('pos', pos)):
        L.require_cuda(t, 'box_loss ' + name)
    if loc_data.dim() != 3 or loc_data.size(2) != 4 or loc_t.shape != loc_data.shape or tuple(pos.shape) != tuple(loc_data.shape[:2]):
        raise ValueError('box_loss: loc_data %s / loc_t %s / pos %s' % (tuple(loc_data.shape), tuple(loc_t.shape), tuple(pos.shape)))
    dev = loc_data.device
    B, P = loc_data.shape[:2]
    with torch.cuda.device(dev), torch.no_grad():
        locd, loctd, posd = LC.f32(loc_data, dev), LC.f32(loc_t, dev), LC.mask_u8(pos, dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        dloc = torch.empty(B, P, 4, dtype=torch.float32, device=dev) if want_grad else None
        d = L.MatchDesc()
        d.B, d.P = B, P
        ws = LC.workspace('BOX_LOSS', d, dev)
        L.check(L.lib().ymi_box_loss_f32(locd.data_ptr(), loctd.data_ptr(), posd.data_ptr(), B, P, float(bbox_alpha),
                                         loss.data_ptr(), None if dloc is None else dloc.data_ptr(), ws.data_ptr(),
                                         L.stream_ptr()), 'ymi_box_loss_f32')
        return loss, dloc


def box_loss(loc_data, loc_t, pos):
    """loc_data, loc_t [B,P,4], pos [B,P] bool -> {'B': cfg.bbox_alpha * smooth_l1(loc_data[pos], loc_t[pos], sum)}."""
    cfg = active_cfg()
    check_switches(cfg)
    return {'B': LC.LossFunction.apply(_box_loss_launch, 1, loc_data, loc_t, pos, float(cfg.bbox_alpha))}
