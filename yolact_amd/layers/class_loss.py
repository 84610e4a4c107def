"""The class term 'C' of MultiBoxLoss with online hard example mining on the HIP kernels (layers/modules/multibox_loss.py:242-296
ohem_conf_loss; csrc/class_loss.hip, include/yolact_amd.h ymi_class_loss_desc).

    ohem_conf_loss(conf_data, conf_t, negpos_ratio=None) -> 0-dim tensor
        conf_data [B,P,C] logits, conf_t [B,P] (class + 1, 0 background, -1 neutral; what match_targets returns).  Once
        differentiable in conf_data: one call of ymi_class_loss_f32 computes the loss and its gradient, backward multiplies the
        stored gradient by the upstream scalar.  The selection of the negatives carries no gradient, as in the reference.
    ohem_terms(conf_data, conf_t, negpos_ratio=None) -> dict(C [1], neg [B,P] bool, num_neg [B] long, d_conf [B,P,C])
        one launch sequence with every output; no autograd.
    check_switches(cfg)
        NotImplementedError naming the cfg field for what the kernels do not implement.

conf_alpha and (without the argument) ohem_negpos_ratio are read from active_cfg().  Two definitions are deliberate where the
reference is loose: the mining key subtracts the row's own maximum, and equal keys at the cut go to the lowest
prior index.  CPU tensors raise: there is no CPU path.
"""
from __future__ import annotations

import ctypes as C

import torch

from .. import _lib as L
from ..config import active_cfg
from . import _loss_common as LC

# cfg field -> the value the kernels implement (every shipped config: data/config.py:517,528 and the focal / objectness switches)
SHIPPED_SWITCHES = {
    'use_focal_loss': False,
    'use_sigmoid_focal_loss': False,
    'use_objectness_score': False,
    'ohem_use_most_confident': False,
    'use_class_balanced_conf': False,
}


def check_switches(cfg):
    """NotImplementedError naming the cfg field for every switch outside what the shipped configs train with."""
    LC.check_shipped_switches(cfg, SHIPPED_SWITCHES, 'ohem_conf_loss')


def _launch(conf_data, conf_t, negpos_ratio, conf_alpha, want_grad):
    """ymi_class_loss_f32 on detached tensors -> (loss [1], d_conf or None, neg uint8 [B,P], num_neg int32 [B])."""
    L.require_cuda(conf_data, 'class_loss conf_data')
    L.require_cuda(conf_t, 'class_loss conf_t')
    if conf_data.dim() != 3 or tuple(conf_t.shape) != tuple(conf_data.shape[:2]):
        raise ValueError('class_loss: conf_data %s / conf_t %s' % (tuple(conf_data.shape), tuple(conf_t.shape)))
    dev = conf_data.device
    B, P, NC = conf_data.shape
    with torch.cuda.device(dev), torch.no_grad():
        confd, ctd = LC.f32(conf_data, dev), LC.i32(conf_t, dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        neg = torch.empty(B, P, dtype=torch.uint8, device=dev)
        num_neg = torch.empty(B, dtype=torch.int32, device=dev)
        dconf = torch.empty(B, P, NC, dtype=torch.float32, device=dev) if want_grad else None
        d = L.ClassLossDesc()
        d.conf, d.conf_t, d.loss, d.neg, d.num_neg = confd.data_ptr(), ctd.data_ptr(), loss.data_ptr(), neg.data_ptr(), num_neg.data_ptr()
        d.d_conf = None if dconf is None else dconf.data_ptr()
        d.B, d.P, d.C, d.negpos_ratio, d.conf_alpha = B, P, NC, int(negpos_ratio), float(conf_alpha)
        ws = LC.workspace('CLASS_LOSS', d, dev)
        L.check(L.lib().ymi_class_loss_f32(C.byref(d), L.stream_ptr()), 'ymi_class_loss_f32')
        return loss, dconf, neg, num_neg


def _ratio(cfg, negpos_ratio):
    return int(cfg.ohem_negpos_ratio if negpos_ratio is None else negpos_ratio)


def ohem_conf_loss(conf_data, conf_t, negpos_ratio=None):
    """conf_data [B,P,C], conf_t [B,P] -> cfg.conf_alpha * cross_entropy(sum) over the positives and the mined negatives."""
    cfg = active_cfg()
    check_switches(cfg)
    return LC.LossFunction.apply(_launch, 1, conf_data, conf_t, _ratio(cfg, negpos_ratio), float(cfg.conf_alpha))


def ohem_terms(conf_data, conf_t, negpos_ratio=None):
    """One launch sequence with every output, no autograd: dict(C [1], neg [B,P] bool, num_neg [B] long, d_conf [B,P,C])."""
    cfg = active_cfg()
    check_switches(cfg)
    loss, dconf, neg, num_neg = _launch(conf_data, conf_t, _ratio(cfg, negpos_ratio), float(cfg.conf_alpha), True)
    return dict(C=loss, neg=neg.bool(), num_neg=num_neg.long(), d_conf=dconf)
