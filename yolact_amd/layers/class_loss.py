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
from torch.autograd.function import once_differentiable

from .. import _lib as L
from ..config import active_cfg

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
    for field, want in SHIPPED_SWITCHES.items():
        if bool(getattr(cfg, field)) != want:
            raise NotImplementedError('yolact_amd ohem_conf_loss: cfg.%s = %r is not supported (the kernels implement %r, what '
                                      'every shipped config trains with)' % (field, getattr(cfg, field), want))


def _launch(conf_data, conf_t, negpos_ratio, conf_alpha, want_grad):
    """ymi_class_loss_f32 on detached tensors -> (loss [1], neg uint8 [B,P], num_neg int32 [B], d_conf or None)."""
    L.require_cuda(conf_data, 'class_loss conf_data')
    L.require_cuda(conf_t, 'class_loss conf_t')
    if conf_data.dim() != 3 or tuple(conf_t.shape) != tuple(conf_data.shape[:2]):
        raise ValueError('class_loss: conf_data %s / conf_t %s' % (tuple(conf_data.shape), tuple(conf_t.shape)))
    dev = conf_data.device
    B, P, NC = conf_data.shape
    with torch.cuda.device(dev), torch.no_grad():
        confd = conf_data.detach().to(dtype=torch.float32).contiguous()
        ctd = conf_t.detach().to(device=dev, dtype=torch.int32).contiguous()
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        neg = torch.empty(B, P, dtype=torch.uint8, device=dev)
        num_neg = torch.empty(B, dtype=torch.int32, device=dev)
        dconf = torch.empty(B, P, NC, dtype=torch.float32, device=dev) if want_grad else None
        d = L.ClassLossDesc()
        d.conf, d.conf_t, d.loss, d.neg, d.num_neg = confd.data_ptr(), ctd.data_ptr(), loss.data_ptr(), neg.data_ptr(), num_neg.data_ptr()
        d.d_conf = None if dconf is None else dconf.data_ptr()
        d.B, d.P, d.C, d.negpos_ratio, d.conf_alpha = B, P, NC, int(negpos_ratio), float(conf_alpha)
        nbytes = L.lib().ymi_workspace_bytes(L.WS_CLASS_LOSS, C.byref(d))
        if nbytes < 0:
            L.check(int(nbytes), 'ymi_workspace_bytes(YMI_WS_CLASS_LOSS)')
        ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
        d.ws = ws.data_ptr()
        L.check(L.lib().ymi_class_loss_f32(C.byref(d), L.stream_ptr()), 'ymi_class_loss_f32')
        return loss, neg, num_neg, dconf


class _ClassLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, conf_data, conf_t, negpos_ratio, conf_alpha):
        loss, _, _, dconf = _launch(conf_data, conf_t, negpos_ratio, conf_alpha, ctx.needs_input_grad[0])
        ctx.grad = dconf
        ctx.dtype = conf_data.dtype
        return loss.reshape(())

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        return (None if ctx.grad is None else (ctx.grad * g).to(ctx.dtype)), None, None, None


def _ratio(cfg, negpos_ratio):
    return int(cfg.ohem_negpos_ratio if negpos_ratio is None else negpos_ratio)


def ohem_conf_loss(conf_data, conf_t, negpos_ratio=None):
    """conf_data [B,P,C], conf_t [B,P] -> cfg.conf_alpha * cross_entropy(sum) over the positives and the mined negatives."""
    cfg = active_cfg()
    check_switches(cfg)
    return _ClassLossFunction.apply(conf_data, conf_t, _ratio(cfg, negpos_ratio), float(cfg.conf_alpha))


def ohem_terms(conf_data, conf_t, negpos_ratio=None):
    """One launch sequence with every output, no autograd: dict(C [1], neg [B,P] bool, num_neg [B] long, d_conf [B,P,C])."""
    cfg = active_cfg()
    check_switches(cfg)
    loss, neg, num_neg, dconf = _launch(conf_data, conf_t, _ratio(cfg, negpos_ratio), float(cfg.conf_alpha), True)
    return dict(C=loss, neg=neg.bool(), num_neg=num_neg.long(), d_conf=dconf)
