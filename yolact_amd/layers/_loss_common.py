"""What the MultiBoxLoss terms (match.py, mask_loss.py, class_loss.py, segm_loss.py) share around their launches: the tensor
coercions, the per-image offsets, the workspace, the switch check, the GT-mask downsampling and the autograd rule."""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from .. import _lib as L


def f32(t, dev):
    return t.detach().to(device=dev, dtype=torch.float32).contiguous()


def i32(t, dev):
    return t.detach().to(device=dev, dtype=torch.int32).contiguous()


def mask_u8(t, dev):
    """A 0 / nonzero mask of any dtype as uint8 0 / 1 (uint8 is taken as it is: the kernels test != 0)."""
    return t.detach().contiguous() if t.dtype == torch.uint8 else t.detach().to(device=dev).ne(0).to(torch.uint8).contiguous()


def offsets(off, dev):
    """B + 1 Python ints -> (int32 ctypes array for the host-side validation, int32 device tensor); the caller keeps both alive."""
    off = list(off)
    return (C.c_int32 * len(off))(*off), torch.tensor(off, dtype=torch.int32).to(dev)


def workspace(what, d, dev):
    """ymi_workspace_bytes(YMI_WS_<what>, d) bytes on dev with d.ws set; the caller keeps the tensor alive over the launch."""
    nbytes = L.lib().ymi_workspace_bytes(getattr(L, 'WS_' + what), C.byref(d))
    if nbytes < 0:
        L.check(int(nbytes), 'ymi_workspace_bytes(YMI_WS_%s)' % what)
    ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
    d.ws = ws.data_ptr()
    return ws


def check_shipped_switches(cfg, table, who, kernels='the kernels implement %r, what every shipped config trains with'):
    """NotImplementedError naming the cfg field for every switch of `table` (field -> implemented value) that cfg sets otherwise."""
    for field, want in table.items():
        if bool(getattr(cfg, field)) != want:
            raise NotImplementedError('yolact_amd %s: cfg.%s = %r is not supported (%s)'
                                      % (who, field, getattr(cfg, field), kernels % (want,)))


def downsample_gt(masks, mask_h, mask_w):
    """[n,H,W] float GT masks -> uint8 [n,mask_h,mask_w], as the reference prepares them (multibox_loss.py:227-230, 519-526)."""
    with torch.no_grad():
        down = F.interpolate(masks.unsqueeze(0), (mask_h, mask_w), mode='bilinear', align_corners=False).squeeze(0)
        return down.gt(0.5).to(torch.uint8)


class LossFunction(torch.autograd.Function):
    """apply(launch, k, *inputs) -> the 0-dim loss, once differentiable in the first k inputs.  launch(*inputs, *want) with k
    bools `want` returns a tuple (loss [1], the k gradients or None where not wanted, ...) from ONE launch sequence; backward
    multiplies the stored gradients by the upstream scalar and casts them to their inputs' dtypes."""

    @staticmethod
    def forward(ctx, launch, k, *inputs):
        out = launch(*inputs, *ctx.needs_input_grad[2:2 + k])
        ctx.grads, ctx.dtypes, ctx.rest = out[1:1 + k], [t.dtype for t in inputs[:k]], len(inputs) - k
        return out[0].reshape(())

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        grads = tuple(None if d is None else (d * g).to(dt) for d, dt in zip(ctx.grads, ctx.dtypes))
        return (None, None) + grads + (None,) * ctx.rest
