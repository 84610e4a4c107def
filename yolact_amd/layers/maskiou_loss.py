"""The mask-IoU term 'I' of YOLACT++ on the HIP kernels of csrc/maskiou_loss.hip (layers/modules/multibox_loss.py:629-672, 684-694).

    lincomb_mask_loss_maskiou(pos, idx_t, mask_data, proto_data, masks, gt_box_t, labels) -> ({'M': loss}, maskiou_targets or None)
        the reference method under cfg.use_maskiou.  'M' is mask_loss.lincomb_mask_loss's term on the same gathered instances (one
        gather, one set of torch.randperm draws: the subset 'M' trains on is the subset the targets are made from).
        maskiou_targets = [maskiou_net_input [n,1,mh,mw], maskiou_t [n], label_t [n]]: the instances whose downsampled GT area
        exceeds cfg.discard_mask_area (boolean indexing, :630-640); None when none survives (:657-658).  maskiou_net_input is
        differentiable once in proto_data and mask_data (ymi_maskiou_input_f32 / _bwd_f32).
    mask_iou_loss(net, maskiou_targets) -> the 0-dim 'I' (:684-694); net is anything with a .maskiou_net FastMaskIoUNet.  One launch
        sequence (_loss_common.LossFunction) runs the net forward on the CURRENT parameter values, the head, and the backward down to
        the net's input and its parameters.
    maskiou_net_apply(seq, x) -> FastMaskIoUNet.forward: [N,Cin,H,W] -> [N,C], differentiable once in x and the parameters.

Binarisation: a pixel counts as predicted where its logit is > 0.  The reference tests fp32 sigmoid > 0.5, which differs only for
logits in (0, ~6e-8] (their sigmoid rounds to 0.5).  The pool's backward sends the gradient to the first maximum in row-major
order, torch's CPU rule.  CPU tensors raise: there is no CPU path.
"""
from __future__ import annotations

import ctypes as C

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from .. import _lib as L
from ..config import active_cfg
from . import _loss_common as LC
from . import mask_loss as ML


def check_switches(cfg):
    """NotImplementedError naming the cfg field for what the term does not implement."""
    ML.check_switches(cfg)
    if not cfg.mask_proto_crop:
        raise NotImplementedError('yolact_amd mask_iou_loss: cfg.mask_proto_crop = False is not supported (the net\'s input is the '
                                  'cropped mask, what both YOLACT++ configs train with)')
    if cfg.maskious_to_train > 0:
        # the reference's subsample there indexes by masks_to_train (:667); no shipped config sets it
        raise NotImplementedError('yolact_amd mask_iou_loss: cfg.maskious_to_train = %r is not supported (every shipped config '
                                  'trains on all mask-IoU samples: -1)' % (cfg.maskious_to_train,))


def _ws(what, d, dev):
    ws = LC.workspace(what, d, dev)
    d.ws_bytes = ws.numel()
    return ws


# ---- the net's input and the targets ------------------------------------------------------------------------------------------------
def _input_desc(proto, coef, box, img_off):
    B, mh, mw, K = proto.shape
    off = [int(v) for v in img_off]
    if len(off) != B + 1 or tuple(box.shape) != (coef.shape[0], 4) or coef.shape[1] != K:
        raise ValueError('maskiou input: proto %s / coef %s / box %s / %d offsets' % (tuple(proto.shape), tuple(coef.shape),
                                                                                       tuple(box.shape), len(off)))
    dev = proto.device
    off_host, off_dev = LC.offsets(off, dev)
    keep = [LC.f32(proto, dev), LC.f32(coef, dev), LC.f32(box, dev), off_host, off_dev]
    d = L.MaskIouInputDesc()
    d.proto, d.coef, d.box = keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr()
    d.img_off, d.img_off_host = off_dev.data_ptr(), C.cast(off_host, C.c_void_p)
    d.B, d.mh, d.mw, d.K, d.N, d.G = B, mh, mw, K, coef.shape[0], 1
    return d, keep


class MaskIouInput(torch.autograd.Function):
    """apply(proto [B,mh,mw,32], coef [N,32], box [N,4], gt uint8 [G,mh,mw], gt_idx [N], img_off (B + 1 ints)) ->
    (x0 [N,mh,mw], iou_t [N]); x0 is once differentiable in proto and coef."""

    @staticmethod
    def forward(ctx, proto, coef, box, gt, gt_idx, img_off):
        for name, t in (('proto', proto), ('coef', coef), ('box', box), ('gt', gt), ('gt_idx', gt_idx)):
            L.require_cuda(t, 'maskiou input ' + name)
        dev = proto.device
        with torch.cuda.device(dev), torch.no_grad():
            d, keep = _input_desc(proto, coef, box, img_off)
            gtd, gidx = LC.mask_u8(gt, dev), LC.i32(gt_idx, dev)
            if gtd.dim() != 3 or tuple(gtd.shape[1:]) != (d.mh, d.mw) or gidx.numel() != d.N:
                raise ValueError('maskiou input: gt %s / gt_idx %s' % (tuple(gt.shape), tuple(gt_idx.shape)))
            x0 = torch.empty(d.N, d.mh, d.mw, dtype=torch.float32, device=dev)
            iou_t = torch.empty(d.N, dtype=torch.float32, device=dev)
            d.gt, d.gt_idx, d.G, d.x0, d.iou_t = gtd.data_ptr(), gidx.data_ptr(), gtd.shape[0], x0.data_ptr(), iou_t.data_ptr()
            L.check(L.lib().ymi_maskiou_input_f32(C.byref(d), L.stream_ptr()), 'ymi_maskiou_input_f32')
        ctx.save_for_backward(proto, coef, box)
        ctx.img_off = [int(v) for v in img_off]
        ctx.mark_non_differentiable(iou_t)
        return x0, iou_t

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _):
        proto, coef, box = ctx.saved_tensors
        want_p, want_c = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_p or want_c):
            return (None,) * 6
        dev = proto.device
        with torch.cuda.device(dev), torch.no_grad():
            d, keep = _input_desc(proto, coef, box, ctx.img_off)
            gd = LC.f32(g, dev)
            dproto = torch.empty(proto.shape, dtype=torch.float32, device=dev) if want_p else None
            dcoef = torch.empty(coef.shape, dtype=torch.float32, device=dev) if want_c else None
            d.d_x0 = gd.data_ptr()
            d.d_proto = None if dproto is None else dproto.data_ptr()
            d.d_coef = None if dcoef is None else dcoef.data_ptr()
            ws = _ws('MASKIOU_INPUT', d, dev)
            L.check(L.lib().ymi_maskiou_input_bwd_f32(C.byref(d), L.stream_ptr()), 'ymi_maskiou_input_bwd_f32')
        return (None if dproto is None else dproto.to(proto.dtype), None if dcoef is None else dcoef.to(coef.dtype),
                None, None, None, None)


def lincomb_mask_loss_maskiou(pos, idx_t, mask_data, proto_data, masks, gt_box_t, labels):
    """MultiBoxLoss.lincomb_mask_loss under cfg.use_maskiou -> ({'M': 0-dim}, [maskiou_net_input, maskiou_t, label_t] or None);
    the arguments of mask_loss.lincomb_mask_loss and labels = one long tensor of classes per image (the non-crowd annotations)."""
    cfg = active_cfg()
    check_switches(cfg)
    L.require_cuda(proto_data, 'lincomb_mask_loss proto_data')
    L.require_cuda(mask_data, 'lincomb_mask_loss mask_data')
    dev = proto_data.device
    mask_h, mask_w = proto_data.size(1), proto_data.size(2)
    coef, box, gt, gt_idx, img_off, weight, _ = ML.gather_instances(pos, idx_t, mask_data, masks, gt_box_t, mask_h, mask_w,
                                                                    int(cfg.masks_to_train))
    gt_rows = gt if gt.size(0) else torch.zeros(1, mask_h, mask_w, dtype=torch.uint8, device=dev)
    losses = {'M': ML.mask_loss(proto_data, coef, box, gt_rows, gt_idx, img_off, weight, crop=bool(cfg.mask_proto_crop),
                                roi_norm=bool(cfg.mask_proto_normalize_emulate_roi_pooling), alpha=float(cfg.mask_alpha))}
    if coef.size(0) == 0:
        return losses, None
    with torch.no_grad():
        label_t = torch.cat([l.to(dev).long() for l in labels])[gt_idx.long()]           # labels[idx][pos_idx_t]
        if cfg.discard_mask_area > 0:                                                    # :630-640
            area = gt.reshape(gt.size(0), -1).ne(0).sum(1)[gt_idx.long()]
            select = area > cfg.discard_mask_area
            image = torch.bucketize(torch.arange(coef.size(0), device=dev), img_off[1:].long(), right=True)
            kept = torch.cumsum(torch.bincount(image[select], minlength=img_off.numel() - 1), 0)
            off = [0] + kept.tolist()                    # one host sync for the offsets, one below for the rows
            if off[-1] == 0:
                return losses, None
            rows = select.nonzero().view(-1)
        else:
            off, rows = img_off.tolist(), None
    if rows is not None:
        coef, box, gt_idx, label_t = coef[rows], box[rows], gt_idx[rows], label_t[rows]
    x0, maskiou_t = MaskIouInput.apply(proto_data, coef, box, gt, gt_idx, off)
    return losses, [x0.unsqueeze(1), maskiou_t, label_t]


# ---- FastMaskIoUNet: forward and backward on the direct convolution kernels -------------------------------------------------------------
def net_layers(seq):
    """The make_net Sequential (Conv2d, ReLU, Conv2d, ReLU, ..) -> ([conv modules], [(kh, kw, stride, pad, relu)])."""
    mods = list(seq)
    convs, geo = [], []
    for i, m in enumerate(mods):
        if isinstance(m, nn.Conv2d):
            if (m.stride[0] != m.stride[1] or m.padding[0] != m.padding[1] or tuple(m.dilation) != (1, 1) or m.groups != 1
                    or m.bias is None or isinstance(m.padding, str)):
                raise NotImplementedError('yolact_amd FastMaskIoUNet: %r is not a plain square-stride biased convolution' % (m,))
            relu = i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)
            convs.append(m)
            geo.append((m.kernel_size[0], m.kernel_size[1], m.stride[0], m.padding[0], int(relu)))
        elif not isinstance(m, nn.ReLU):
            raise NotImplementedError('yolact_amd FastMaskIoUNet: layer %r is not implemented' % (m,))
    if not convs:
        raise ValueError('yolact_amd FastMaskIoUNet: no convolution')
    return convs, tuple(geo)


def _pack(w):
    """[Cout,Cin,kh,kw] -> [kh*kw*Cin, ceil4(Cout)] fp32, the layout of ymi_conv2d_direct_nhwc_f32 (a permute of the CURRENT values)."""
    Cout, Cin, kh, kw = w.shape
    out = torch.zeros(kh * kw * Cin, (Cout + 3) // 4 * 4, dtype=torch.float32, device=w.device)
    out[:, :Cout] = w.detach().float().permute(2, 3, 1, 0).reshape(kh * kw * Cin, Cout)
    return out


def _net_forward(x, params, geo):
    """x [N,H,W,Cin] fp32 contiguous -> (activations [x, y1, .., yL], packed filters, pooled [N,C])."""
    lib, s, dev = L.lib(), L.stream_ptr(), x.device
    acts, packed = [x], []
    for (kh, kw, stride, pad, relu), w, b in zip(geo, params[0::2], params[1::2]):
        N, H, W, Cin = acts[-1].shape
        Cout = w.shape[0]
        if w.shape[1] != Cin or tuple(w.shape[2:]) != (kh, kw) or b.numel() != Cout:
            raise ValueError('FastMaskIoUNet: weight %s / bias %s on %d channels' % (tuple(w.shape), tuple(b.shape), Cin))
        Ho, Wo = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
        if Ho < 1 or Wo < 1:
            raise ValueError('FastMaskIoUNet: a %d x %d map is too small for a %d x %d / %d convolution' % (H, W, kh, kw, stride))
        pk, bias = _pack(w), LC.f32(b, dev)
        y = torch.empty(N, Ho, Wo, Cout, dtype=torch.float32, device=dev)
        L.check(lib.ymi_conv2d_direct_nhwc_f32(acts[-1].data_ptr(), pk.data_ptr(), bias.data_ptr(), y.data_ptr(), N, H, W, Cin, Ho, Wo,
                                               Cout, kh, kw, stride, pad, relu, s), 'FastMaskIoUNet conv')
        acts.append(y)
        packed.append(pk)
    N, H, W, Cc = acts[-1].shape
    pool = torch.empty(N, Cc, dtype=torch.float32, device=dev)
    L.check(lib.ymi_global_maxpool_nhwc_f32(acts[-1].data_ptr(), pool.data_ptr(), N, H * W, Cc, s), 'FastMaskIoUNet max')
    return acts, packed, pool


def _net_backward(acts, packed, geo, d_pool, want_x, want_p):
    """d_pool [N,C] -> (dx [N,H,W,Cin] or None, [dw [Cout,Cin,kh,kw], db [Cout], ..] with None where not wanted)."""
    lib, s, dev = L.lib(), L.stream_ptr(), d_pool.device
    N, H, W, Cc = acts[-1].shape
    dy = torch.empty_like(acts[-1])
    L.check(lib.ymi_global_maxpool_bwd_nhwc_f32(acts[-1].data_ptr(), d_pool.data_ptr(), dy.data_ptr(), N, H * W, Cc, s),
            'FastMaskIoUNet max backward')
    grads = [None] * (2 * len(geo))
    first = min([i for i in range(len(geo)) if want_p[2 * i] or want_p[2 * i + 1]] or [len(geo)])
    for i in reversed(range(len(geo))):
        if not want_x and i < first:
            break
        kh, kw, stride, pad, relu = geo[i]
        x, y = acts[i], acts[i + 1]
        d = L.ConvBwdDesc()
        d.x, d.w, d.y, d.dy = x.data_ptr(), packed[i].data_ptr(), y.data_ptr(), dy.data_ptr()
        d.B, d.H, d.W, d.Cin = x.shape
        d.Ho, d.Wo, d.Cout = y.shape[1:]
        d.kh, d.kw, d.stride, d.pad, d.relu = kh, kw, stride, pad, relu
        dx = torch.empty_like(x) if (want_x or i > first) else None
        want_w = want_p[2 * i] or want_p[2 * i + 1]
        dw = torch.empty_like(packed[i]) if want_w else None
        db = torch.empty(y.shape[3], dtype=torch.float32, device=dev) if want_w else None
        d.dx, d.dw, d.db = (None if t is None else t.data_ptr() for t in (dx, dw, db))
        ws = _ws('CONV_BWD', d, dev) if want_w else None
        L.check(lib.ymi_conv2d_bwd_nhwc_f32(C.byref(d), s), 'ymi_conv2d_bwd_nhwc_f32')
        if want_w:
            Cout, Cin = y.shape[3], x.shape[3]
            grads[2 * i] = dw[:, :Cout].reshape(kh, kw, Cin, Cout).permute(3, 2, 0, 1).contiguous() if want_p[2 * i] else None
            grads[2 * i + 1] = db if want_p[2 * i + 1] else None
        dy = dx
    return (dy if want_x else None), grads


def _nhwc(x):
    if x.dim() != 4:
        raise ValueError('FastMaskIoUNet: the input must be [N,C,H,W], got %s' % (tuple(x.shape),))
    return x.detach().float().permute(0, 2, 3, 1).contiguous()


class MaskIouNet(torch.autograd.Function):
    """apply(geo, x [N,Cin,H,W], w1, b1, .., wL, bL) -> [N,C]: the convolutions, ReLUs and the global max-pool."""

    @staticmethod
    def forward(ctx, geo, x, *params):
        with torch.cuda.device(x.device), torch.no_grad():
            acts, packed, pool = _net_forward(_nhwc(x), params, geo)
        # the activations and the packed filters are this call's own copies; the inputs are saved too, so that autograd's version
        # check refuses a backward after x or a parameter was edited in place
        ctx.save_for_backward(x, *params)
        ctx.geo, ctx.acts, ctx.packed = geo, acts, packed
        ctx.dtypes = [x.dtype] + [p.dtype for p in params]
        return pool

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        need = ctx.needs_input_grad
        ctx.saved_tensors                                # (the version check)
        with torch.cuda.device(g.device), torch.no_grad():
            dx, grads = _net_backward(ctx.acts, ctx.packed, ctx.geo, g.float().contiguous(), need[1], need[2:])
        out = [None if dx is None else dx.permute(0, 3, 1, 2)] + grads
        return (None,) + tuple(None if t is None else t.to(dt) for t, dt in zip(out, ctx.dtypes))


def maskiou_net_apply(seq, x):
    """FastMaskIoUNet.forward: seq = its .maskiou_net Sequential."""
    L.require_cuda(x, 'FastMaskIoUNet input')
    convs, geo = net_layers(seq)
    params = []
    for m in convs:
        L.require_cuda(m.weight, 'FastMaskIoUNet weight')
        params += [m.weight, m.bias]
    return MaskIouNet.apply(geo, x, *params)


def _launch_loss(*args):
    """(x, w1, b1, .., wL, bL, iou_t, label_t, alpha, geo, *want) -> (loss [1], dx, dw1, db1, ..): ONE launch sequence."""
    n = (len(args) - 6) // 2                          # 1 + n differentiable inputs, 4 others, 1 + n wants
    x, params, (iou_t, label_t, alpha, geo), want = args[0], args[1:1 + n], args[1 + n:5 + n], args[5 + n:]
    dev = x.device
    with torch.cuda.device(dev), torch.no_grad():
        acts, packed, pool = _net_forward(_nhwc(x), params, geo)
        N, Cc = pool.shape
        iou, lab = LC.f32(iou_t, dev), LC.i32(label_t, dev)
        if iou.numel() != N or lab.numel() != N:
            raise ValueError('mask_iou_loss: %d inputs, %d targets, %d labels' % (N, iou.numel(), lab.numel()))
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        d_pool = torch.empty_like(pool) if any(want) else None
        d = L.MaskIouHeadDesc()
        d.pool, d.iou_t, d.label, d.loss = pool.data_ptr(), iou.data_ptr(), lab.data_ptr(), loss.data_ptr()
        d.d_pool = None if d_pool is None else d_pool.data_ptr()
        d.N, d.C, d.alpha = N, Cc, float(alpha)
        ws = _ws('MASKIOU_HEAD', d, dev)
        L.check(L.lib().ymi_maskiou_head_f32(C.byref(d), L.stream_ptr()), 'ymi_maskiou_head_f32')
        if d_pool is None:
            return (loss,) + (None,) * (1 + n)
        dx, grads = _net_backward(acts, packed, geo, d_pool, want[0], want[1:])
        return (loss, None if dx is None else dx.permute(0, 3, 1, 2)) + tuple(grads)


def mask_iou_loss(net, maskiou_targets):
    """MultiBoxLoss.mask_iou_loss (:684-694) -> the 0-dim loss, differentiable once in maskiou_net_input and net.maskiou_net's
    parameters."""
    cfg = active_cfg()
    check_switches(cfg)
    maskiou_net_input, maskiou_t, label_t = maskiou_targets
    L.require_cuda(maskiou_net_input, 'mask_iou_loss maskiou_net_input')
    convs, geo = net_layers(net.maskiou_net.maskiou_net)
    params = []
    for m in convs:
        L.require_cuda(m.weight, 'mask_iou_loss weight')
        params += [m.weight, m.bias]
    return LC.LossFunction.apply(_launch_loss, 1 + len(params), maskiou_net_input, *params, maskiou_t, label_t,
                                 float(cfg.maskiou_alpha), geo)
