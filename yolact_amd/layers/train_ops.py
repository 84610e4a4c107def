"""Differentiable building blocks of the train-mode heads, protonet and FPN on the HIP kernels (csrc/conv_train.hip and the conv
engine).

    conv2d_act(x, weight, bias, padding, act)            -> y [B,H,W,Cout]: act(conv(x, weight) + bias), act in {None, 'relu', 'tanh'}
    conv2d_multi(x, [(weight, bias, act), ..], padding)  -> one y per entry: up to three convolutions of the SAME input as one launch
                                                            (the head's bbox / conf / mask layers, yolact.py:169-173)
    upsample2x(x, relu)                                  -> [B,2H,2W,C]: F.interpolate(scale_factor=2, bilinear, align_corners=False)

    conv2d_down(x, weight, bias, act)                    -> [B,Ho,Wo,Cout]: the same at stride 2 with padding k // 2 (the FPN's
                                                            downsample layers, yolact.py:349-351); 3x3 and 1x1, Cin % 32 == 0
    upsample_add(top, lat)                               -> F.interpolate(top, size of lat, bilinear, align_corners=False) + lat (the
                                                            FPN's top-down sum, yolact.py:332-334), any size of lat >= that of top

    conv2d_plain(x, weight, stride)                      -> [B,Ho,Wo,Cout]: a bias-free convolution, 3x3 / pad 1 or 1x1 / pad 0 at stride 1 or 2
                                                            (the backbone's convolutions, backbone.py:19-31); Cin % 32 == 0
    batch_norm_act(x, bn, batch_stats, residual, relu)   -> relu(bn(x) + residual) for an nn.BatchNorm2d, batch statistics or frozen
    bottleneck(x, block, batch_stats)                    -> a modules.Bottleneck (backbone.py:37-57); bn3 + shortcut + ReLU are one launch

x and the results are NHWC fp32 GPU tensors; weight and bias are nn.Conv2d parameters in torch layout.  Everything is once
differentiable in x, every weight and every bias.  Each call packs its filters from the CURRENT parameter values (a permute; no
cache), launches only what needs_input_grad asks for, and saves its inputs, so autograd's version check refuses a backward after an
in-place edit.  Geometry: 3x3 / stride 1 / pad 1 and 1x1 / pad 0, Cin % 32 == 0, any Cout; anything else raises NotImplementedError
naming it.  CPU tensors raise: there is no CPU path.

Launches of one convolution's backward: ymi_act_bwd_f32 per output (g = dy * act'(y), side by side in one buffer whose channel stride
is padded to a multiple of 32, padding zeroed), ymi_conv_wgrad_nhwc_f32 once over all outputs (dw, db), ymi_conv2d_nhwc_f32 once on g
with the filters flipped in both taps and transposed in (Cin, Cout) (dx).  conv2d_down: the same with ymi_conv_wgrad_desc.stride = 2;
its dx first spreads g over a zeroed [B,H,W,ldg] buffer (gz[:, ::2, ::2] = g) and then runs the stride-1 data gradient on it, which
spends four times the useful FLOPs (fine for the FPN's 18 x 18 and 9 x 9 maps, not for a backbone).  upsample_add: d_lat = dy,
d_top = ymi_bilinear_size_bwd_nhwc_f32 (a gather in a fixed order).  conv2d_plain: dw from ymi_conv_wgrad_nhwc_f32 with db = NULL; dx at
stride 1 from the flipped-filter engine launch, at stride 2 from ymi_conv_dgrad_s2_nhwc_f32 (csrc/conv_dgrad.hip: only the taps that
exist, no zero-filled buffer).  batch_norm_act: ymi_bn_fwd_nhwc_f32 / ymi_bn_bwd_nhwc_f32 (csrc/bn_train.hip).
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from .. import _lib as L
from . import _loss_common as LC

ACTS = {None: L.ACT_NONE, 'none': L.ACT_NONE, 'relu': L.ACT_RELU, 'tanh': L.ACT_TANH}


def _ceil(a, b):
    return (a + b - 1) // b * b


def check_conv(weight, padding, stride=1, dilation=1, groups=1, who='conv2d_act'):
    """NotImplementedError naming what of a convolution's geometry the kernels do not take -> (kh, pad)."""
    pair = lambda v: (int(v), int(v)) if isinstance(v, int) else tuple(int(e) for e in v)
    if isinstance(padding, str):
        raise NotImplementedError('yolact_amd %s: padding = %r is not supported (an integer padding is)' % (who, padding))
    stride, dilation, padding = pair(stride), pair(dilation), pair(padding)
    Cout, Cin, kh, kw = weight.shape
    if stride != (1, 1):
        raise NotImplementedError('yolact_amd %s: stride = %r is not supported (stride 1 is)' % (who, stride))
    if dilation != (1, 1):
        raise NotImplementedError('yolact_amd %s: dilation = %r is not supported (dilation 1 is)' % (who, dilation))
    if groups != 1:
        raise NotImplementedError('yolact_amd %s: groups = %r is not supported (groups 1 is)' % (who, groups))
    if (kh, kw, padding) not in (((3, 3, (1, 1))), (1, 1, (0, 0))):
        raise NotImplementedError('yolact_amd %s: a %d x %d kernel with padding = %r is not supported (3 x 3 / padding 1 and '
                                  '1 x 1 / padding 0 are)' % (who, kh, kw, padding))
    if Cin % 32 != 0:
        raise NotImplementedError('yolact_amd %s: Cin = %d is not supported (a multiple of 32 input channels is)' % (who, Cin))
    return kh, padding[0]


def _engine_conv(x, ldx, wpk, bias, Cin, Cout, k, pad, segs, stride=1):
    """One ymi_conv2d_nhwc_f32 launch on the exact-fp32 tiles: x [B,H,W,ldx], wpk [CoutPad][k*k*Cin], segs = (n0, n1, act, tensor)."""
    B, H, W = x.shape[:3]
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    d = L.ConvDesc()
    d.x, d.w, d.bias = x.data_ptr(), wpk.data_ptr(), (None if bias is None else bias.data_ptr())
    d.B, d.H, d.W, d.Cin, d.ldx, d.Ho, d.Wo, d.Cout = B, H, W, Cin, ldx, Ho, Wo, Cout
    d.kh, d.kw, d.stride, d.pad, d.Kpad, d.tile = k, k, stride, pad, k * k * Cin, L.TILE_AUTO
    d.nseg = len(segs)
    for i, (n0, n1, act, y) in enumerate(segs):
        d.seg[i] = L.ConvSeg(n0, n1, act, n1 - n0, Ho * Wo * (n1 - n0), y.data_ptr())
    L.check(L.lib().ymi_conv2d_nhwc_f32(C.byref(d), L.stream_ptr()), 'ymi_conv2d_nhwc_f32')


def _pack_forward(wcat):
    """[Cout,Cin,kh,kw] -> [ceil128(Cout)][kh*kw*Cin], k = (ky*kw + kx)*Cin + c (a permute of the CURRENT values)."""
    Cout, Cin, kh, kw = wcat.shape
    out = torch.zeros(_ceil(Cout, 128), kh * kw * Cin, dtype=torch.float32, device=wcat.device)
    out[:Cout] = wcat.permute(0, 2, 3, 1).reshape(Cout, kh * kw * Cin)
    return out


def _pack_dgrad(wcat, ldg):
    """The filters of the data gradient: flipped in both taps, transposed in (Cin, Cout), Cout padded to ldg with zeros ->
    [ceil128(Cin)][kh*kw*ldg]."""
    Cout, Cin, kh, kw = wcat.shape
    t = F.pad(wcat.flip(2, 3).permute(1, 2, 3, 0), (0, ldg - Cout))          # [Cin,kh,kw,ldg]
    out = torch.zeros(_ceil(Cin, 128), kh * kw * ldg, dtype=torch.float32, device=wcat.device)
    out[:Cin] = t.reshape(Cin, kh * kw * ldg)
    return out


class ConvMulti(torch.autograd.Function):
    """apply(k, pad, acts, x, w1, b1, .., wn, bn) -> (y1, .., yn)."""

    @staticmethod
    def forward(ctx, k, pad, acts, x, *params):
        dev = x.device
        ws, bs = params[0::2], params[1::2]
        couts = [int(w.shape[0]) for w in ws]
        Cin = int(ws[0].shape[1])
        with torch.cuda.device(dev), torch.no_grad():
            xd = LC.f32(x, dev)
            B, H, W, _ = xd.shape
            wcat = torch.cat([w.detach().float() for w in ws], 0) if len(ws) > 1 else ws[0].detach().float()
            bcat = torch.cat([b.detach().float() for b in bs], 0).contiguous()
            ys, segs, n0 = [], [], 0
            for co, a in zip(couts, acts):
                y = torch.empty(B, H, W, co, dtype=torch.float32, device=dev)
                ys.append(y)
                segs.append((n0, n0 + co, a, y))
                n0 += co
            _engine_conv(xd, Cin, _pack_forward(wcat), bcat, Cin, n0, k, pad, segs)
        # the outputs are this call's own tensors; the inputs are saved too, so that autograd's version check refuses a backward
        # after x or a parameter was edited in place
        ctx.save_for_backward(x, *params, *ys)
        ctx.k, ctx.pad, ctx.acts, ctx.couts = k, pad, acts, couts
        ctx.dtypes = [x.dtype] + [p.dtype for p in params]
        return tuple(ys)

    @staticmethod
    @once_differentiable
    def backward(ctx, *dys):
        need = ctx.needs_input_grad[3:]
        saved = ctx.saved_tensors                         # (the version check)
        n = len(ctx.couts)
        x, params, ys = saved[0], saved[1:1 + 2 * n], saved[1 + 2 * n:]
        want_x, want_p = need[0], need[1:]
        if not any(need):
            return (None,) * (3 + len(need))
        dev = x.device
        lib, s = L.lib(), L.stream_ptr()
        k, pad, couts = ctx.k, ctx.pad, ctx.couts
        with torch.cuda.device(dev), torch.no_grad():
            xd = LC.f32(x, dev)
            B, H, W, Cin = xd.shape
            npos, ctot = B * H * W, sum(couts)
            ldg = _ceil(ctot, 32)
            g = torch.empty(B, H, W, ldg, dtype=torch.float32, device=dev)
            n0, keep = 0, []
            for i, (co, a, y, dy) in enumerate(zip(couts, ctx.acts, ys, dys)):
                dyd = torch.zeros_like(y) if dy is None else LC.f32(dy, dev)
                keep.append(dyd)
                cpad = co + (ldg - ctot if i == len(couts) - 1 else 0)
                L.check(lib.ymi_act_bwd_f32(y.data_ptr(), dyd.data_ptr(), g.data_ptr() + 4 * n0, npos, co, cpad, co, co, ldg, a, s),
                        'ymi_act_bwd_f32')
                n0 += co
            grads = [None] * len(params)
            want_w, want_b = any(want_p[0::2]), any(want_p[1::2])
            if want_w or want_b:
                d = L.ConvWgradDesc()
                dw = torch.empty(k * k * Cin, ctot, dtype=torch.float32, device=dev) if want_w else None
                db = torch.empty(ctot, dtype=torch.float32, device=dev) if want_b else None
                d.x, d.g = xd.data_ptr(), g.data_ptr()
                d.dw, d.db = (None if t is None else t.data_ptr() for t in (dw, db))
                d.B, d.H, d.W, d.Cin, d.Cout, d.ldg, d.kh, d.kw, d.pad = B, H, W, Cin, ctot, ldg, k, k, pad
                ws = LC.workspace('CONV_WGRAD', d, dev)
                d.ws_bytes = ws.numel()
                L.check(lib.ymi_conv_wgrad_nhwc_f32(C.byref(d), s), 'ymi_conv_wgrad_nhwc_f32')
                n0 = 0
                for i, co in enumerate(couts):
                    if want_p[2 * i]:
                        grads[2 * i] = dw[:, n0:n0 + co].reshape(k, k, Cin, co).permute(3, 2, 0, 1).contiguous()
                    if want_p[2 * i + 1]:
                        grads[2 * i + 1] = db[n0:n0 + co].clone()
                    n0 += co
            dx = None
            if want_x:
                wcat = torch.cat([w.detach().float() for w in params[0::2]], 0)
                dx = torch.empty(B, H, W, Cin, dtype=torch.float32, device=dev)
                _engine_conv(g, ldg, _pack_dgrad(wcat, ldg), None, ldg, Cin, k, k - 1 - pad, [(0, Cin, L.ACT_NONE, dx)])
        out = [dx] + grads
        return (None, None, None) + tuple(None if t is None else t.to(dt) for t, dt in zip(out, ctx.dtypes))


def conv2d_multi(x, layers, padding, stride=1, dilation=1, groups=1):
    """layers = [(weight, bias, act), ..] (one to three convolutions of equal geometry on the same x) -> tuple of NHWC outputs."""
    L.require_cuda(x, 'conv2d_act x')
    if not 1 <= len(layers) <= 3:
        raise ValueError('conv2d_multi: one to three convolutions share a launch, got %d' % len(layers))
    if x.dim() != 4:
        raise ValueError('conv2d_act: x must be [B,H,W,Cin], got %s' % (tuple(x.shape),))
    params, acts, geo = [], [], None
    for w, b, act in layers:
        L.require_cuda(w, 'conv2d_act weight')
        if act not in ACTS:
            raise NotImplementedError('yolact_amd conv2d_act: act = %r is not supported (None, \'relu\' and \'tanh\' are)' % (act,))
        if b is None:
            raise NotImplementedError('yolact_amd conv2d_act: bias = None is not supported (a biased convolution is)')
        g = check_conv(w, padding, stride, dilation, groups) + (int(w.shape[1]),)
        if geo is not None and g != geo:
            raise ValueError('conv2d_multi: the convolutions differ in geometry: %r and %r' % (geo, g))
        geo = g
        if b.numel() != w.shape[0]:
            raise ValueError('conv2d_act: weight %s / bias %s' % (tuple(w.shape), tuple(b.shape)))
        params += [w, b]
        acts.append(ACTS[act])
    if x.shape[3] != geo[2]:
        raise ValueError('conv2d_act: x %s has %d channels, the weight takes %d' % (tuple(x.shape), x.shape[3], geo[2]))
    return ConvMulti.apply(geo[0], geo[1], tuple(acts), x, *params)


def conv2d_act(x, weight, bias, padding, act=None, stride=1, dilation=1, groups=1):
    """act(conv2d(x, weight, bias, padding)) on NHWC x -> NHWC."""
    return conv2d_multi(x, [(weight, bias, act)], padding, stride, dilation, groups)[0]


class Upsample2x(torch.autograd.Function):
    """apply(x [B,H,W,C], relu) -> [B,2H,2W,C]."""

    @staticmethod
    def forward(ctx, x, relu):
        dev = x.device
        with torch.cuda.device(dev), torch.no_grad():
            xd = LC.f32(x, dev)
            B, H, W, Cc = xd.shape
            y = torch.empty(B, 2 * H, 2 * W, Cc, dtype=torch.float32, device=dev)
            L.check(L.lib().ymi_bilinear_nhwc_f32(xd.data_ptr(), y.data_ptr(), B, H, W, Cc, 2 * H, 2 * W, 0.5, 0.5, int(relu),
                                                  L.stream_ptr()), 'ymi_bilinear_nhwc_f32')
        ctx.save_for_backward(*((x, y) if relu else (x,)))
        ctx.relu, ctx.dtype = int(relu), x.dtype
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, y = (tuple(ctx.saved_tensors) + (None,))[:2]   # (the version check)
        if not ctx.needs_input_grad[0]:
            return None, None
        dev = x.device
        with torch.cuda.device(dev), torch.no_grad():
            B, H, W, Cc = x.shape
            dyd = LC.f32(dy, dev)
            dx = torch.empty(B, H, W, Cc, dtype=torch.float32, device=dev)
            L.check(L.lib().ymi_bilinear_bwd_nhwc_f32(dyd.data_ptr(), None if y is None else y.data_ptr(), dx.data_ptr(),
                                                      B, H, W, Cc, 2 * H, 2 * W, ctx.relu, L.stream_ptr()),
                    'ymi_bilinear_bwd_nhwc_f32')
        return dx.to(ctx.dtype), None


def upsample2x(x, relu=False):
    """F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=False) (+ ReLU) on NHWC x."""
    L.require_cuda(x, 'upsample2x x')
    if x.dim() != 4 or x.shape[3] % 4 != 0:
        raise NotImplementedError('yolact_amd upsample2x: x %s is not supported ([B,H,W,C] with C %% 4 == 0 is)' % (tuple(x.shape),))
    return Upsample2x.apply(x, bool(relu))


def check_down(weight, who='conv2d_down'):
    """NotImplementedError naming what of a stride-2 convolution's geometry the kernels do not take -> (k, pad = k // 2)."""
    if weight.dim() != 4:
        raise NotImplementedError('yolact_amd %s: a weight of shape %s is not supported ([Cout,Cin,k,k] is)' % (who, tuple(weight.shape)))
    Cout, Cin, kh, kw = weight.shape
    if (kh, kw) not in ((3, 3), (1, 1)):
        raise NotImplementedError('yolact_amd %s: a %d x %d kernel at stride 2 is not supported (3 x 3 / padding 1 and 1 x 1 / '
                                  'padding 0 are)' % (who, kh, kw))
    if Cin % 32 != 0:
        raise NotImplementedError('yolact_amd %s: Cin = %d is not supported (a multiple of 32 input channels is)' % (who, Cin))
    return kh, kh // 2


class ConvDown(torch.autograd.Function):
    """apply(k, act, x [B,H,W,Cin], weight, bias) -> y [B,Ho,Wo,Cout], Ho = (H + 2 (k // 2) - k) // 2 + 1: a stride-2 convolution."""

    @staticmethod
    def forward(ctx, k, act, x, weight, bias):
        dev = x.device
        Cout, Cin = int(weight.shape[0]), int(weight.shape[1])
        pad = k // 2
        with torch.cuda.device(dev), torch.no_grad():
            xd = LC.f32(x, dev)
            B, H, W, _ = xd.shape
            y = torch.empty(B, (H + 2 * pad - k) // 2 + 1, (W + 2 * pad - k) // 2 + 1, Cout, dtype=torch.float32, device=dev)
            _engine_conv(xd, Cin, _pack_forward(weight.detach().float()), LC.f32(bias, dev), Cin, Cout, k, pad, [(0, Cout, act, y)],
                         stride=2)
        ctx.save_for_backward(x, weight, bias, y)          # (the inputs: autograd's version check)
        ctx.k, ctx.act = k, act
        ctx.dtypes = [x.dtype, weight.dtype, bias.dtype]
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        want_x, want_w, want_b = ctx.needs_input_grad[2:]
        x, weight, bias, y = ctx.saved_tensors
        if not (want_x or want_w or want_b):
            return (None,) * 5
        dev = x.device
        lib, s = L.lib(), L.stream_ptr()
        k, pad = ctx.k, ctx.k // 2
        with torch.cuda.device(dev), torch.no_grad():
            xd = LC.f32(x, dev)
            B, H, W, Cin = xd.shape
            _, Ho, Wo, Cout = y.shape
            ldg = _ceil(Cout, 32)
            dyd = LC.f32(dy, dev)
            g = torch.empty(B, Ho, Wo, ldg, dtype=torch.float32, device=dev)
            L.check(lib.ymi_act_bwd_f32(y.data_ptr(), dyd.data_ptr(), g.data_ptr(), B * Ho * Wo, Cout, ldg, Cout, Cout, ldg, ctx.act, s),
                    'ymi_act_bwd_f32')
            dw = db = dx = None
            if want_w or want_b:
                d = L.ConvWgradDesc()
                dwf = torch.empty(k * k * Cin, Cout, dtype=torch.float32, device=dev) if want_w else None
                db = torch.empty(Cout, dtype=torch.float32, device=dev) if want_b else None
                d.x, d.g = xd.data_ptr(), g.data_ptr()
                d.dw, d.db = (None if t is None else t.data_ptr() for t in (dwf, db))
                d.B, d.H, d.W, d.Cin, d.Cout, d.ldg, d.kh, d.kw, d.pad, d.stride = B, H, W, Cin, Cout, ldg, k, k, pad, 2
                ws = LC.workspace('CONV_WGRAD', d, dev)
                d.ws_bytes = ws.numel()
                L.check(lib.ymi_conv_wgrad_nhwc_f32(C.byref(d), s), 'ymi_conv_wgrad_nhwc_f32')
                if want_w:
                    dw = dwf.reshape(k, k, Cin, Cout).permute(3, 2, 0, 1).contiguous()
            if want_x:
                # g with zeros between its pixels, exactly H x W (even and odd sizes), then the stride-1 data gradient: the added
                # zeros change no bit of a sum, and a pixel no window reads (1x1) gets an exact +0.0.  Four times the useful FLOPs.
                gz = torch.zeros(B, H, W, ldg, dtype=torch.float32, device=dev)
                gz[:, ::2, ::2] = g
                dx = torch.empty(B, H, W, Cin, dtype=torch.float32, device=dev)
                _engine_conv(gz, ldg, _pack_dgrad(weight.detach().float(), ldg), None, ldg, Cin, k, k - 1 - pad, [(0, Cin, L.ACT_NONE, dx)])
        out = [dx, dw, db]
        return (None, None) + tuple(None if t is None else t.to(dt) for t, dt in zip(out, ctx.dtypes))


def conv2d_down(x, weight, bias, act=None):
    """act(conv2d(x, weight, bias, stride=2, padding=k // 2)) on NHWC x -> NHWC: 3 x 3 / pad 1 and 1 x 1 / pad 0, Cin % 32 == 0."""
    L.require_cuda(x, 'conv2d_down x')
    L.require_cuda(weight, 'conv2d_down weight')
    if act not in ACTS:
        raise NotImplementedError('yolact_amd conv2d_down: act = %r is not supported (None, \'relu\' and \'tanh\' are)' % (act,))
    if bias is None:
        raise NotImplementedError('yolact_amd conv2d_down: bias = None is not supported (a biased convolution is)')
    k, _ = check_down(weight)
    if x.dim() != 4 or x.shape[3] != weight.shape[1]:
        raise ValueError('conv2d_down: x %s for a weight %s ([B,H,W,Cin] is expected)' % (tuple(x.shape), tuple(weight.shape)))
    if bias.numel() != weight.shape[0]:
        raise ValueError('conv2d_down: weight %s / bias %s' % (tuple(weight.shape), tuple(bias.shape)))
    return ConvDown.apply(k, ACTS[act], x, weight, bias)


class UpsampleAdd(torch.autograd.Function):
    """apply(top [B,h,w,C], lat [B,H,W,C]) -> bilinear(top -> H x W) + lat."""

    @staticmethod
    def forward(ctx, top, lat):
        dev = lat.device
        with torch.cuda.device(dev), torch.no_grad():
            td = LC.f32(top, dev)
            y = lat.detach().to(torch.float32).clone(memory_format=torch.contiguous_format)     # never write into an autograd input
            B, H, W, Cc = y.shape
            L.check(L.lib().ymi_bilinear_add_nhwc_f32(td.data_ptr(), y.data_ptr(), B, td.shape[1], td.shape[2], Cc, H, W, None,
                                                      L.stream_ptr()), 'ymi_bilinear_add_nhwc_f32')
        ctx.save_for_backward(top, lat)                     # (the version check)
        ctx.dtypes = (top.dtype, lat.dtype)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        top, lat = ctx.saved_tensors
        want_top, want_lat = ctx.needs_input_grad
        d_top = None
        if want_top:
            dev = top.device
            with torch.cuda.device(dev), torch.no_grad():
                dyd = LC.f32(dy, dev)
                B, h, w, Cc = top.shape
                d_top = torch.empty(B, h, w, Cc, dtype=torch.float32, device=dev)
                L.check(L.lib().ymi_bilinear_size_bwd_nhwc_f32(dyd.data_ptr(), d_top.data_ptr(), B, h, w, Cc, dyd.shape[1], dyd.shape[2],
                                                               L.stream_ptr()), 'ymi_bilinear_size_bwd_nhwc_f32')
            d_top = d_top.to(ctx.dtypes[0])
        return d_top, (dy.to(ctx.dtypes[1]) if want_lat else None)


def upsample_add(top, lat):
    """F.interpolate(top, size=lat.shape[1:3], mode='bilinear', align_corners=False) + lat on NHWC tensors (the FPN's top-down sum)."""
    L.require_cuda(top, 'upsample_add top')
    L.require_cuda(lat, 'upsample_add lat')
    if top.dim() != 4 or lat.dim() != 4 or top.shape[0] != lat.shape[0] or top.shape[3] != lat.shape[3] or top.shape[3] % 4 != 0:
        raise NotImplementedError('yolact_amd upsample_add: top %s / lat %s is not supported ([B,h,w,C] and [B,H,W,C] with '
                                  'C %% 4 == 0 are)' % (tuple(top.shape), tuple(lat.shape)))
    if top.shape[1] > lat.shape[1] or top.shape[2] > lat.shape[2]:
        raise NotImplementedError('yolact_amd upsample_add: a top map %s larger than the lateral %s is not supported (the backward '
                                  'handles Ho >= Hi, Wo >= Wi)' % (tuple(top.shape[1:3]), tuple(lat.shape[1:3])))
    return UpsampleAdd.apply(top, lat)


class SharedParams(torch.autograd.Function):
    """apply(n, *params) -> n aliases of every parameter, use-major (use 0's parameters, use 1's, ..).  The backward adds a
    parameter's n gradients in use order: g0 + g1 + .. + g(n-1), whatever order autograd ran the uses in."""

    @staticmethod
    def forward(ctx, n, *params):
        ctx.n, ctx.k = n, len(params)
        return tuple(p.view_as(p) for _ in range(n) for p in params)

    @staticmethod
    @once_differentiable
    def backward(ctx, *gs):
        out = []
        for j in range(ctx.k):
            tot = None
            for u in range(ctx.n):
                g = gs[u * ctx.k + j]
                if g is not None:
                    tot = g if tot is None else tot + g
            out.append(tot)
        return (None,) + tuple(out)


def share_params(n, params):
    """[params of use 0, params of use 1, ..]: n lists of aliases whose gradients are summed in use order."""
    params = list(params)
    flat = SharedParams.apply(n, *params)
    return [list(flat[u * len(params):(u + 1) * len(params)]) for u in range(n)]


# ---- the backbone: bias-free convolutions, BatchNorm, the bottleneck ----------------------------------------------------------------------
def check_plain(weight, stride, who='conv2d_plain'):
    """NotImplementedError naming what of a bias-free convolution's geometry the kernels do not take -> (k, pad = k // 2, stride)."""
    stride = (int(stride),) * 2 if isinstance(stride, int) else tuple(int(e) for e in stride)
    if stride not in ((1, 1), (2, 2)):
        raise NotImplementedError('yolact_amd %s: stride = %r is not supported (stride 1 and stride 2 are)' % (who, stride))
    if stride == (2, 2):
        return check_down(weight, who) + (2,)
    if weight.dim() != 4:
        raise NotImplementedError('yolact_amd %s: a weight of shape %s is not supported ([Cout,Cin,k,k] is)' % (who, tuple(weight.shape)))
    k = int(weight.shape[2])
    return check_conv(weight, k // 2, who=who) + (1,)


def _pack_dgrad_s2(w, cpad):
    """The filters of ymi_conv_dgrad_s2_nhwc_f32: [Cout,Cin,k,k] -> [k][k][cpad/4][Cin][4], Cout padded to cpad with zeros."""
    Cout, Cin, k, _ = w.shape
    t = F.pad(w.permute(2, 3, 0, 1), (0, 0, 0, cpad - Cout))                    # [k,k,cpad,Cin]
    return t.reshape(k, k, cpad // 4, 4, Cin).permute(0, 1, 2, 4, 3).contiguous()


class ConvPlain(torch.autograd.Function):
    """apply(k, stride, x [B,H,W,Cin], weight) -> y [B,Ho,Wo,Cout], padding k // 2, no bias."""

    @staticmethod
    def forward(ctx, k, stride, x, weight):
        dev = x.device
        Cout, Cin = int(weight.shape[0]), int(weight.shape[1])
        pad = k // 2
        with torch.cuda.device(dev), torch.no_grad():
            xd = LC.f32(x, dev)
            B, H, W, _ = xd.shape
            y = torch.empty(B, (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1, Cout, dtype=torch.float32, device=dev)
            _engine_conv(xd, Cin, _pack_forward(weight.detach().float()), None, Cin, Cout, k, pad, [(0, Cout, L.ACT_NONE, y)],
                         stride=stride)
        ctx.save_for_backward(x, weight)                   # (the inputs: autograd's version check)
        ctx.k, ctx.stride, ctx.oshape = k, stride, tuple(y.shape)
        ctx.dtypes = [x.dtype, weight.dtype]
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        want_x, want_w = ctx.needs_input_grad[2:]
        x, weight = ctx.saved_tensors
        if not (want_x or want_w):
            return (None,) * 4
        dev = x.device
        lib, s = L.lib(), L.stream_ptr()
        k, pad, stride = ctx.k, ctx.k // 2, ctx.stride
        with torch.cuda.device(dev), torch.no_grad():
            xd = LC.f32(x, dev)
            B, H, W, Cin = xd.shape
            _, Ho, Wo, Cout = ctx.oshape
            ldg = _ceil(Cout, 32)
            g = LC.f32(dy, dev)
            if ldg != Cout:                                # (no backbone layer: their widths are multiples of 32)
                g = F.pad(g, (0, ldg - Cout))
            dw = dx = None
            if want_w:
                d = L.ConvWgradDesc()
                dwf = torch.empty(k * k * Cin, Cout, dtype=torch.float32, device=dev)
                d.x, d.g, d.dw, d.db = xd.data_ptr(), g.data_ptr(), dwf.data_ptr(), None
                d.B, d.H, d.W, d.Cin, d.Cout, d.ldg, d.kh, d.kw, d.pad, d.stride = B, H, W, Cin, Cout, ldg, k, k, pad, stride
                ws = LC.workspace('CONV_WGRAD', d, dev)
                d.ws_bytes = ws.numel()
                L.check(lib.ymi_conv_wgrad_nhwc_f32(C.byref(d), s), 'ymi_conv_wgrad_nhwc_f32')
                dw = dwf.reshape(k, k, Cin, Cout).permute(3, 2, 0, 1).contiguous()
            if want_x:
                dx = torch.empty(B, H, W, Cin, dtype=torch.float32, device=dev)
                wf = weight.detach().float()
                if stride == 1:
                    _engine_conv(g, ldg, _pack_dgrad(wf, ldg), None, ldg, Cin, k, k - 1 - pad, [(0, Cin, L.ACT_NONE, dx)])
                else:
                    wpk = _pack_dgrad_s2(wf, ldg)
                    d = L.ConvDgradDesc()
                    d.g, d.w, d.dx = g.data_ptr(), wpk.data_ptr(), dx.data_ptr()
                    d.B, d.H, d.W, d.Cin, d.Cout, d.ldg, d.kh, d.kw, d.pad, d.stride = B, H, W, Cin, ldg, ldg, k, k, pad, 2
                    L.check(lib.ymi_conv_dgrad_s2_nhwc_f32(C.byref(d), s), 'ymi_conv_dgrad_s2_nhwc_f32')
        out = [dx, dw]
        return (None, None) + tuple(None if t is None else t.to(dt) for t, dt in zip(out, ctx.dtypes))


def conv2d_plain(x, weight, stride=1):
    """conv2d(x, weight, None, stride, padding=k // 2) on NHWC x -> NHWC: 3 x 3 / pad 1 and 1 x 1 / pad 0, stride 1 or 2, Cin % 32 == 0."""
    L.require_cuda(x, 'conv2d_plain x')
    L.require_cuda(weight, 'conv2d_plain weight')
    k, _, st = check_plain(weight, stride)
    if x.dim() != 4 or x.shape[3] != weight.shape[1]:
        raise ValueError('conv2d_plain: x %s for a weight %s ([B,H,W,Cin] is expected)' % (tuple(x.shape), tuple(weight.shape)))
    return ConvPlain.apply(k, st, x, weight)


class BnAct(torch.autograd.Function):
    """apply(stats, relu, eps, momentum, running_mean, running_var, x [..,C], residual or None, gamma, beta) -> y.  stats: batch
    statistics (the running ones are updated in place) or the running ones as they are."""

    @staticmethod
    def forward(ctx, stats, relu, eps, momentum, rmean, rvar, x, residual, gamma, beta):
        dev = x.device
        with torch.cuda.device(dev), torch.no_grad():
            xd = LC.f32(x, dev)
            Cc = xd.shape[-1]
            npos = xd.numel() // Cc
            y = torch.empty_like(xd)
            mean = torch.empty(Cc, dtype=torch.float32, device=dev)
            invstd = torch.empty(Cc, dtype=torch.float32, device=dev)
            rd = None if residual is None else LC.f32(residual, dev)
            gd, bd = LC.f32(gamma, dev), LC.f32(beta, dev)
            d = L.BnDesc()
            d.x, d.res, d.gamma, d.beta = xd.data_ptr(), (None if rd is None else rd.data_ptr()), gd.data_ptr(), bd.data_ptr()
            d.running_mean, d.running_var = rmean.data_ptr(), rvar.data_ptr()
            d.y, d.mean, d.invstd = y.data_ptr(), mean.data_ptr(), invstd.data_ptr()
            d.npos, d.C, d.training, d.relu, d.eps, d.momentum = npos, Cc, int(stats), int(relu), eps, momentum
            ws = LC.workspace('BN', d, dev)
            d.ws_bytes = ws.numel()
            L.check(L.lib().ymi_bn_fwd_nhwc_f32(C.byref(d), L.stream_ptr()), 'ymi_bn_fwd_nhwc_f32')
        # the inputs are saved too: autograd's version check refuses a backward after x or a parameter was edited in place
        ctx.save_for_backward(x, gamma, beta, y, mean, invstd, *(() if residual is None else (residual,)))
        ctx.stats, ctx.relu, ctx.eps = int(stats), int(relu), eps
        ctx.dtypes = [x.dtype, None if residual is None else residual.dtype, gamma.dtype, beta.dtype]
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        want_x, want_r, want_g, want_b = ctx.needs_input_grad[6:]
        x, gamma, beta, y, mean, invstd = ctx.saved_tensors[:6]      # (the version check)
        if not (want_x or want_r or want_g or want_b):
            return (None,) * 10
        dev = x.device
        with torch.cuda.device(dev), torch.no_grad():
            xd, dyd, gd = LC.f32(x, dev), LC.f32(dy, dev), LC.f32(gamma, dev)
            Cc = xd.shape[-1]
            new = lambda like: torch.empty_like(like)
            dx = new(xd) if want_x else None
            # without a ReLU d_res is dy itself
            dres = new(xd) if (want_r and ctx.relu) else None
            dg = torch.empty(Cc, dtype=torch.float32, device=dev) if want_g else None
            db = torch.empty(Cc, dtype=torch.float32, device=dev) if want_b else None
            if dx is not None or dres is not None or dg is not None or db is not None:
                d = L.BnDesc()
                d.x, d.gamma, d.y, d.mean, d.invstd, d.dy = (xd.data_ptr(), gd.data_ptr(), y.data_ptr(), mean.data_ptr(),
                                                             invstd.data_ptr(), dyd.data_ptr())
                d.dx, d.d_res, d.dgamma, d.dbeta = (None if t is None else t.data_ptr() for t in (dx, dres, dg, db))
                d.npos, d.C, d.training, d.relu, d.eps = xd.numel() // Cc, Cc, ctx.stats, ctx.relu, ctx.eps
                ws = LC.workspace('BN', d, dev)
                d.ws_bytes = ws.numel()
                L.check(L.lib().ymi_bn_bwd_nhwc_f32(C.byref(d), L.stream_ptr()), 'ymi_bn_bwd_nhwc_f32')
            if want_r and not ctx.relu:
                dres = dyd
        out = [dx, dres, dg, db]
        return (None,) * 6 + tuple(None if (t is None or dt is None) else t.to(dt) for t, dt in zip(out, ctx.dtypes))


def batch_norm_act(x, bn, batch_stats=None, residual=None, relu=False):
    """relu(bn(x) + residual) on NHWC x for an nn.BatchNorm2d `bn`.  batch_stats None follows bn.training; True: the batch statistics
    (running_mean / running_var updated in place, num_batches_tracked incremented); False: the running statistics (frozen)."""
    L.require_cuda(x, 'batch_norm_act x')
    if not isinstance(bn, torch.nn.BatchNorm2d):
        raise NotImplementedError('yolact_amd batch_norm_act: a %s is not supported (an nn.BatchNorm2d is)' % type(bn).__name__)
    if not bn.affine:
        raise NotImplementedError('yolact_amd batch_norm_act: affine = False is not supported')
    if not bn.track_running_stats:
        raise NotImplementedError('yolact_amd batch_norm_act: track_running_stats = False is not supported')
    if bn.momentum is None:
        raise NotImplementedError('yolact_amd batch_norm_act: momentum = None (a cumulative average) is not supported')
    stats = bool(bn.training if batch_stats is None else batch_stats)
    Cc = int(bn.num_features)
    if x.dim() < 2 or x.shape[-1] != Cc or Cc % 4 != 0:
        raise NotImplementedError('yolact_amd batch_norm_act: x %s for %d features is not supported ([..,C] with C %% 4 == 0 is)'
                                  % (tuple(x.shape), Cc))
    if residual is not None:
        L.require_cuda(residual, 'batch_norm_act residual')
        if residual.shape != x.shape:
            raise ValueError('batch_norm_act: residual %s for x %s' % (tuple(residual.shape), tuple(x.shape)))
    if stats and x.numel() // Cc < 2:
        raise NotImplementedError('yolact_amd batch_norm_act: batch statistics over npos = %d values per channel are not supported '
                                  '(more than one is; PyTorch refuses it too)' % (x.numel() // Cc))
    L.require_cuda(bn.weight, 'batch_norm_act bn.weight')
    for t in (bn.running_mean, bn.running_var):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != x.device:
            raise NotImplementedError('yolact_amd batch_norm_act: running statistics that are not contiguous fp32 on the device of x '
                                      'are not supported')
    y = BnAct.apply(stats, bool(relu), float(bn.eps), float(bn.momentum), bn.running_mean, bn.running_var, x, residual, bn.weight,
                    bn.bias)
    if stats:
        with torch.no_grad():
            bn.num_batches_tracked += 1
        for t in (bn.running_mean, bn.running_var):        # written by the kernel: tell autograd's version check, as an in-place op does
            torch.autograd.graph.increment_version(t)
    return y


def check_bottleneck(block, name='block'):
    """NotImplementedError naming what of a backbone block the kernels do not take."""
    from .. import modules as M
    if not isinstance(block, M.Bottleneck):
        raise NotImplementedError('yolact_amd bottleneck: %s is a %s, which is not supported (a Bottleneck is)' % (name, type(block).__name__))
    if block.use_dcn or not isinstance(block.conv2, torch.nn.Conv2d):
        raise NotImplementedError('yolact_amd bottleneck: %s is a DCN block (use_dcn = True), which is not supported yet' % name)
    convs = [('conv1', block.conv1, 1, 1), ('conv2', block.conv2, 3, block.stride), ('conv3', block.conv3, 1, 1)]
    if block.downsample is not None:
        convs.append(('downsample.0', block.downsample[0], 1, block.stride))
    for n, m, k, st in convs:
        if (tuple(m.kernel_size), tuple(m.stride), tuple(m.padding), tuple(m.dilation), m.groups, m.bias is None) != \
                ((k, k), (st, st), (k // 2, k // 2), (1, 1), 1, True):
            raise NotImplementedError('yolact_amd bottleneck: %s.%s = %r is not supported (a bias-free %d x %d / stride %d / padding %d '
                                      'is)' % (name, n, m, k, k, st, k // 2))
        check_plain(m.weight, st, 'bottleneck %s.%s' % (name, n))


def bottleneck(x, block, batch_stats=None):
    """backbone.py:37-57 on NHWC x: relu(bn1(conv1 x)), relu(bn2(conv2 .)), relu(bn3(conv3 .) + (downsample(x) or x))."""
    L.require_cuda(x, 'bottleneck x')
    check_bottleneck(block)
    out = batch_norm_act(conv2d_plain(x, block.conv1.weight), block.bn1, batch_stats, relu=True)
    out = batch_norm_act(conv2d_plain(out, block.conv2.weight, block.stride), block.bn2, batch_stats, relu=True)
    out = conv2d_plain(out, block.conv3.weight)
    res = x
    if block.downsample is not None:
        res = batch_norm_act(conv2d_plain(x, block.downsample[0].weight, block.stride), block.downsample[1], batch_stats)
    return batch_norm_act(out, block.bn3, batch_stats, residual=res, relu=True)
