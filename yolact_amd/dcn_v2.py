"""The reference's `dcn_v2` module surface (external/DCNv2/dcn_v2.py) on the HIP kernels.

    dcn_v2_conv(input, offset, mask, weight, bias, stride, padding, dilation, deformable_groups)     dcn_v2.py:16-52
    DCNv2(in_channels, out_channels, kernel_size, stride, padding, dilation=1, deformable_groups=1)  dcn_v2.py:55-96
    DCN(...)  = DCNv2 + conv_offset_mask, forward(input)                                             dcn_v2.py:97-128

Inside a `Yolact` plan these modules are parameter containers (the engine reads weight / bias / conv_offset_mask once and
emits `ymi_dcn_v2_forward_f32` ops, yolact_amd/engine.py).  Called on their own — the reference's own known-answer test does
that (external/DCNv2/test.py:32-67) — they run the same C-ABI entry points: NCHW fp32 in, NCHW fp32 out, like
`_ext.dcn_v2_forward` (src/vision.cpp:3-8, src/dcn_v2.h:9-39).  What YOLACT++ constructs is supported: 3x3, padding 1,
dilation 1, one deformable group (backbone.py:22-26).  PyTorch does the layout changes (NCHW <-> NHWC) and owns the memory; the
arithmetic of the deformable op is in the HIP library.

Differentiable: the deformable op itself.  When grad mode is on and one of input / offset / mask / weight / bias requires grad,
`dcn_v2_conv` is a `torch.autograd.Function` (the reference's `_DCNv2`, dcn_v2.py:16-52) whose backward is
`ymi_dcn_v2_backward_f32` (csrc/dcn_bwd.hip): gradients for all five tensors, once differentiable (no double backward), sums of
fp32 atomics (fp32-class accurate, not bit-reproducible from run to run).  The forward VALUE is the one the no-grad path
computes, bit for bit.  `DCN.forward` under grad mode is the reference's formulation (dcn_v2.py:118-128): conv_offset_mask, chunk
and sigmoid through PyTorch (whose autograd carries their gradients), then the deformable op.  Not differentiable: anything
inside an engine plan (there the modules are parameter containers), `Yolact` in training mode (it raises), CPU tensors (they
raise: there is no CPU path).
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable
from torch.nn.modules.utils import _pair

from . import _lib as L


def _ceil(a, b):
    return (a + b - 1) // b * b


from torch.utils.weak import WeakIdKeyDictionary

_pack_cache = WeakIdKeyDictionary()     # weight TENSOR OBJECT -> {(version, bias identity / version, shape, geometry, device): Packed}


def _packed(weight, bias, stride, pad, cin_pad, device):
    """engine.Packed of (weight, bias) (packing splits the filters on the host: worth caching for modules called in a loop).  Keyed
    on the weight tensor OBJECT (identity) through a weak dictionary — an entry dies with its tensor, so a recycled address can never hit a
    stale pack and no dead module's parameters stay pinned on the GPU (round-4 advisor: the key used to be data_ptr + _version) —
    plus its version counter (in-place edits), the bias object / version, the shapes, the geometry and the device, plus how many
    loss-guarded optimiser launches have written each of them (optim.guarded_writes: such a write bumps the version only once it is
    settled, which a forward must not wait for)."""
    from .engine import Packed
    from .optim import guarded_writes
    sub = _pack_cache.get(weight)
    if sub is None:
        sub = _pack_cache[weight] = {}
    key = (weight._version, tuple(weight.shape), None if bias is None else (id(bias), bias._version, tuple(bias.shape)),
           stride, pad, cin_pad, str(device), guarded_writes(weight), guarded_writes(bias))
    pk = sub.get(key)
    if pk is None:
        sub.clear()                            # one live pack per weight tensor: an older version's pack is garbage
        pk = sub[key] = Packed(weight, bias, None, stride, pad, cin_pad, device)
    return pk


def _nhwc_padded(x, cpad):
    xn = x.detach().to(torch.float32).permute(0, 2, 3, 1)
    if cpad != xn.shape[-1]:
        xn = torch.nn.functional.pad(xn, (0, cpad - xn.shape[-1]))
    return xn.contiguous()


def _fill_desc(d, xd, pk, y, Ho, Wo, amax, h2):
    B, H, W, Cx = xd.shape
    d.x, d.w = xd.data_ptr(), pk.w.data_ptr()
    d.scale = pk.scale.data_ptr() if pk.scale is not None else None
    d.bias = pk.bias.data_ptr() if pk.bias is not None else None
    d.B, d.H, d.W, d.Cin, d.ldx = B, H, W, pk.Cin, Cx
    d.Ho, d.Wo, d.Cout = Ho, Wo, pk.Cout
    d.kh, d.kw, d.stride, d.pad, d.Kpad = pk.kh, pk.kw, pk.stride, pk.pad, pk.Kpad
    d.cin_alg, d.cout_alg = pk.cin_alg, pk.cout_alg
    d.nseg = 1
    d.seg[0] = L.ConvSeg(0, pk.Cout, L.ACT_NONE, pk.Cout, Ho * Wo * pk.Cout, y.data_ptr())
    if h2:
        planes, sc2, winv = pk.h2()
        d.w_h2, d.scale_h2, d.winv_h2 = planes.data_ptr(), sc2.data_ptr(), winv.data_ptr()
        d.x_amax = amax.data_ptr()


def _input_bound(xd):
    """A magnitude-bound slot (ymi_conv_desc.x_amax) raised to max|x| by ymi_amax_f32."""
    from ._lib import AMAX_SLOT_FLOATS
    amax = torch.zeros(AMAX_SLOT_FLOATS, dtype=torch.float32, device=xd.device)
    L.check(L.lib().ymi_amax_f32(xd.data_ptr(), xd.numel(), amax.data_ptr(), L.stream_ptr()), 'ymi_amax_f32')
    return amax


def _check_geometry(weight, stride, padding, dilation, deformable_groups):
    st, pd, dl = _pair(stride), _pair(padding), _pair(dilation)
    if tuple(weight.shape[2:4]) != (3, 3) or pd != (1, 1) or dl != (1, 1) or deformable_groups != 1 or st[0] != st[1]:
        raise NotImplementedError('yolact_amd dcn_v2: only the 3x3 / padding 1 / dilation 1 / one-group DCN that YOLACT++ '
                                  'constructs (backbone.py:22-26); got kernel %s stride %s padding %s dilation %s groups %d'
                                  % (tuple(weight.shape[2:4]), st, pd, dl, deformable_groups))
    return st[0]


def _dcn_launch(xd, om, mask_is_prob, pk, Ho, Wo):
    """xd [B,H,W,Cin_pad] NHWC, om [B,Ho,Wo,ldo] NHWC (18 offsets | 9 mask channels) -> y [B,Ho,Wo,Cout] NHWC."""
    y = torch.empty(xd.shape[0], Ho, Wo, pk.Cout, dtype=torch.float32, device=xd.device)
    # the pipelined fp16x2 gather-GEMM (csrc/dcn.hip) where its epilogue applies (Cout % 4 == 0), else the general loader on the
    # exact-fp32 MFMA tiles; both are fp32-class (include/yolact_amd.h, YMI_TILE_H2)
    h2 = pk.Cout % 4 == 0
    amax = _input_bound(xd) if h2 else None
    dd = L.DcnDesc()
    _fill_desc(dd.conv, xd, pk, y, Ho, Wo, amax, h2)
    M = xd.shape[0] * Ho * Wo
    dd.conv.tile = (L.TILE_H2 | L.TILE_DCNP | (L.DCNP_64x128_W8 if M >= 16384 else L.DCNP_32x128)) if h2 else L.TILE_AUTO
    dd.offmask, dd.ldo, dd.mask_is_prob = om.data_ptr(), om.shape[3], 1 if mask_is_prob else 0
    L.check(L.lib().ymi_dcn_v2_forward_f32(C.byref(dd), L.stream_ptr()), 'ymi_dcn_v2_forward_f32')
    return y


def _weight_nhwc_padded(weight, cpad):
    """[Cout,Cin,3,3] -> fp32 [Cout,3,3,cpad] (the unpacked layout of ymi_dcn_bwd_desc.w)."""
    return _nhwc_padded(weight, cpad)


def _dcn_backward(input, offset, mask, weight, gy, st, needs):
    """ymi_dcn_v2_backward_f32 for NCHW / OIHW tensors; needs = (input, offset, mask, weight, bias) wanted.  Returns the five
    gradients (None where not wanted) in NCHW / OIHW fp32."""
    from .engine import out_size
    B, Cin, H, W = input.shape
    Cout = weight.shape[0]
    Ho, Wo = out_size(H, 3, st, 1), out_size(W, 3, st, 1)
    dev = input.device
    with torch.cuda.device(dev), torch.no_grad():
        cin_p = _ceil(Cin, 32)
        xd = _nhwc_padded(input, cin_p)
        om = torch.cat([offset, mask], 1).detach().to(torch.float32).permute(0, 2, 3, 1).contiguous()
        wd = _weight_nhwc_padded(weight, cin_p)
        gyd = gy.detach().to(torch.float32).permute(0, 2, 3, 1).contiguous()
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        gx = new(B, H, W, cin_p) if needs[0] else None
        go = new(B, Ho, Wo, 18) if needs[1] else None
        gm = new(B, Ho, Wo, 9) if needs[2] else None
        gw = new(Cout, 3, 3, cin_p) if needs[3] else None
        gb = new(Cout) if needs[4] else None
        d = L.DcnBwdDesc()
        d.x, d.offmask, d.w, d.gy = xd.data_ptr(), om.data_ptr(), wd.data_ptr(), gyd.data_ptr()
        for name, t in (('gx', gx), ('g_offset', go), ('g_mask', gm), ('gw', gw), ('gbias', gb)):
            setattr(d, name, None if t is None else t.data_ptr())
        d.B, d.H, d.W, d.Cin, d.ldx, d.Ho, d.Wo, d.Cout = B, H, W, cin_p, cin_p, Ho, Wo, Cout
        d.kh, d.kw, d.stride, d.pad, d.dilation, d.deformable_groups = 3, 3, st, 1, 1, 1
        d.ldo, d.mask_is_prob, d.om_layout = 27, 1, 0
        L.check(L.lib().ymi_dcn_v2_backward_f32(C.byref(d), L.stream_ptr()), 'ymi_dcn_v2_backward_f32')
        nchw = lambda t: None if t is None else t.permute(0, 3, 1, 2).contiguous()
        return (nchw(None if gx is None else gx[..., :Cin]), nchw(go), nchw(gm), nchw(None if gw is None else gw[..., :Cin]), gb)


class _DCNv2Function(torch.autograd.Function):
    """`_DCNv2` (dcn_v2.py:16-52).  `value`: None, or a callable that computes the forward value another (equivalent) way —
    DCN.forward passes its two-launch no-grad path, so that the module's output does not depend on grad mode."""

    @staticmethod
    def forward(ctx, input, offset, mask, weight, bias, stride, padding, dilation, deformable_groups, value=None):
        ctx.st = _check_geometry(weight, stride, padding, dilation, deformable_groups)
        ctx.save_for_backward(input, offset, mask, weight, bias)
        if value is not None:
            return value()
        return _dcn_forward(input, offset, mask, weight, bias, ctx.st)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        input, offset, mask, weight, bias = ctx.saved_tensors
        needs = tuple(ctx.needs_input_grad[:5])
        needs = needs[:4] + (needs[4] and bias is not None,)
        grads = _dcn_backward(input, offset, mask, weight, gy, ctx.st, needs)
        like = (input, offset, mask, weight, bias)
        grads = tuple(None if g is None else g.to(t.dtype) for g, t in zip(grads, like))
        return grads + (None, None, None, None, None)


def _dcn_forward(input, offset, mask, weight, bias, st):
    from .engine import out_size
    B, Cin, H, W = input.shape
    Ho, Wo = out_size(H, 3, st, 1), out_size(W, 3, st, 1)
    dev = input.device
    with torch.cuda.device(dev), torch.no_grad():
        cin_p = _ceil(Cin, 32)                    # zero channels x zero filters: the kernels take Cin % 32 == 0
        xd = _nhwc_padded(input, cin_p)
        om = torch.cat([offset, mask], 1).detach().to(torch.float32).permute(0, 2, 3, 1).contiguous()
        pk = _packed(weight, bias, st, 1, cin_p if cin_p != Cin else None, dev)
        y = _dcn_launch(xd, om, True, pk, Ho, Wo)
        return y.permute(0, 3, 1, 2).contiguous()


def _wants_grad(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def dcn_v2_conv(input, offset, mask, weight, bias, stride, padding, dilation, deformable_groups):
    """`_DCNv2.apply` (dcn_v2.py:16-52): input [B,Cin,H,W], offset [B,18,Ho,Wo] (channel 2k = dh_k, 2k+1 = dw_k),
    mask [B,9,Ho,Wo] = the modulation itself (callers pass torch.sigmoid(...), dcn_v2.py:122), weight [Cout,Cin,3,3], bias
    [Cout] -> [B,Cout,Ho,Wo].  Differentiable in all five tensors when grad mode is on and one of them requires grad (module
    docstring); otherwise — and for the forward value in either case — the launches below."""
    from .engine import out_size
    L.require_cuda(input, 'dcn_v2_conv input')
    st = _check_geometry(weight, stride, padding, dilation, deformable_groups)
    B, Cin, H, W = input.shape
    Ho, Wo = out_size(H, 3, st, 1), out_size(W, 3, st, 1)
    if tuple(offset.shape) != (B, 18, Ho, Wo) or tuple(mask.shape) != (B, 9, Ho, Wo) or weight.shape[1] != Cin:
        raise ValueError('dcn_v2_conv: offset %s / mask %s / weight %s do not fit input %s at stride %d'
                         % (tuple(offset.shape), tuple(mask.shape), tuple(weight.shape), tuple(input.shape), st))
    if _wants_grad(input, offset, mask, weight, bias):
        return _DCNv2Function.apply(input, offset, mask, weight, bias, stride, padding, dilation, deformable_groups)
    return _dcn_forward(input, offset, mask, weight, bias, st)


class DCNv2(nn.Module):
    """dcn_v2.py:55-96."""

    def __init__(self, in_channels, out_channels, kernel_size, stride, padding, dilation=1, deformable_groups=1):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride = _pair(kernel_size), _pair(stride)
        self.padding, self.dilation = _pair(padding), _pair(dilation)
        self.deformable_groups = deformable_groups
        if (self.kernel_size != (3, 3) or self.padding != (1, 1) or self.dilation != (1, 1) or deformable_groups != 1
                or self.stride[0] != self.stride[1]):            # (DCN.forward launches with stride[0]: an asymmetric pair must not pass)
            raise NotImplementedError('only the 3x3 / pad 1 / one-group / square-stride DCN that YOLACT++ constructs (backbone.py:22-26)')
        self.weight = nn.Parameter(torch.zeros(out_channels, in_channels, *self.kernel_size))
        self.bias = nn.Parameter(torch.zeros(out_channels))
        self.reset_parameters()

    def reset_parameters(self):
        n = self.in_channels * self.kernel_size[0] * self.kernel_size[1]
        with torch.no_grad():
            self.weight.uniform_(-1.0 / n ** 0.5, 1.0 / n ** 0.5)
            self.bias.zero_()

    def forward(self, input, offset, mask):
        k = self.deformable_groups * self.kernel_size[0] * self.kernel_size[1]
        assert 2 * k == offset.shape[1] and k == mask.shape[1]
        return dcn_v2_conv(input, offset, mask, self.weight, self.bias, self.stride, self.padding, self.dilation,
                           self.deformable_groups)


class DCN(DCNv2):
    """dcn_v2.py:97-128: DCNv2 + the 27-channel offset / mask convolution; forward(input)."""

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, padding=1, dilation=1, deformable_groups=1):
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, deformable_groups)
        self.conv_offset_mask = nn.Conv2d(in_channels, 27, 3, stride=self.stride, padding=1, bias=True)
        self.init_offset()

    def init_offset(self):
        with torch.no_grad():
            self.conv_offset_mask.weight.zero_()
            self.conv_offset_mask.bias.zero_()

    def forward(self, input):
        """out = conv_offset_mask(input); offset = out[:, :18]; mask = sigmoid(out[:, 18:]); dcn_v2_conv(...) — as two launches
        of the HIP library: the 27-channel 3x3 convolution, then the gather-GEMM reading its NHWC output directly (the sigmoid is
        applied in the kernel, as in the engine's plans).

        Under grad mode (the input or a parameter requires grad) the autograd graph is the reference's (dcn_v2.py:118-128):
        conv_offset_mask, chunk, cat and sigmoid are PyTorch operations, the deformable op is `_DCNv2Function`; the VALUE is still
        that of the two launches, so the module's output does not depend on grad mode.  (The gradient is therefore taken at
        PyTorch's offsets / modulation, which equal the library's to fp32 round-off.)"""
        L.require_cuda(input, 'DCN input')
        if _wants_grad(input, *self.parameters()):
            out = self.conv_offset_mask(input)
            o1, o2, mask = torch.chunk(out, 3, dim=1)
            offset = torch.cat((o1, o2), dim=1)
            mask = torch.sigmoid(mask)
            return _DCNv2Function.apply(input, offset, mask, self.weight, self.bias, self.stride, self.padding, self.dilation,
                                        self.deformable_groups, lambda: self._forward_two_launches(input))
        return self._forward_two_launches(input)

    def _forward_two_launches(self, input):
        from .engine import out_size
        st = self.stride[0]
        B, Cin, H, W = input.shape
        Ho, Wo = out_size(H, 3, st, 1), out_size(W, 3, st, 1)
        dev = input.device
        with torch.cuda.device(dev), torch.no_grad():
            cin_p = _ceil(Cin, 32)
            xd = _nhwc_padded(input, cin_p)
            cp = cin_p if cin_p != Cin else None
            pko = _packed(self.conv_offset_mask.weight, self.conv_offset_mask.bias, st, 1, cp, dev)
            om = torch.empty(B, Ho, Wo, 27, dtype=torch.float32, device=dev)
            d = L.ConvDesc()
            _fill_desc(d, xd, pko, om, Ho, Wo, None, False)
            L.check(L.lib().ymi_conv2d_nhwc_f32(C.byref(d), L.stream_ptr()), 'conv_offset_mask')
            pk = _packed(self.weight, self.bias, st, 1, cp, dev)
            y = _dcn_launch(xd, om, False, pk, Ho, Wo)
            return y.permute(0, 3, 1, 2).contiguous()
