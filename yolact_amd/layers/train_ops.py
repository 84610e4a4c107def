"""Differentiable building blocks of the train-mode heads, protonet, FPN, ResNet stages, ResNet stem and DarkNet backbone on the HIP
kernels (csrc/conv_train.hip, csrc/conv_wgrad_h2.hip, csrc/conv_dgrad.hip, csrc/bn_train.hip, csrc/stem_train.hip, csrc/darknet_train.hip and the conv engine).

    conv2d_act(x, weight, bias, padding, act)            -> y [B,H,W,Cout]: act(conv(x, weight) + bias), act in {None, 'relu', 'tanh'}
    conv2d_multi(x, [(weight, bias, act), ..], padding)  -> one y per entry: up to three convolutions of the SAME input as one launch
                                                            (the head's bbox / conf / mask layers, yolact.py:169-173)
    conv2d_down(x, weight, bias, act)                    -> [B,Ho,Wo,Cout]: the same at stride 2 with padding k // 2 (the FPN's
                                                            downsample layers, yolact.py:349-351)
    conv2d_plain(x, weight, stride)                      -> [B,Ho,Wo,Cout]: a bias-free convolution with padding k // 2 at stride 1 or 2
                                                            (the backbone's convolutions, backbone.py:19-31)
    upsample2x(x, relu)                                  -> [B,2H,2W,C]: F.interpolate(scale_factor=2, bilinear, align_corners=False)
    upsample_add(top, lat)                               -> F.interpolate(top, size of lat, bilinear, align_corners=False) + lat (the
                                                            FPN's top-down sum, yolact.py:332-334), any size of lat >= that of top
    batch_norm_act(x, bn, batch_stats, residual, relu)   -> relu(bn(x) + residual) for an nn.BatchNorm2d, batch statistics or frozen
    bottleneck(x, block, batch_stats)                    -> a modules.Bottleneck (backbone.py:37-57); bn3 + shortcut + ReLU are one launch
    deform_conv(x, om, weight, bias, stride)             -> [B,Ho,Wo,Cout]: a DCN's modulated deformable 3x3 (dcn_v2.py:16-52) from the raw
                                                            conv_offset_mask output om [B,Ho,Wo,27] (offsets, then mask logits)
    dcn_bottleneck(x, block, batch_stats)                -> a modules.Bottleneck whose conv2 is a DCN (use_dcn = True)
    stem_conv(x4, weight)                                -> [B,Ho,Wo,Cout]: the stem's 7x7 / stride 2 / padding 3 convolution of 3 channels
                                                            (backbone.py:77) on the image padded to 4 channels, x4 [B,H,W,4]
    max_pool_3x3_s2(x)                                   -> [B,Hp,Wp,C]: F.max_pool2d(x, 3, 2, 1) (backbone.py:80)
    batch_norm_leaky(x, bn, batch_stats, residual)       -> leaky_relu(bn(x), 0.1) + residual: the residual BEHIND the activation
    preconv(x4, weight)                                  -> [B,H,W,Cout]: DarkNet's 3x3 / stride 1 / padding 1 convolution of 3 channels
                                                            (backbone.py:268) on the image padded to 4 channels, x4 [B,H,W,4]
    dark_unit(x, seq, batch_stats, residual)             -> a DarkNet unit, Sequential(conv, BatchNorm2d, LeakyReLU(0.1)): conv2d_plain,
                                                            then batch_norm_leaky
    dark_block(x, block, batch_stats)                    -> a modules.DarkNetBlock (backbone.py:235-247): conv2(conv1(x)) + x
    wgrad_mode(mode) / set_wgrad_mode(mode)              the weight-gradient kernel of the four convolutions and deform_conv's GEMM: 'fp32'
                                                            (default) or 'fp16x2' (csrc/conv_wgrad_h2.hip); a context manager and a setter
    conv_mode(mode) / set_conv_mode(mode)                the tiles of the same convolutions' forward and data gradient: 'fp32' (default)
                                                            or 'fp16x2' (filters packed on the device by csrc/conv_pack_h2.hip, the
                                                            engine's fp16x2 tiles); a switch of its own, with get_conv_mode,
                                                            check_conv_mode and CONV_MODES beside it

x and the results are NHWC fp32 GPU tensors; weight and bias are nn.Conv2d parameters in torch layout.  Everything is once
differentiable in x, every weight and every bias.  Each call packs its filters from the CURRENT parameter values (a permute; no
cache), launches only what needs_input_grad asks for, and saves its inputs, so autograd's version check refuses a backward after an
in-place edit.  CPU tensors raise: there is no CPU path.

The four convolutions are one autograd.Function, Conv, behind four validators (_check_geometry, whose faces are check_conv, check_down
and check_plain): 3x3 / pad 1 and 1x1 / pad 0, stride 1 or 2, dilation 1, groups 1, Cin % 32 == 0, any Cout.  Forward: one
ymi_conv2d_nhwc_f32 launch over all outputs.  Backward:
  g    with a bias: ymi_act_bwd_f32 per output (g = dy * act'(y), act None too), side by side in one buffer whose channel stride ldg
       is ceil32 of the summed widths, padding zeroed by the last output's launch.  Without one (conv2d_plain): dy itself, F.pad-ed
       to ldg only when Cout % 32 != 0, and no activation launch.
  dw   _weight_grad: the wgrad mode's entry once over all outputs (dw, and db when there is a bias), then _unpack_dw per output.
  dx   _data_grad.  Stride 1: ymi_conv2d_nhwc_f32 on g with the filters flipped in both taps and transposed in (Cin, Cout).
       Stride 2 has two routes.  conv2d_plain: ymi_conv_dgrad_s2_nhwc_f32 (csrc/conv_dgrad.hip: only the taps that exist).
       conv2d_down (zero_insert = True): g spread over a zeroed [B,H,W,ldg] buffer (gz[:, ::2, ::2] = g), then the stride-1 launch,
       four times the useful FLOPs.  The two routes agree bit for bit only on exact grids.  The FPN keeps its own because it is the
       faster one there: at 3x3 256 -> 256, B = 8, 18 x 18 and 9 x 9 the kernel's grid is 48 and 16 blocks for 256 CUs, and
       forward_fpn forward + backward measured 4712 us with the kernel against 4637 us with this route, the parent's own spread
       being 62 us (profiles/train_net_ab.txt).
Both modes are read by the forward and kept on ctx; set_wgrad_mode and set_conv_mode say what follows them and what does not.
BatchNorm with none, ReLU or LeakyReLU(0.1) is one autograd.Function, Bn (csrc/bn_train.hip); the stem's and DarkNet's convolution of
the image are one, ImageConv, driven by a spec (STEM, PRE); the plain and the DCN bottleneck are one body, _bottleneck.
"""
from __future__ import annotations

import collections
import contextlib
import ctypes as C
import threading

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from .. import _lib as L
from . import _loss_common as LC

ACTS = {None: L.ACT_NONE, 'none': L.ACT_NONE, 'relu': L.ACT_RELU, 'tanh': L.ACT_TANH}


def _ceil(a, b):
    return (a + b - 1) // b * b


def _out_size(H, W, k, pad, stride):
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def _pair(v):
    return (int(v), int(v)) if isinstance(v, int) else tuple(int(e) for e in v)


def _check_geometry(who, weight, stride, padding=None, dilation=1, groups=1, strides=(1, 2)):
    """NotImplementedError naming what of a convolution's geometry the kernels do not take -> (k, pad, stride).  `strides`: what the
    caller takes.  padding None: k // 2 is meant, and a weight that is not 4-D is refused by name (with a padding the weight is an
    nn.Conv2d's, and its shape is unpacked before anything is looked at)."""
    if isinstance(padding, str):
        raise NotImplementedError('yolact_amd %s: padding = %r is not supported (an integer padding is)' % (who, padding))
    stride, dilation = _pair(stride), _pair(dilation)
    if padding is not None:
        padding, (Cout, Cin, kh, kw) = _pair(padding), weight.shape
    if stride not in [(s, s) for s in strides]:
        raise NotImplementedError('yolact_amd %s: stride = %r is not supported (%s %s)'
                                  % (who, stride, ' and '.join('stride %d' % s for s in strides), 'is' if len(strides) == 1 else 'are'))
    if padding is None:
        if weight.dim() != 4:
            raise NotImplementedError('yolact_amd %s: a weight of shape %s is not supported ([Cout,Cin,k,k] is)' % (who, tuple(weight.shape)))
        Cout, Cin, kh, kw = weight.shape
        padding = (kh // 2, kh // 2)
    if dilation != (1, 1):
        raise NotImplementedError('yolact_amd %s: dilation = %r is not supported (dilation 1 is)' % (who, dilation))
    if groups != 1:
        raise NotImplementedError('yolact_amd %s: groups = %r is not supported (groups 1 is)' % (who, groups))
    if (kh, kw, padding) not in ((3, 3, (1, 1)), (1, 1, (0, 0))):
        what = 'at stride 2' if stride == (2, 2) else 'with padding = %r' % (padding,)
        raise NotImplementedError('yolact_amd %s: a %d x %d kernel %s is not supported (3 x 3 / padding 1 and 1 x 1 / padding 0 are)'
                                  % (who, kh, kw, what))
    if Cin % 32 != 0:
        raise NotImplementedError('yolact_amd %s: Cin = %d is not supported (a multiple of 32 input channels is)' % (who, Cin))
    return kh, padding[0], stride[0]


def check_conv(weight, padding, stride=1, dilation=1, groups=1, who='conv2d_act'):
    """The geometry of a stride-1 convolution with its padding given -> (k, pad)."""
    return _check_geometry(who, weight, stride, padding, dilation, groups, strides=(1,))[:2]


def check_down(weight, who='conv2d_down'):
    """The geometry of a stride-2 convolution with padding k // 2 -> (k, pad)."""
    return _check_geometry(who, weight, 2)[:2]


def check_plain(weight, stride, who='conv2d_plain'):
    """The geometry of a bias-free convolution with padding k // 2 at stride 1 or 2 -> (k, pad, stride)."""
    return _check_geometry(who, weight, stride)


def _engine_conv(x, ldx, wpk, bias, Cin, Cout, k, pad, segs, stride=1, h2=None):
    """One ymi_conv2d_nhwc_f32 launch on the exact-fp32 tiles: x [B,H,W,ldx], wpk [CoutPad][Kpad], Kpad = k*k*Cin or, for the Cin-4
    loader, its ceil32; segs = (n0, n1, act, tensor).  h2 = (planes [2][CoutPad][Kpad], winv [CoutPad]) of _pack_h2: the same launch on
    the fp16x2 tile _h2_tile picks, with the magnitude bound of x from one ymi_amax_f32 launch; wpk is then never read and may be
    the planes themselves (the fp16x2 kernels take their filters from w_h2; the entry's validation wants w non-null and aligned)."""
    B, H, W = x.shape[:3]
    Ho, Wo = _out_size(H, W, k, pad, stride)
    d = L.ConvDesc()
    d.x, d.w, d.bias = x.data_ptr(), wpk.data_ptr(), (None if bias is None else bias.data_ptr())
    d.B, d.H, d.W, d.Cin, d.ldx, d.Ho, d.Wo, d.Cout = B, H, W, Cin, ldx, Ho, Wo, Cout
    d.kh, d.kw, d.stride, d.pad, d.Kpad, d.tile = k, k, stride, pad, int(wpk.shape[-1]), L.TILE_AUTO
    d.nseg = len(segs)
    for i, (n0, n1, act, y) in enumerate(segs):
        d.seg[i] = L.ConvSeg(n0, n1, act, n1 - n0, Ho * Wo * (n1 - n0), y.data_ptr())
    if h2 is not None:
        planes, winv = h2
        # no BatchNorm is folded into a training convolution: the epilogue's scale is the inverse filter scale itself
        d.w_h2, d.scale_h2, d.winv_h2 = planes.data_ptr(), winv.data_ptr(), winv.data_ptr()
        amax = _amax_slot(x.device)
        L.check(L.lib().ymi_amax_f32(x.data_ptr(), x.numel(), amax.data_ptr(), L.stream_ptr()), 'ymi_amax_f32')
        d.x_amax = amax.data_ptr()
        d.tile = _h2_tile(d)
    L.check(L.lib().ymi_conv2d_nhwc_f32(C.byref(d), L.stream_ptr()), 'ymi_conv2d_nhwc_f32')


_slots = threading.local()                               # .pool: (device, stream, chunk, slots handed out) of this thread
_SLOTS_PER_CHUNK = 256


def _amax_slot(dev):
    """A zeroed magnitude-bound slot (ymi_conv_desc.x_amax).  Slots are cut from a chunk of 256 that one memset zeroes, and no slot
    is handed out twice, so a launch costs no fill of its own; a chunk belongs to one thread, device and stream, and its memory goes
    back to the allocator, in stream order, when its last slot's launch has been enqueued."""
    stream = torch.cuda.current_stream(dev).cuda_stream
    pool = getattr(_slots, 'pool', None)
    if pool is None or pool[0] != (dev, stream) or pool[2] == _SLOTS_PER_CHUNK:
        pool = _slots.pool = [(dev, stream), torch.zeros(_SLOTS_PER_CHUNK, L.AMAX_SLOT_FLOATS, dtype=torch.float32, device=dev), 0]
    pool[2] += 1
    return pool[1][pool[2] - 1]


def _h2_pays(k):
    """Whether a convolution runs on the fp16x2 tiles under conv_mode('fp16x2'): the 3 x 3 ones do, the 1 x 1 ones stay on the
    exact-fp32 tiles.  A static class rule from profiles/conv_h2_train_probe_b8.txt: every 3 x 3 class of a step gains or stays within
    the spread of the class, while the pointwise ones are bound by the traffic of x and y, to which the mode adds the pass for the bound
    of x: of eighteen measured calls five are slower by more than the spread, the ten faster ones gain through the cheaper packing
    rather than the tile, and the class's sum, 1647 against 1680 us, lies inside its summed spread of 43 us."""
    return k == 3


def _h2_tile(d):
    """The fp16x2 tile of a described convolution: a static rule, no tune table, nothing measured at run time.  Where the pipelined
    kernel of csrc/dcn.hip takes the descriptor (run_pipe: one dense output, Cout % 4 == 0, no activation or ReLU; its fourth
    condition, two chunks of 32 along K, holds for every 3 x 3) and the output fills its 128 columns (Cout >= 128: at 64 the
    engine's 64x64 measured 100 us against 125) its tile, 64x128 on eight waves from M = 16384 rows and 32x128 below, as
    dcn_v2._dcn_launch chooses; otherwise the engine's own choice (ymi_conv_pick_tile) as its fp16x2 variant, 128x32, which has
    none, becoming 64x32 split in K."""
    M = d.B * d.Ho * d.Wo
    g0 = d.seg[0]
    if (d.nseg == 1 and g0.n0 == 0 and g0.n1 == d.Cout and d.Cout % 4 == 0 and d.Cout >= 128 and g0.act in (L.ACT_NONE, L.ACT_RELU)
            and d.Kpad // 32 >= 2 and M * d.Cout < 1 << 31):
        return L.TILE_H2 | L.TILE_DCNP | (L.DCNP_64x128_W8 if M >= 16384 else L.DCNP_32x128)
    tile = L.lib().ymi_conv_pick_tile(C.byref(d))
    if tile < 0:
        L.check(tile, 'ymi_conv_pick_tile')
    return (L.TILE_64x32_K2 if tile == L.TILE_128x32 else tile) | L.TILE_H2


def _pack_h2(ws, Cin, k, mode, ld=0):
    """One ymi_conv_pack_h2_f32 launch over the parameters ws (their CURRENT values, read in place: no permute, no concatenation)
    -> (planes int16 [2][RowsPad][Kp], winv fp32 [RowsPad]).  mode 0: the layout of _pack_forward; mode 1: that of _pack_dgrad(., ld)."""
    dev = ws[0].device
    ws = [LC.f32(w, dev) for w in ws]                       # (fp32 contiguous parameters: themselves, no copy)
    couts = [int(w.shape[0]) for w in ws]
    rows_pad = _ceil(sum(couts) if mode == 0 else Cin, 128)
    Kp = k * k * (Cin if mode == 0 else ld)
    planes = torch.empty(2, rows_pad, Kp, dtype=torch.int16, device=dev)
    winv = torch.empty(rows_pad, dtype=torch.float32, device=dev)
    d = L.ConvPackDesc()
    for i, w in enumerate(ws):
        d.w[i], d.cout[i] = w.data_ptr(), couts[i]
    d.planes, d.winv, d.w32 = planes.data_ptr(), winv.data_ptr(), None
    d.n, d.Cin, d.k, d.mode, d.ld = len(ws), Cin, k, mode, ld
    L.check(L.lib().ymi_conv_pack_h2_f32(C.byref(d), L.stream_ptr()), 'ymi_conv_pack_h2_f32')
    return planes, winv


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


def _pack_dgrad_s2(w, cpad):
    """The filters of ymi_conv_dgrad_s2_nhwc_f32: [Cout,Cin,k,k] -> [k][k][cpad/4][Cin][4], Cout padded to cpad with zeros."""
    Cout, Cin, k, _ = w.shape
    t = F.pad(w.permute(2, 3, 0, 1), (0, 0, 0, cpad - Cout))                    # [k,k,cpad,Cin]
    return t.reshape(k, k, cpad // 4, 4, Cin).permute(0, 1, 2, 4, 3).contiguous()


def _cat_f32(ts):
    """The CURRENT values of the parameters ts in fp32, along dim 0."""
    ts = [t.detach().float() for t in ts]
    return ts[0] if len(ts) == 1 else torch.cat(ts, 0)


def _engine_filters(ws, k, mode, ldg=None):
    """The filters of an engine launch from the parameters ws, each [co,Cin,k,k] -> (wpk, h2) as _engine_conv takes them.  ldg None:
    the forward layout (_pack_forward); an ldg: the data gradient's (_pack_dgrad(., ldg)).  mode 'fp16x2' where _h2_pays: the planes
    of _pack_h2 with their inverse scales, the planes standing in for wpk; otherwise the packed fp32 filters and h2 = None."""
    if mode == 'fp16x2' and _h2_pays(k):
        h2 = _pack_h2(ws, int(ws[0].shape[1]), k, 0) if ldg is None else _pack_h2(ws, int(ws[0].shape[1]), k, 1, ldg)
        return h2[0], h2
    wcat = _cat_f32(ws)
    return (_pack_forward(wcat) if ldg is None else _pack_dgrad(wcat, ldg)), None


WGRAD_MODES = {'fp32': ('ymi_conv_wgrad_nhwc_f32', 'CONV_WGRAD'), 'fp16x2': ('ymi_conv_wgrad_nhwc_h2', 'CONV_WGRAD_H2')}
CONV_MODES = ('fp32', 'fp16x2')
_wgrad = threading.local()                               # .mode: this thread's weight-gradient mode, 'fp32' where never set
_conv = threading.local()                                # .mode: this thread's forward / data-gradient mode, 'fp32' where never set


def _check_mode(word, modes, mode):
    if mode not in modes:
        raise ValueError("%s mode %r: 'fp32' and 'fp16x2' are the modes" % (word, mode))
    return mode


def _set_mode(local, word, modes, mode):
    old = getattr(local, 'mode', 'fp32')
    local.mode = _check_mode(word, modes, mode)
    return old


@contextlib.contextmanager
def _mode_scope(local, word, modes, mode):
    old = _set_mode(local, word, modes, mode)
    try:
        yield
    finally:
        local.mode = old


def check_wgrad_mode(mode):
    return _check_mode('wgrad', WGRAD_MODES, mode)


def get_wgrad_mode():
    """The calling thread's weight-gradient mode."""
    return getattr(_wgrad, 'mode', 'fp32')


def set_wgrad_mode(mode):
    """The weight-gradient kernel of every Conv whose FORWARD runs on this thread from now on -> the mode it replaces.  'fp32':
    ymi_conv_wgrad_nhwc_f32, the default, whose bits the goldens pin.  'fp16x2': ymi_conv_wgrad_nhwc_h2 (csrc/conv_wgrad_h2.hip), the
    same sums on the fp16 matrix pipe with both operands split in two fp16 planes: other bits, equal on every run, within the fp32
    bar of fp64.  The forward, dx, the stem, the pre-convolution and the mask-IoU net do not read the mode."""
    return _set_mode(_wgrad, 'wgrad', WGRAD_MODES, mode)


def wgrad_mode(mode):
    """with wgrad_mode('fp16x2'): the forwards inside record the mode; their backward uses it wherever and whenever it runs."""
    return _mode_scope(_wgrad, 'wgrad', WGRAD_MODES, mode)


def check_conv_mode(mode):
    return _check_mode('conv', CONV_MODES, mode)


def get_conv_mode():
    """The calling thread's forward / data-gradient mode."""
    return getattr(_conv, 'mode', 'fp32')


def set_conv_mode(mode):
    """The tiles of the forward and of the data gradient of every Conv whose FORWARD runs on this thread from now on -> the mode it
    replaces; a switch of its own beside set_wgrad_mode.  'fp32': the exact-fp32 tiles, the default, whose bits the goldens pin.
    'fp16x2': where _h2_pays says so (the 3 x 3 convolutions) the filters are packed on the device as two fp16 planes under one
    power-of-two scale per row (ymi_conv_pack_h2_f32), the input's magnitude bound comes from a ymi_amax_f32 launch, and the same
    ymi_conv2d_nhwc_f32 runs on the fp16x2 tile _h2_tile picks: other bits, equal on every run, within the fp32 bar of fp64.  The
    1 x 1 convolutions, deform_conv's GEMM among them, keep the fp32 tiles and their bits.  The forward, the stride-1 dx and
    conv2d_down's zero-insert dx follow the mode; ymi_conv_dgrad_s2_nhwc_f32 (conv2d_plain's stride-2 dx), dw, db, the stem, the
    pre-convolution, the BatchNorm kernels and the mask-IoU net do not read it."""
    return _set_mode(_conv, 'conv', CONV_MODES, mode)


def conv_mode(mode):
    """with conv_mode('fp16x2'): the forwards inside run on the fp16x2 tiles and record the mode; their dx uses it wherever and
    whenever the backward runs."""
    return _mode_scope(_conv, 'conv', CONV_MODES, mode)


def _weight_grad(xd, g, ldg, Cin, ctot, k, pad, stride, want_w, want_b, mode='fp32'):
    """One launch of the mode's weight-gradient entry on xd [B,H,W,Cin] and g [B,Ho,Wo,ldg] -> (dw_flat [k*k*Cin, ctot], db [ctot]),
    None where not wanted."""
    dev = xd.device
    B, H, W = xd.shape[:3]
    dw = torch.empty(k * k * Cin, ctot, dtype=torch.float32, device=dev) if want_w else None
    db = torch.empty(ctot, dtype=torch.float32, device=dev) if want_b else None
    d = L.ConvWgradDesc()
    d.x, d.g = xd.data_ptr(), g.data_ptr()
    d.dw, d.db = (None if t is None else t.data_ptr() for t in (dw, db))
    d.B, d.H, d.W, d.Cin, d.Cout, d.ldg, d.kh, d.kw, d.pad, d.stride = B, H, W, Cin, ctot, ldg, k, k, pad, stride
    entry, kind = WGRAD_MODES[mode]
    ws = LC.workspace(kind, d, dev)
    d.ws_bytes = ws.numel()
    L.check(getattr(L.lib(), entry)(C.byref(d), L.stream_ptr()), entry)
    return dw, db


def _unpack_dw(dw_flat, k, Cin):
    """Columns [k*k*Cin, co] of the weight gradient -> [co,Cin,k,k]."""
    return dw_flat.reshape(k, k, Cin, dw_flat.shape[1]).permute(3, 2, 0, 1).contiguous()


def _data_grad(g, ldg, ws, B, H, W, k, pad, stride, zero_insert, mode='fp32'):
    """dx [B,H,W,Cin] from g [B,Ho,Wo,ldg] and the parameters ws, each [co,Cin,k,k] (the module docstring has the routes).  mode
    'fp16x2': the stride-1 launch (the zero-insert route's too) on the fp16x2 tiles, its filters from _pack_h2."""
    dev, Cin = g.device, int(ws[0].shape[1])
    if stride == 2 and zero_insert:
        # g with zeros between its pixels, exactly H x W (even and odd sizes), then the stride-1 data gradient: the added zeros
        # change no bit of a sum, and a pixel no window reads (1x1) gets an exact +0.0
        gz = torch.zeros(B, H, W, ldg, dtype=torch.float32, device=dev)
        gz[:, ::2, ::2] = g
        g, stride = gz, 1
    dx = torch.empty(B, H, W, Cin, dtype=torch.float32, device=dev)
    if stride == 1:
        wpk, h2 = _engine_filters(ws, k, mode, ldg)
        _engine_conv(g, ldg, wpk, None, ldg, Cin, k, k - 1 - pad, [(0, Cin, L.ACT_NONE, dx)], h2=h2)
    else:
        wpk = _pack_dgrad_s2(_cat_f32(ws), ldg)
        d = L.ConvDgradDesc()
        d.g, d.w, d.dx = g.data_ptr(), wpk.data_ptr(), dx.data_ptr()
        d.B, d.H, d.W, d.Cin, d.Cout, d.ldg, d.kh, d.kw, d.pad, d.stride = B, H, W, Cin, ldg, ldg, k, k, pad, 2
        L.check(L.lib().ymi_conv_dgrad_s2_nhwc_f32(C.byref(d), L.stream_ptr()), 'ymi_conv_dgrad_s2_nhwc_f32')
    return dx


class Conv(torch.autograd.Function):
    """apply(k, pad, stride, acts, zero_insert, x [B,H,W,Cin], w1, b1, .., wn, bn) -> (y1, .., yn), each [B,Ho,Wo,Cout_i].  Every b
    is a tensor, or every b is None (then there is one output and no activation).  zero_insert: the route of a stride-2 dx."""

    @staticmethod
    def forward(ctx, k, pad, stride, acts, zero_insert, x, *params):
        dev = x.device
        ws, bs = params[0::2], params[1::2]
        biased = bs[0] is not None
        couts = [int(w.shape[0]) for w in ws]
        Cin = int(ws[0].shape[1])
        with torch.cuda.device(dev), torch.no_grad():
            xd = LC.f32(x, dev)
            B, H, W, _ = xd.shape
            Ho, Wo = _out_size(H, W, k, pad, stride)
            ys, segs, n0 = [], [], 0
            for co, a in zip(couts, acts):
                y = torch.empty(B, Ho, Wo, co, dtype=torch.float32, device=dev)
                ys.append(y)
                segs.append((n0, n0 + co, a, y))
                n0 += co
            mode = get_conv_mode()
            bias = _cat_f32(bs).contiguous() if biased else None
            wpk, h2 = _engine_filters(ws, k, mode)
            _engine_conv(xd, Cin, wpk, bias, Cin, n0, k, pad, segs, stride=stride, h2=h2)
        # the inputs are saved so that autograd's version check refuses a backward after x or a parameter was edited in place; the
        # outputs (this call's own tensors) are what an activation's backward reads
        ctx.save_for_backward(x, *((*params, *ys) if biased else ws))
        ctx.geo, ctx.acts, ctx.couts, ctx.biased, ctx.zero_insert = (k, pad, stride), acts, couts, biased, zero_insert
        ctx.dtypes = [x.dtype] + [None if p is None else p.dtype for p in params]
        # autograd runs a CUDA backward on a thread of its own, where the thread-local mode is the default: the forward's is kept
        ctx.wgrad, ctx.conv = get_wgrad_mode(), mode
        return tuple(ys)

    @staticmethod
    @once_differentiable
    def backward(ctx, *dys):
        need = ctx.needs_input_grad[5:]
        saved = ctx.saved_tensors                         # (the version check)
        if not any(need):
            return (None,) * (5 + len(need))
        (k, pad, stride), couts, n = ctx.geo, ctx.couts, len(ctx.couts)
        x, ws, ys = (saved[0], saved[1:1 + 2 * n:2], saved[1 + 2 * n:]) if ctx.biased else (saved[0], saved[1:], ())
        want_x, want_p = need[0], need[1:]
        dev = x.device
        with torch.cuda.device(dev), torch.no_grad():
            xd = LC.f32(x, dev)
            B, H, W, Cin = xd.shape
            Ho, Wo = _out_size(H, W, k, pad, stride)
            ctot = sum(couts)
            ldg = _ceil(ctot, 32)
            if ctx.biased:
                g = torch.empty(B, Ho, Wo, ldg, dtype=torch.float32, device=dev)
                n0, keep = 0, []
                for i, (co, a, y, dy) in enumerate(zip(couts, ctx.acts, ys, dys)):
                    dyd = torch.zeros_like(y) if dy is None else LC.f32(dy, dev)
                    keep.append(dyd)
                    cpad = co + (ldg - ctot if i == n - 1 else 0)
                    L.check(L.lib().ymi_act_bwd_f32(y.data_ptr(), dyd.data_ptr(), g.data_ptr() + 4 * n0, B * Ho * Wo, co, cpad, co, co,
                                                    ldg, a, L.stream_ptr()), 'ymi_act_bwd_f32')
                    n0 += co
            else:
                g = LC.f32(dys[0], dev)
                if ldg != ctot:                            # (no backbone layer: their widths are multiples of 32)
                    g = F.pad(g, (0, ldg - ctot))
            grads = [None] * len(want_p)
            want_w, want_b = any(want_p[0::2]), any(want_p[1::2])
            if want_w or want_b:
                dw, db = _weight_grad(xd, g, ldg, Cin, ctot, k, pad, stride, want_w, want_b, ctx.wgrad)
                n0 = 0
                for i, co in enumerate(couts):
                    if want_p[2 * i]:
                        grads[2 * i] = _unpack_dw(dw[:, n0:n0 + co], k, Cin)
                    if want_p[2 * i + 1]:
                        grads[2 * i + 1] = db if n == 1 else db[n0:n0 + co].clone()
                    n0 += co
            dx = _data_grad(g, ldg, ws, B, H, W, k, pad, stride, ctx.zero_insert, ctx.conv) if want_x else None
        out = [dx] + grads
        return (None,) * 5 + tuple(None if t is None else t.to(dt) for t, dt in zip(out, ctx.dtypes))


def _check_act_bias(who, act, bias):
    if act not in ACTS:
        raise NotImplementedError('yolact_amd %s: act = %r is not supported (None, \'relu\' and \'tanh\' are)' % (who, act))
    if bias is None:
        raise NotImplementedError('yolact_amd %s: bias = None is not supported (a biased convolution is)' % who)


def _check_x(who, x, weight):
    if x.dim() != 4 or x.shape[3] != weight.shape[1]:
        raise ValueError('%s: x %s for a weight %s ([B,H,W,Cin] is expected)' % (who, tuple(x.shape), tuple(weight.shape)))


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
        _check_act_bias('conv2d_act', act, b)
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
    return Conv.apply(geo[0], geo[1], 1, tuple(acts), False, x, *params)


def conv2d_act(x, weight, bias, padding, act=None, stride=1, dilation=1, groups=1):
    """act(conv2d(x, weight, bias, padding)) on NHWC x -> NHWC."""
    return conv2d_multi(x, [(weight, bias, act)], padding, stride, dilation, groups)[0]


def conv2d_down(x, weight, bias, act=None):
    """act(conv2d(x, weight, bias, stride=2, padding=k // 2)) on NHWC x -> NHWC: 3 x 3 / pad 1 and 1 x 1 / pad 0, Cin % 32 == 0."""
    L.require_cuda(x, 'conv2d_down x')
    L.require_cuda(weight, 'conv2d_down weight')
    _check_act_bias('conv2d_down', act, bias)
    k, pad = check_down(weight)
    _check_x('conv2d_down', x, weight)
    if bias.numel() != weight.shape[0]:
        raise ValueError('conv2d_down: weight %s / bias %s' % (tuple(weight.shape), tuple(bias.shape)))
    return Conv.apply(k, pad, 2, (ACTS[act],), True, x, weight, bias)[0]


def conv2d_plain(x, weight, stride=1):
    """conv2d(x, weight, None, stride, padding=k // 2) on NHWC x -> NHWC: 3 x 3 / pad 1 and 1 x 1 / pad 0, stride 1 or 2, Cin % 32 == 0."""
    L.require_cuda(x, 'conv2d_plain x')
    L.require_cuda(weight, 'conv2d_plain weight')
    k, pad, st = check_plain(weight, stride)
    _check_x('conv2d_plain', x, weight)
    return Conv.apply(k, pad, st, (L.ACT_NONE,), False, x, weight, None)[0]


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


LEAKY_SLOPE = 0.1


class Bn(torch.autograd.Function):
    """apply(act, stats, eps, momentum, running_mean, running_var, x [..,C], residual or None, gamma, beta) -> y.  act None or 'relu':
    act(bn(x) + residual) (ymi_bn_fwd_nhwc_f32 / ymi_bn_bwd_nhwc_f32); 'leaky': leaky_relu(bn(x), 0.1) + residual, the residual BEHIND
    the activation (ymi_bn_leaky_fwd_nhwc_f32 / ymi_bn_leaky_bwd_nhwc_f32).  stats: batch statistics (the running ones are updated in
    place) or the running ones as they are.  The leaky slope decision z > 0 is the forward's: without a residual the backward reads
    it from y, with one from the bit mask the forward wrote (1/32 of the map, saved beside the residual)."""

    @staticmethod
    def forward(ctx, act, stats, eps, momentum, rmean, rvar, x, residual, gamma, beta):
        dev = x.device
        leaky, relu = act == 'leaky', int(act == 'relu')
        with torch.cuda.device(dev), torch.no_grad():
            xd = LC.f32(x, dev)
            Cc = xd.shape[-1]
            npos = xd.numel() // Cc
            y = torch.empty_like(xd)
            mean = torch.empty(Cc, dtype=torch.float32, device=dev)
            invstd = torch.empty(Cc, dtype=torch.float32, device=dev)
            rd = None if residual is None else LC.f32(residual, dev)
            mask = torch.empty((xd.numel() + 31) // 32, dtype=torch.int32, device=dev) if leaky and residual is not None else None
            gd, bd = LC.f32(gamma, dev), LC.f32(beta, dev)
            d = L.BnDesc()
            d.x, d.res, d.gamma, d.beta = xd.data_ptr(), (None if rd is None else rd.data_ptr()), gd.data_ptr(), bd.data_ptr()
            d.running_mean, d.running_var = rmean.data_ptr(), rvar.data_ptr()
            d.y, d.mean, d.invstd = y.data_ptr(), mean.data_ptr(), invstd.data_ptr()
            d.npos, d.C, d.training, d.relu, d.eps, d.momentum = npos, Cc, int(stats), relu, eps, momentum
            ws = LC.workspace('BN', d, dev)
            d.ws_bytes = ws.numel()
            _bn_launch('ymi_bn_leaky_fwd_nhwc_f32' if leaky else 'ymi_bn_fwd_nhwc_f32', leaky, d, mask)
        # the inputs are saved too: autograd's version check refuses a backward after x or a parameter was edited in place
        ctx.save_for_backward(x, gamma, beta, y, mean, invstd, *(t for t in (residual, mask) if t is not None))
        ctx.stats, ctx.leaky, ctx.relu, ctx.eps = int(stats), leaky, relu, eps
        ctx.dtypes = [x.dtype, None if residual is None else residual.dtype, gamma.dtype, beta.dtype]
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        want_x, want_r, want_g, want_b = ctx.needs_input_grad[6:]
        x, gamma, beta, y, mean, invstd = ctx.saved_tensors[:6]      # (the version check)
        mask = ctx.saved_tensors[7] if len(ctx.saved_tensors) > 7 else None
        if not (want_x or want_r or want_g or want_b):
            return (None,) * 10
        dev = x.device
        with torch.cuda.device(dev), torch.no_grad():
            xd, dyd, gd = LC.f32(x, dev), LC.f32(dy, dev), LC.f32(gamma, dev)
            Cc = xd.shape[-1]
            dx = torch.empty_like(xd) if want_x else None
            # d_res is a kernel output only under a ReLU; otherwise it is dy itself
            dres = torch.empty_like(xd) if (want_r and ctx.relu) else None
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
                _bn_launch('ymi_bn_leaky_bwd_nhwc_f32' if ctx.leaky else 'ymi_bn_bwd_nhwc_f32', ctx.leaky, d, mask)
            if want_r and not ctx.relu:
                dres = dyd
        out = [dx, dres, dg, db]
        return (None,) * 6 + tuple(None if (t is None or dt is None) else t.to(dt) for t, dt in zip(out, ctx.dtypes))


def _bn_launch(entry, leaky, d, mask):
    """A BatchNorm entry on its descriptor; the leaky ones take the bit mask (or null) behind it."""
    args = (C.byref(d), None if mask is None else mask.data_ptr(), L.stream_ptr()) if leaky else (C.byref(d), L.stream_ptr())
    L.check(getattr(L.lib(), entry)(*args), entry)


def _check_bn(who, x, bn, batch_stats, residual):
    """What batch_norm_act and batch_norm_leaky refuse, named -> whether the batch statistics are used."""
    L.require_cuda(x, who + ' x')
    if not isinstance(bn, torch.nn.BatchNorm2d):
        raise NotImplementedError('yolact_amd %s: a %s is not supported (an nn.BatchNorm2d is)' % (who, type(bn).__name__))
    if not bn.affine:
        raise NotImplementedError('yolact_amd %s: affine = False is not supported' % who)
    if not bn.track_running_stats:
        raise NotImplementedError('yolact_amd %s: track_running_stats = False is not supported' % who)
    if bn.momentum is None:
        raise NotImplementedError('yolact_amd %s: momentum = None (a cumulative average) is not supported' % who)
    stats = bool(bn.training if batch_stats is None else batch_stats)
    Cc = int(bn.num_features)
    if x.dim() < 2 or x.shape[-1] != Cc or Cc % 4 != 0:
        raise NotImplementedError('yolact_amd %s: x %s for %d features is not supported ([..,C] with C %% 4 == 0 is)'
                                  % (who, tuple(x.shape), Cc))
    if residual is not None:
        L.require_cuda(residual, who + ' residual')
        if residual.shape != x.shape:
            raise ValueError('%s: residual %s for x %s' % (who, tuple(residual.shape), tuple(x.shape)))
    if stats and x.numel() // Cc < 2:
        raise NotImplementedError('yolact_amd %s: batch statistics over npos = %d values per channel are not supported '
                                  '(more than one is; PyTorch refuses it too)' % (who, x.numel() // Cc))
    L.require_cuda(bn.weight, who + ' bn.weight')
    for t in (bn.running_mean, bn.running_var):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != x.device:
            raise NotImplementedError('yolact_amd %s: running statistics that are not contiguous fp32 on the device of x '
                                      'are not supported' % who)
    return stats


def _bn_stats_written(bn):
    """After a launch with batch statistics: what nn.BatchNorm2d itself does to its buffers besides the values."""
    with torch.no_grad():
        bn.num_batches_tracked += 1
    for t in (bn.running_mean, bn.running_var):            # written by the kernel: tell autograd's version check, as an in-place op does
        torch.autograd.graph.increment_version(t)


def _batch_norm(who, act, x, bn, batch_stats, residual):
    stats = _check_bn(who, x, bn, batch_stats, residual)
    y = Bn.apply(act, stats, float(bn.eps), float(bn.momentum), bn.running_mean, bn.running_var, x, residual, bn.weight, bn.bias)
    if stats:
        _bn_stats_written(bn)
    return y


def batch_norm_act(x, bn, batch_stats=None, residual=None, relu=False):
    """relu(bn(x) + residual) on NHWC x for an nn.BatchNorm2d `bn`.  batch_stats None follows bn.training; True: the batch statistics
    (running_mean / running_var updated in place, num_batches_tracked incremented); False: the running statistics (frozen)."""
    return _batch_norm('batch_norm_act', 'relu' if relu else None, x, bn, batch_stats, residual)


def batch_norm_leaky(x, bn, batch_stats=None, residual=None):
    """leaky_relu(bn(x), 0.1) + residual on NHWC x for an nn.BatchNorm2d `bn`: the residual is added AFTER the activation (a
    DarkNetBlock's `conv2(conv1(x)) + x`).  batch_stats as in batch_norm_act."""
    return _batch_norm('batch_norm_leaky', 'leaky', x, bn, batch_stats, residual)


def _check_block(who, block, name, dcn):
    """What bottleneck (dcn False) and dcn_bottleneck (dcn True) refuse alike, named: the block's kind and every plain convolution
    of it, in forward order."""
    from .. import modules as M
    if not isinstance(block, M.Bottleneck):
        raise NotImplementedError('yolact_amd %s: %s is a %s, which is not supported (a Bottleneck is)' % (who, name, type(block).__name__))
    if dcn and (not block.use_dcn or not isinstance(block.conv2, M.DCN)):
        raise NotImplementedError('yolact_amd %s: %s is not a DCN block (use_dcn = False), which is not supported (bottleneck takes it)'
                                  % (who, name))
    if not dcn and (block.use_dcn or not isinstance(block.conv2, torch.nn.Conv2d)):
        raise NotImplementedError('yolact_amd %s: %s is a DCN block (use_dcn = True), which is not supported yet' % (who, name))
    convs = [('conv1', block.conv1, 1, 1)] + ([] if dcn else [('conv2', block.conv2, 3, block.stride)]) + [('conv3', block.conv3, 1, 1)]
    if block.downsample is not None:
        convs.append(('downsample.0', block.downsample[0], 1, block.stride))
    for n, m, k, st in convs:
        if (tuple(m.kernel_size), tuple(m.stride), tuple(m.padding), tuple(m.dilation), m.groups, m.bias is None) != \
                ((k, k), (st, st), (k // 2, k // 2), (1, 1), 1, True):
            raise NotImplementedError('yolact_amd %s: %s.%s = %r is not supported (a bias-free %d x %d / stride %d / padding %d is)'
                                      % (who, name, n, m, k, k, st, k // 2))
        check_plain(m.weight, st, '%s %s.%s' % (who, name, n))


def _bottleneck(x, block, batch_stats, conv2):
    """backbone.py:37-57 on NHWC x: relu(bn1(conv1 x)), relu(bn2(conv2(.))), relu(bn3(conv3 .) + (downsample(x) or x)); conv2(map) is
    how the block's middle convolution runs.  The order of the calls is part of train_net's gradient-summation contract."""
    out = batch_norm_act(conv2d_plain(x, block.conv1.weight), block.bn1, batch_stats, relu=True)
    out = batch_norm_act(conv2(out), block.bn2, batch_stats, relu=True)
    out = conv2d_plain(out, block.conv3.weight)
    res = x
    if block.downsample is not None:
        res = batch_norm_act(conv2d_plain(x, block.downsample[0].weight, block.stride), block.downsample[1], batch_stats)
    return batch_norm_act(out, block.bn3, batch_stats, residual=res, relu=True)


def check_bottleneck(block, name='block'):
    """NotImplementedError naming what of a backbone block the kernels do not take."""
    _check_block('bottleneck', block, name, False)


def bottleneck(x, block, batch_stats=None):
    """backbone.py:37-57 on NHWC x: relu(bn1(conv1 x)), relu(bn2(conv2 .)), relu(bn3(conv3 .) + (downsample(x) or x))."""
    L.require_cuda(x, 'bottleneck x')
    check_bottleneck(block)
    return _bottleneck(x, block, batch_stats, lambda t: conv2d_plain(t, block.conv2.weight, block.stride))


def check_deform(weight, stride=1, padding=1, dilation=1, deformable_groups=1, who='deform_conv'):
    """NotImplementedError naming what of a deformable convolution the kernels do not take: anything but the 3 x 3 / padding 1 /
    dilation 1 / one deformable group / square stride 1 or 2 DCN that YOLACT++ constructs (backbone.py:22-26) on a multiple of 32
    input channels -> stride."""
    if weight.dim() != 4:
        raise NotImplementedError('yolact_amd %s: a weight of shape %s is not supported ([Cout,Cin,3,3] is)' % (who, tuple(weight.shape)))
    Cout, Cin, kh, kw = weight.shape
    if (kh, kw) != (3, 3):
        raise NotImplementedError('yolact_amd %s: a %d x %d kernel is not supported (3 x 3 is)' % (who, kh, kw))
    if isinstance(stride, str) or _pair(stride) not in ((1, 1), (2, 2)):
        raise NotImplementedError('yolact_amd %s: stride = %r is not supported (stride 1 and stride 2 are)' % (who, stride))
    if isinstance(padding, str) or _pair(padding) != (1, 1):
        raise NotImplementedError('yolact_amd %s: padding = %r is not supported (padding 1 is)' % (who, padding))
    if _pair(dilation) != (1, 1):
        raise NotImplementedError('yolact_amd %s: dilation = %r is not supported (dilation 1 is)' % (who, dilation))
    if deformable_groups != 1:
        raise NotImplementedError('yolact_amd %s: deformable_groups = %r is not supported (one deformable group is)'
                                  % (who, deformable_groups))
    if Cin % 32 != 0:
        raise NotImplementedError('yolact_amd %s: Cin = %d is not supported (a multiple of 32 input channels is)' % (who, Cin))
    return _pair(stride)[0]


def _cols_desc(xd, omd, stride):
    B, H, W, Cin = xd.shape
    Ho, Wo = _out_size(H, W, 3, 1, stride)
    d = L.DcnColsDesc()
    d.x, d.om = xd.data_ptr(), omd.data_ptr()
    d.B, d.H, d.W, d.Cin, d.Ho, d.Wo, d.stride = B, H, W, Cin, Ho, Wo, stride
    return d, Ho, Wo


class DeformCols(torch.autograd.Function):
    """apply(stride, x [B,H,W,Cin], om [B,Ho,Wo,27]) -> col [B,Ho,Wo,9*Cin], col[m, k*Cin + c] = sigmoid(logit_k) * bilinear(x, point_k)[c]
    (csrc/dcn_train.hip).  The backward writes the inverted index's entries, sorts their int32 keys stably with torch.sort, and
    gathers gx in that order; g_om is one launch of fixed-tree dot products."""

    @staticmethod
    def forward(ctx, stride, x, om):
        dev = x.device
        with torch.cuda.device(dev), torch.no_grad():
            xd, omd = LC.f32(x, dev), LC.f32(om, dev)
            d, Ho, Wo = _cols_desc(xd, omd, stride)
            col = torch.empty(xd.shape[0], Ho, Wo, 9 * xd.shape[3], dtype=torch.float32, device=dev)
            d.col = col.data_ptr()
            L.check(L.lib().ymi_dcn_cols_fwd_f32(C.byref(d), L.stream_ptr()), 'ymi_dcn_cols_fwd_f32')
        ctx.save_for_backward(x, om)                        # (the version check)
        ctx.stride, ctx.dtypes = stride, (x.dtype, om.dtype)
        return col

    @staticmethod
    @once_differentiable
    def backward(ctx, dcol):
        x, om = ctx.saved_tensors
        want_x, want_om = ctx.needs_input_grad[1:3]
        if not (want_x or want_om):
            return None, None, None
        dev = x.device
        with torch.cuda.device(dev), torch.no_grad():
            xd, omd, dcold = LC.f32(x, dev), LC.f32(om, dev), LC.f32(dcol, dev)
            d, Ho, Wo = _cols_desc(xd, omd, ctx.stride)
            B, H, W, _ = xd.shape
            d.dcol = dcold.data_ptr()
            gx = g_om = None
            if want_x:
                n = 36 * B * Ho * Wo
                keys = torch.empty(n, dtype=torch.int32, device=dev)
                coef = torch.empty(n, dtype=torch.float32, device=dev)
                d.keys, d.coef = keys.data_ptr(), coef.data_ptr()
                L.check(L.lib().ymi_dcn_cols_entries_f32(C.byref(d), L.stream_ptr()), 'ymi_dcn_cols_entries_f32')
                # ascending target pixel, ties in entry order: the permutation of a stable sort is unique, whatever its internals
                skeys, order = torch.sort(keys, stable=True)
                seg = torch.empty(B * H * W + 1, dtype=torch.int32, device=dev)
                gx = torch.empty_like(xd)
                d.sorted_keys, d.order, d.seg, d.gx = skeys.data_ptr(), order.data_ptr(), seg.data_ptr(), gx.data_ptr()
            if want_om:
                g_om = torch.empty_like(omd)
                d.g_om = g_om.data_ptr()
            L.check(L.lib().ymi_dcn_cols_bwd_f32(C.byref(d), L.stream_ptr()), 'ymi_dcn_cols_bwd_f32')
        return None, (None if gx is None else gx.to(ctx.dtypes[0])), (None if g_om is None else g_om.to(ctx.dtypes[1]))


def deform_conv(x, om, weight, bias, stride=1):
    """The modulated deformable convolution of a DCN (dcn_v2.py:16-52, 118-128) on NHWC x [B,H,W,Cin]: om [B,Ho,Wo,27] is the RAW
    output of the DCN's conv_offset_mask (channel 2k = dh_k, 2k + 1 = dw_k, 18 + k = the mask logit of tap k = 3i + j; the sigmoid is
    applied here), weight [Cout,Cin,3,3] and bias [Cout] (or None) in torch layout -> [B,Ho,Wo,Cout].  Two steps: the modulated
    column tensor (DeformCols), then Conv as a 1 x 1 convolution of its 9 Cin channels with the weight viewed as [Cout, 9 Cin, 1, 1]
    (autograd carries the gradient back to [Cout,Cin,3,3]).  Once differentiable in x, om, weight and bias; no floating-point
    atomics, the same inputs give the same bits."""
    L.require_cuda(x, 'deform_conv x')
    L.require_cuda(om, 'deform_conv om')
    L.require_cuda(weight, 'deform_conv weight')
    st = check_deform(weight, stride)
    _check_x('deform_conv', x, weight)
    Cout, Cin = int(weight.shape[0]), int(weight.shape[1])
    B, H, W, _ = x.shape
    Ho, Wo = _out_size(H, W, 3, 1, st)
    if tuple(om.shape) != (B, Ho, Wo, 27):
        raise ValueError('deform_conv: om %s for x %s at stride %d ([B,Ho,Wo,27] = %s is expected)'
                         % (tuple(om.shape), tuple(x.shape), st, (B, Ho, Wo, 27)))
    if bias is not None:
        L.require_cuda(bias, 'deform_conv bias')
        if bias.numel() != Cout:
            raise ValueError('deform_conv: weight %s / bias %s' % (tuple(weight.shape), tuple(bias.shape)))
    if min(B, H, W, Ho, Wo) < 1:
        raise ValueError('deform_conv: x %s has no output pixel at stride %d' % (tuple(x.shape), st))
    # the column tensor is the 1 x 1 convolution's input: the conv engine and the weight gradient address it with 31-bit byte offsets
    if B * Ho * Wo * 9 * Cin >= 1 << 29 or B * H * W * Cin >= 1 << 29:
        raise NotImplementedError('yolact_amd deform_conv: x %s gives a column tensor of %d elements, which is not supported (fewer '
                                  'than 2^29, 2 GiB, are)' % (tuple(x.shape), B * Ho * Wo * 9 * Cin))
    w1 = weight.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin, 1, 1)
    k, pad = check_conv(w1, 0, who='deform_conv')
    col = DeformCols.apply(st, x, om)
    return Conv.apply(k, pad, 1, (L.ACT_NONE,), False, col, w1, bias)[0]


def check_dcn_bottleneck(block, name='block'):
    """NotImplementedError naming what of a DCN backbone block (a modules.Bottleneck with use_dcn = True) the kernels do not take."""
    _check_block('dcn_bottleneck', block, name, True)
    dcn, st = block.conv2, block.stride
    if tuple(dcn.stride) != (st, st):
        raise NotImplementedError('yolact_amd dcn_bottleneck: %s.conv2 has stride %r in a block of stride %r, which is not supported'
                                  % (name, tuple(dcn.stride), st))
    check_deform(dcn.weight, dcn.stride, dcn.padding, dcn.dilation, dcn.deformable_groups, 'dcn_bottleneck %s.conv2' % name)
    com = dcn.conv_offset_mask
    if (tuple(com.kernel_size), tuple(com.stride), tuple(com.padding), tuple(com.dilation), com.groups, com.bias is None,
            com.out_channels) != ((3, 3), (st, st), (1, 1), (1, 1), 1, False, 27):
        raise NotImplementedError('yolact_amd dcn_bottleneck: %s.conv2.conv_offset_mask = %r is not supported (a biased 3 x 3 / '
                                  'stride %d / padding 1 convolution to 27 channels is)' % (name, com, st))
    check_plain(com.weight, st, 'dcn_bottleneck %s.conv2.conv_offset_mask' % name)


def dcn_bottleneck(x, block, batch_stats=None):
    """backbone.py:37-57 on NHWC x for a block whose conv2 is a DCN (dcn_v2.py:97-128): relu(bn1(conv1 x)); om = conv_offset_mask of
    that map; relu(bn2(deform_conv(., om))); relu(bn3(conv3 .) + (downsample(x) or x))."""
    L.require_cuda(x, 'dcn_bottleneck x')
    check_dcn_bottleneck(block)
    dcn = block.conv2
    com = dcn.conv_offset_mask

    def conv2(out):
        om = conv2d_act(out, com.weight, com.bias, 1) if block.stride == 1 else conv2d_down(out, com.weight, com.bias)
        return deform_conv(out, om, dcn.weight, dcn.bias, block.stride)
    return _bottleneck(x, block, batch_stats, conv2)


# the two convolutions of the 3-channel image: (name, k, pad, stride, weight-gradient descriptor, its workspace kind, its entry)
ImageConvSpec = collections.namedtuple('ImageConvSpec', 'name k pad stride desc ws entry')
STEM = ImageConvSpec('stem_conv', 7, 3, 2, L.StemWgradDesc, 'STEM_WGRAD', 'ymi_stem_wgrad_nhwc_f32')
PRE = ImageConvSpec('preconv', 3, 1, 1, L.PreconvWgradDesc, 'PRECONV_WGRAD', 'ymi_preconv_wgrad_nhwc_f32')


def _check_image_conv(s, who, weight, stride, padding, dilation, groups, bias):
    """NotImplementedError naming what of a convolution of the image the kernels do not take: anything but a bias-free s.k x s.k /
    stride s.stride / padding s.pad / dilation 1 / groups 1 convolution of 3 input channels to a multiple of 32 output channels."""
    if weight.dim() != 4:
        raise NotImplementedError('yolact_amd %s: a weight of shape %s is not supported ([Cout,3,%d,%d] is)'
                                  % (who, tuple(weight.shape), s.k, s.k))
    Cout, Cin, kh, kw = weight.shape
    if (kh, kw) != (s.k, s.k):
        raise NotImplementedError('yolact_amd %s: a %d x %d kernel is not supported (%d x %d is)' % (who, kh, kw, s.k, s.k))
    if isinstance(stride, str) or _pair(stride) != (s.stride, s.stride):
        raise NotImplementedError('yolact_amd %s: stride = %r is not supported (stride %d is)' % (who, stride, s.stride))
    if isinstance(padding, str) or _pair(padding) != (s.pad, s.pad):
        raise NotImplementedError('yolact_amd %s: padding = %r is not supported (padding %d is)' % (who, padding, s.pad))
    if _pair(dilation) != (1, 1):
        raise NotImplementedError('yolact_amd %s: dilation = %r is not supported (dilation 1 is)' % (who, dilation))
    if groups != 1:
        raise NotImplementedError('yolact_amd %s: groups = %r is not supported (groups 1 is)' % (who, groups))
    if Cin != 3:
        raise NotImplementedError('yolact_amd %s: Cin = %d is not supported (3 input channels are, on an input padded to 4)' % (who, Cin))
    if bias is not None:
        raise NotImplementedError('yolact_amd %s: a bias is not supported (a bias-free convolution is)' % who)
    if Cout % 32 != 0:
        raise NotImplementedError('yolact_amd %s: Cout = %d is not supported (a multiple of 32 output channels is)' % (who, Cout))


def check_stem(weight, stride=2, padding=3, dilation=1, groups=1, bias=None, who='stem_conv'):
    """What of the stem convolution (7 x 7 / stride 2 / padding 3, backbone.py:77) the kernels do not take (_check_image_conv)."""
    _check_image_conv(STEM, who, weight, stride, padding, dilation, groups, bias)


def check_preconv(weight, stride=1, padding=1, dilation=1, groups=1, bias=None, who='preconv'):
    """What of DarkNet's pre-convolution (3 x 3 / stride 1 / padding 1, backbone.py:268) the kernels do not take (_check_image_conv)."""
    _check_image_conv(PRE, who, weight, stride, padding, dilation, groups, bias)


def _pack_image(w):
    """[Cout,3,k,k] -> [ceil128(Cout)][ceil32(4*k*k)], column (ky*k + kx)*4 + c with c = 3 and the columns from 4*k*k on zero (a
    permute of the CURRENT values): [..][224] for the stem, [..][64] for the pre-convolution."""
    Cout, _, k, _ = w.shape
    out = torch.zeros(_ceil(Cout, 128), _ceil(k * k * 4, 32), dtype=torch.float32, device=w.device)
    out[:Cout, :k * k * 4] = F.pad(w.permute(0, 2, 3, 1), (0, 1)).reshape(Cout, k * k * 4)
    return out


class ImageConv(torch.autograd.Function):
    """apply(spec, x4 [B,H,W,4], weight [Cout,3,k,k]) -> [B,Ho,Wo,Cout]; differentiable in the weight.  One ymi_conv2d_nhwc_f32 launch
    through the engine's Cin-4 loader with the filter's fourth input channel zero; the backward is the spec's weight-gradient entry
    on the SAME x4 (its fourth channel reaches nothing), then _unpack_dw."""

    @staticmethod
    def forward(ctx, s, x4, weight):
        dev = x4.device
        Cout = int(weight.shape[0])
        with torch.cuda.device(dev), torch.no_grad():
            xd = LC.f32(x4, dev)
            B, H, W, _ = xd.shape
            Ho, Wo = _out_size(H, W, s.k, s.pad, s.stride)
            y = torch.empty(B, Ho, Wo, Cout, dtype=torch.float32, device=dev)
            _engine_conv(xd, 4, _pack_image(weight.detach().float()), None, 4, Cout, s.k, s.pad, [(0, Cout, L.ACT_NONE, y)],
                         stride=s.stride)
        ctx.save_for_backward(x4, weight)                   # (the version check)
        ctx.spec, ctx.dtype = s, weight.dtype
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x4, weight = ctx.saved_tensors                      # (the version check)
        if not ctx.needs_input_grad[2]:
            return None, None, None
        s, dev = ctx.spec, x4.device
        Cout = int(weight.shape[0])
        with torch.cuda.device(dev), torch.no_grad():
            xd, g = LC.f32(x4, dev), LC.f32(dy, dev)
            B, H, W, _ = xd.shape
            dw = torch.empty(s.k * s.k * 3, Cout, dtype=torch.float32, device=dev)
            d = s.desc()
            d.x, d.g, d.dw = xd.data_ptr(), g.data_ptr(), dw.data_ptr()
            d.B, d.H, d.W, d.Cout, d.ldg = B, H, W, Cout, Cout
            ws = LC.workspace(s.ws, d, dev)
            d.ws_bytes = ws.numel()
            L.check(getattr(L.lib(), s.entry)(C.byref(d), L.stream_ptr()), s.entry)
            out = _unpack_dw(dw, s.k, 3)
        return None, None, out.to(ctx.dtype)


def _image_conv(s, x4, weight, bias, stride, padding, dilation, groups):
    L.require_cuda(x4, s.name + ' x4')
    L.require_cuda(weight, s.name + ' weight')
    _check_image_conv(s, s.name, weight, stride, padding, dilation, groups, bias)
    if x4.dim() != 4 or x4.shape[3] != 4:
        raise ValueError('%s: x4 %s ([B,H,W,4], the image padded to 4 channels, is expected)' % (s.name, tuple(x4.shape)))
    # nothing upstream of the image needs a gradient, and returning None would silently give a zero one
    if x4.requires_grad:
        raise NotImplementedError('yolact_amd %s: an x4 that requires grad is not supported (the gradient with respect to the '
                                  'image is not computed; detach it)' % s.name)
    return ImageConv.apply(s, x4, weight)


def stem_conv(x4, weight, bias=None, stride=2, padding=3, dilation=1, groups=1):
    """conv2d(x, weight, None, stride 2, padding 3) for a [Cout,3,7,7] weight on x4 [B,H,W,4], the NHWC image with a fourth channel of
    zeros -> NHWC.  Differentiable in the weight only."""
    return _image_conv(STEM, x4, weight, bias, stride, padding, dilation, groups)


def preconv(x4, weight, bias=None, stride=1, padding=1, dilation=1, groups=1):
    """conv2d(x, weight, None, stride 1, padding 1) for a [Cout,3,3,3] weight (DarkNet's _preconv, backbone.py:268) on x4 [B,H,W,4], the
    NHWC image with a fourth channel of zeros -> NHWC.  Differentiable in the weight only, like stem_conv."""
    return _image_conv(PRE, x4, weight, bias, stride, padding, dilation, groups)


class MaxPool3x3S2(torch.autograd.Function):
    """apply(x [B,H,W,C]) -> [B,Hp,Wp,C]."""

    @staticmethod
    def forward(ctx, x):
        dev = x.device
        with torch.cuda.device(dev), torch.no_grad():
            xd = LC.f32(x, dev)
            B, H, W, Cc = xd.shape
            y = torch.empty(B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cc, dtype=torch.float32, device=dev)
            L.check(L.lib().ymi_maxpool_fwd_nhwc_f32(xd.data_ptr(), y.data_ptr(), B, H, W, Cc, L.stream_ptr()), 'ymi_maxpool_fwd_nhwc_f32')
        ctx.save_for_backward(x)                            # the backward finds the argmax in it again; (the version check)
        ctx.dtype = x.dtype
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors                            # (the version check)
        if not ctx.needs_input_grad[0]:
            return None
        dev = x.device
        with torch.cuda.device(dev), torch.no_grad():
            xd, dyd = LC.f32(x, dev), LC.f32(dy, dev)
            B, H, W, Cc = xd.shape
            dx = torch.empty_like(xd)
            L.check(L.lib().ymi_maxpool_bwd_nhwc_f32(xd.data_ptr(), dyd.data_ptr(), dx.data_ptr(), B, H, W, Cc, L.stream_ptr()),
                    'ymi_maxpool_bwd_nhwc_f32')
        return dx.to(ctx.dtype)


def max_pool_3x3_s2(x):
    """F.max_pool2d(x, 3, 2, 1) on NHWC x -> NHWC; of equal maxima the first in row-major window order takes the gradient."""
    L.require_cuda(x, 'max_pool_3x3_s2 x')
    if x.dim() != 4 or x.shape[3] % 4 != 0 or min(x.shape) < 1:
        raise NotImplementedError('yolact_amd max_pool_3x3_s2: x %s is not supported ([B,H,W,C] with C %% 4 == 0 is)' % (tuple(x.shape),))
    return MaxPool3x3S2.apply(x)


def _check_unit(seq, who, name):
    """A DarkNet unit: Sequential(bias-free Conv2d, BatchNorm2d, LeakyReLU(0.1)) -> (conv, bn); anything else is refused by name."""
    mods = list(seq) if isinstance(seq, torch.nn.Sequential) else None
    if mods is None or len(mods) != 3 or not isinstance(mods[0], torch.nn.Conv2d) or not isinstance(mods[1], torch.nn.BatchNorm2d) \
            or not isinstance(mods[2], torch.nn.LeakyReLU):
        raise NotImplementedError('yolact_amd %s: %s = %r is not supported (a Sequential of Conv2d, BatchNorm2d, LeakyReLU(0.1) is)'
                                  % (who, name, seq))
    if mods[2].negative_slope != LEAKY_SLOPE:
        raise NotImplementedError('yolact_amd %s: %s has negative_slope = %r, which is not supported (0.1 is)'
                                  % (who, name, mods[2].negative_slope))
    conv = mods[0]
    if conv.bias is not None:
        raise NotImplementedError('yolact_amd %s: %s.0 has a bias, which is not supported (a bias-free convolution is)' % (who, name))
    if isinstance(conv.padding, str) or tuple(conv.padding) != (conv.kernel_size[0] // 2,) * 2:
        raise NotImplementedError('yolact_amd %s: %s.0 has padding = %r, which is not supported (padding k // 2 is)'
                                  % (who, name, conv.padding))
    if tuple(conv.dilation) != (1, 1) or conv.groups != 1:
        raise NotImplementedError('yolact_amd %s: %s.0 has dilation = %r / groups = %r, which is not supported (dilation 1 / groups 1 '
                                  'is)' % (who, name, tuple(conv.dilation), conv.groups))
    return conv, mods[1]


def dark_unit(x, seq, batch_stats=None, residual=None):
    """A DarkNet unit (backbone.py:222-233's conv, BatchNorm2d, LeakyReLU(0.1)) on NHWC x, + residual behind the activation."""
    L.require_cuda(x, 'dark_unit x')
    conv, bn = _check_unit(seq, 'dark_unit', 'seq')
    check_plain(conv.weight, conv.stride, 'dark_unit seq.0')
    return batch_norm_leaky(conv2d_plain(x, conv.weight, conv.stride), bn, batch_stats, residual)


def _check_dark_block(block, who, name):
    from .. import modules as M
    if not isinstance(block, M.DarkNetBlock):
        raise NotImplementedError('yolact_amd %s: %s is a %s, which is not supported (a DarkNetBlock is)' % (who, name, type(block).__name__))
    for n, k in (('conv1', 1), ('conv2', 3)):
        conv, _ = _check_unit(getattr(block, n), who, '%s.%s' % (name, n))
        if tuple(conv.kernel_size) != (k, k) or tuple(conv.stride) != (1, 1):
            raise NotImplementedError('yolact_amd %s: %s.%s.0 = %r is not supported (a %d x %d / stride 1 convolution is)'
                                      % (who, name, n, conv, k, k))
        check_plain(conv.weight, 1, '%s %s.%s.0' % (who, name, n))
    if block.conv2[0].out_channels != block.conv1[0].in_channels:
        raise NotImplementedError('yolact_amd %s: %s maps %d to %d channels, which is not supported (the residual needs equal widths)'
                                  % (who, name, block.conv1[0].in_channels, block.conv2[0].out_channels))


def dark_block(x, block, batch_stats=None):
    """A DarkNetBlock (backbone.py:235-247) on NHWC x: conv2(conv1(x)) + x, the sum behind conv2's LeakyReLU."""
    L.require_cuda(x, 'dark_block x')
    _check_dark_block(block, 'dark_block', 'block')
    return dark_unit(dark_unit(x, block.conv1, batch_stats), block.conv2, batch_stats, residual=x)


def check_darknet(bb, name='backbone'):
    """NotImplementedError naming what of a DarkNet backbone the kernels do not take."""
    from .. import modules as M
    who = 'darknet'
    if not isinstance(bb, M.DarkNetBackbone):
        raise NotImplementedError('yolact_amd %s: %s is a %s, which is not supported (a DarkNetBackbone is)' % (who, name, type(bb).__name__))
    conv, _ = _check_unit(bb._preconv, who, name + '._preconv')
    check_preconv(conv.weight, conv.stride, conv.padding, conv.dilation, conv.groups, conv.bias, '%s %s._preconv.0' % (who, name))
    for i, layer in enumerate(bb.layers):
        mods = list(layer)
        if not mods:
            raise NotImplementedError('yolact_amd %s: %s.layers.%d is empty, which is not supported' % (who, name, i))
        conv, _ = _check_unit(mods[0], who, '%s.layers.%d.0' % (name, i))
        if tuple(conv.kernel_size) != (3, 3) or tuple(conv.stride) != (2, 2):
            raise NotImplementedError('yolact_amd %s: %s.layers.%d.0.0 = %r is not supported (a 3 x 3 / stride 2 convolution is)'
                                      % (who, name, i, conv))
        check_plain(conv.weight, 2, '%s %s.layers.%d.0.0' % (who, name, i))
        for j, block in enumerate(mods[1:], 1):
            _check_dark_block(block, who, '%s.layers.%d.%d' % (name, i, j))
