"""Oracles of train_ops.conv_mode('fp16x2') (csrc/conv_pack_h2.hip and the fp16x2 tiles of the conv engine), shared by
tests/test_conv_h2_host.py and tests/test_gpu_conv_h2.py.

    pack_np(ws, mode, ld)               the pack in numpy, by index arithmetic (no permute): planes int16 [2][RowsPad][Kp] and winv
                                        [RowsPad], the row scale by ymi_h2_scale's rule (wgrad_h2_ref.h2_scale)
    pack_torch(ws, mode, ld)            the exact oracle: engine.split2_planes_f16 of train_ops._pack_forward / _pack_dgrad
    PACK_CASES / pack_inputs(name)      the filter sets of the pack test
    oracle(case, dtype)                 y, dx, dw, db of a convolution case by torch autograd through F.conv2d in `dtype`
    restate(x, w, k, pad, stride, ...)  the forward's arithmetic in numpy: one power-of-two scale for x from max |x|, one per filter
                                        row, t = fp32(v s), h = fp16(t), l = fp16(t - h), the three products hh + hl + lh as fp32
                                        matrix products added in fp32, the scales undone by powers of two.  drop_lh: without the
                                        x_l w_h product.  drop_block: one block of 32 input channels reads as zero.
    dgrad_as_forward(g, w, pad)         the stride-1 data gradient as a forward convolution: (g, w flipped and transposed, k - 1 - pad)
    error_bound(x, w, k, pad, stride)   E [B,Ho,Wo,Cout] of the range cases (the derivation is in tests/test_gpu_conv_h2.py)
    CASES / inputs(name)                the shape cases: name -> what is called on what
    RANGE / range_inputs(kind)          the range cases on the 5 x 7 shape
"""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from wgrad_h2_ref import bar, h2_scale  # noqa: F401  (the project's bar; ymi_h2_scale in Python)


def _ceil(a, b):
    return (a + b - 1) // b * b


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


# ---- the pack ------------------------------------------------------------------------------------------------------------------------
def packing_np(ws, mode, ld=0):
    """The unsplit packing [RowsPad][Kp] in fp32 by index arithmetic.  ws: numpy arrays [co,Cin,k,k]."""
    cat = np.concatenate(ws, 0)
    ctot, Cin, k, _ = cat.shape
    if mode == 0:
        out = np.zeros((_ceil(ctot, 128), k * k * Cin), np.float32)
        for ky in range(k):
            for kx in range(k):
                out[:ctot, (ky * k + kx) * Cin:(ky * k + kx + 1) * Cin] = cat[:, :, ky, kx]
    else:
        out = np.zeros((_ceil(Cin, 128), k * k * ld), np.float32)
        for ky in range(k):
            for kx in range(k):
                out[:Cin, (ky * k + kx) * ld:(ky * k + kx) * ld + ctot] = cat[:, :, k - 1 - ky, k - 1 - kx].T
    return out


def split_rows_np(P):
    """[R][K] fp32 -> (planes int16 [2][R][K], winv fp32 [R]): per row s = h2_scale(max |row|), h = fp16(v s), l = fp16(v s - h)."""
    s = np.array([h2_scale(m) for m in np.abs(P).max(axis=1)], np.float64)
    with np.errstate(over='ignore', invalid='ignore', under='ignore'):
        t = (P * s[:, None].astype(np.float32)).astype(np.float32)
        h = t.astype(np.float16)
        l = (t - h.astype(np.float32)).astype(np.float32).astype(np.float16)
    return np.stack([h.view(np.int16), l.view(np.int16)]), (1.0 / s).astype(np.float32)


def pack_np(ws, mode, ld=0):
    return split_rows_np(packing_np([w.numpy() for w in ws], mode, ld))


def pack_torch(ws, mode, ld=0):
    """engine.split2_planes_f16 of the torch packing -> numpy (planes int16 [2][RowsPad][Kp], winv [RowsPad])."""
    from yolact_amd.engine import split2_planes_f16
    from yolact_amd.layers import train_ops as TO
    cat = torch.cat(list(ws), 0)
    planes, winv = split2_planes_f16(TO._pack_forward(cat) if mode == 0 else TO._pack_dgrad(cat, ld))
    return planes.numpy(), winv.numpy()


# name -> (filter shapes, ld of mode 1, what is special).  Every row maximum is 0 or a normal number in [2^-100, 2^100]: the range in
# which the device pack must equal the torch packing bit for bit.
PACK_CASES = {
    '1x1_5': ([(5, 32, 1, 1)], 32, None),
    '3x3_130': ([(130, 64, 3, 3)], 160, None),                          # crosses a 128-row pad and mode 1's 128-column block; 30 zero columns
    'head3': ([(12, 32, 3, 3), (243, 32, 3, 3), (96, 32, 3, 3)], 352, None),   # the prediction head's three tensors, 351 channels
    'zero_filter': ([(40, 32, 3, 3)], 64, 'zero_filter'),               # filter 7 all zero: a zero row in mode 0
    'zero_channel': ([(40, 32, 1, 1)], 64, 'zero_channel'),             # input channel 9 all zero: a zero row in mode 1
    'mag_filters': ([(6, 64, 3, 3)], 32, 'mag_filters'),                # filters of magnitude 2^-60 and 2^50: rows in mode 0
    'mag_channels': ([(6, 64, 3, 3)], 32, 'mag_channels'),              # input channels of those magnitudes: rows in mode 1
    'cin288': ([(8, 288, 3, 3)], 32, None),                             # more channels than one staging pass of mode 0 holds
    'two_1x1': ([(70, 32, 1, 1), (20, 32, 1, 1)], 96, None),            # two pointwise tensors, more filters than one pass of mode 1 holds in flight
}
_CACHE = {}


def pack_inputs(name):
    """-> list of fp32 filter tensors, seeded by the name; cached and never written to."""
    key = ('pack', name)
    if key not in _CACHE:
        shapes, ld, special = PACK_CASES[name]
        gen = _gen(name)
        ws = [torch.randn(*s, generator=gen) * 0.05 for s in shapes]
        if special == 'zero_filter':
            ws[0][7] = 0
        elif special == 'zero_channel':
            ws[0][:, 9] = 0
        elif special == 'mag_filters':
            ws[0][1] *= 2.0 ** -60
            ws[0][2] *= 2.0 ** 50
        elif special == 'mag_channels':
            ws[0][:, 3] *= 2.0 ** -60
            ws[0] *= 2.0 ** 50                                           # then channel 3 is 2^-10 and the others 2^50
            ws[0][:, 5] *= 2.0 ** -110                                   # and channel 5 is 2^-60
        _CACHE[key] = [w.contiguous() for w in ws]
    return _CACHE[key]


# ---- the convolutions ----------------------------------------------------------------------------------------------------------------
def out_size(n, k, pad, stride):
    return (n + 2 * pad - k) // stride + 1


def conv64(x, w, b, pad, stride, dtype=torch.float64):
    """x [B,H,W,Cin], w [Cout,Cin,k,k] -> y [B,Ho,Wo,Cout] in dtype."""
    y = F.conv2d(x.permute(0, 3, 1, 2).to(dtype), w.to(dtype), None if b is None else b.to(dtype), stride=stride, padding=pad)
    return y.permute(0, 2, 3, 1).contiguous()


def im2col(x, k, pad, stride):
    """x [B,H,W,Cin] numpy -> [P, k*k*Cin] over the output positions, zeros outside the input; column (ky*k + kx)*Cin + c."""
    B, H, W, Cin = x.shape
    Ho, Wo = out_size(H, k, pad, stride), out_size(W, k, pad, stride)
    xp = np.zeros((B, H + 2 * pad + stride, W + 2 * pad + stride, Cin), dtype=x.dtype)
    xp[:, pad:pad + H, pad:pad + W] = x
    cols = [xp[:, ky:ky + stride * Ho:stride, kx:kx + stride * Wo:stride] for ky in range(k) for kx in range(k)]
    return np.concatenate(cols, axis=3).reshape(B * Ho * Wo, k * k * Cin)


def split_np(v, s):
    """fp32 array v, scale s (scalar or broadcastable) -> (h, l) as fp32 arrays holding fp16 values."""
    with np.errstate(over='ignore', invalid='ignore', under='ignore'):
        t = (v.astype(np.float32) * np.asarray(s, np.float32)).astype(np.float32)
        h = t.astype(np.float16)
        l = (t - h.astype(np.float32)).astype(np.float32).astype(np.float16)
    return h.astype(np.float32), l.astype(np.float32)


def restate(x, w, k, pad, stride, drop_lh=False, drop_block=None):
    """x [B,H,W,Cin], w [Cout,Cin,k,k] fp32 tensors -> y [B,Ho,Wo,Cout] fp32 tensor by the mode's arithmetic (module docstring).
    fp16 x fp16 products are exact in fp32; the sums are numpy's fp32 matrix products (another order than the kernel's: the restatement
    shows that the arithmetic meets the bars, not the bits)."""
    xn = x.numpy()
    B, H, W, Cin = xn.shape
    Cout = w.shape[0]
    P = packing_np([w.numpy()], 0)[:Cout]                                 # [Cout, k*k*Cin]
    sx = h2_scale(np.abs(xn).max())
    sw = np.array([h2_scale(m) for m in np.abs(P).max(axis=1)], np.float64)
    xh, xl = split_np(xn, sx)
    wh, wl = split_np(P, sw[:, None])
    if drop_block is not None:
        for t in range(k * k):
            wh[:, t * Cin + 32 * drop_block:t * Cin + 32 * drop_block + 32] = 0
            wl[:, t * Cin + 32 * drop_block:t * Cin + 32 * drop_block + 32] = 0
    ah, al = im2col(xh, k, pad, stride), im2col(xl, k, pad, stride)
    with np.errstate(over='ignore', invalid='ignore', under='ignore'):
        acc = ah @ wh.T + ah @ wl.T
        if not drop_lh:
            acc = acc + al @ wh.T
        # the scales are powers of two: undone one after the other, the product of the scales is never formed
        y = (acc * np.float32(1.0 / sx)) * (1.0 / sw).astype(np.float32)[None, :]
    return torch.from_numpy(y.astype(np.float32)).view(B, out_size(H, k, pad, stride), out_size(W, k, pad, stride), Cout)


def dgrad_as_forward(g, w, pad):
    """The stride-1 data gradient dx = conv(g, w'), w'[ci,co,ky,kx] = w[co,ci,k-1-ky,k-1-kx], padding k - 1 - pad -> (g, w', pad')."""
    k = w.shape[2]
    return g, w.flip(2, 3).permute(1, 0, 2, 3).contiguous(), k - 1 - pad


def error_bound(x, w, k, pad, stride):
    """E[m,co] = (3 * 2^-22 + K * 2^-24) * sum |x| |w| + 2^-38 * (amax_x * sum |w[co]| + rowmax_w[co] * sum |x|), K = k k Cin, the sums
    in fp64 over what the output reads (a tap outside the map reads nothing) -> [B,Ho,Wo,Cout]."""
    xn = x.numpy().astype(np.float64)
    B, H, W, Cin = xn.shape
    Cout = w.shape[0]
    P = np.abs(packing_np([w.numpy()], 0)[:Cout].astype(np.float64))
    a = np.abs(im2col(xn, k, pad, stride))
    reads = im2col(np.ones_like(xn), k, pad, stride)
    K = k * k * Cin
    E = (3 * 2.0 ** -22 + K * 2.0 ** -24) * (a @ P.T) + 2.0 ** -38 * (np.abs(xn).max() * (reads @ P.T) + a.sum(1)[:, None] * P.max(1)[None, :])
    return torch.from_numpy(E).view(B, out_size(H, k, pad, stride), out_size(W, k, pad, stride), Cout)


# name -> (op, x shape, [(filter shape, biased, act)], stride).  op: the public function; padding k // 2 everywhere.
CASES = {
    'act_tanh': ('conv2d_act', (2, 5, 7, 64), [((40, 64, 3, 3), True, 'tanh')], 1),         # test_gpu_wgrad_h2.conv_case's three
    'down': ('conv2d_down', (2, 7, 6, 32), [((48, 32, 3, 3), True, None)], 2),
    'plain_s2': ('conv2d_plain', (2, 6, 7, 32), [((64, 32, 1, 1), False, None)], 2),
    'head3': ('conv2d_multi', (2, 5, 5, 32), [((12, 32, 3, 3), True, None), ((243, 32, 3, 3), True, None), ((96, 32, 3, 3), True, 'tanh')], 1),
    '1x1_cin32': ('conv2d_plain', (2, 6, 7, 32), [((64, 32, 1, 1), False, None)], 1),        # Kpad / 32 = 1: the pipelined kernel refuses
    'big_m': ('conv2d_plain', (1, 128, 128, 32), [((128, 32, 3, 3), False, None)], 1),       # M = 16384, Cin = 32, a full 128-column tile
    'wide': ('conv2d_plain', (2, 6, 7, 128), [((128, 128, 3, 3), False, None)], 1),          # 128 columns both ways, M = 84
    'narrow_big_m': ('conv2d_plain', (2, 128, 128, 32), [((30, 32, 3, 3), False, None)], 1),  # M = 32768, N <= 32: the engine picks 128x32
    'plain3_s2': ('conv2d_plain', (2, 6, 7, 32), [((64, 32, 3, 3), False, None)], 2),        # a 3x3 whose dx is the tap-exact kernel's
}


def inputs(name):
    """-> (x [B,H,W,Cin], [(w, b or None)], [gy per output, NHWC]) fp32, seeded by the name; cached and never written to."""
    key = ('conv', name)
    if key not in _CACHE:
        op, xs, layers, stride = CASES[name]
        gen = _gen(name)
        x = torch.randn(*xs, generator=gen)
        params = [(torch.randn(*ws, generator=gen) * 0.05, torch.randn(ws[0], generator=gen) if biased else None) for ws, biased, _ in layers]
        k = layers[0][0][2]
        Ho, Wo = out_size(xs[1], k, k // 2, stride), out_size(xs[2], k, k // 2, stride)
        gys = [torch.randn(xs[0], Ho, Wo, ws[0], generator=gen) for ws, _, _ in layers]
        _CACHE[key] = (x, params, gys)
    return _CACHE[key]


def oracle(name, dtype):
    """-> dict(y0.., dx, w0.., b0..) in fp64 values computed in `dtype`; cached."""
    key = ('oracle', name, dtype)
    if key not in _CACHE:
        op, xs, layers, stride = CASES[name]
        x, params, gys = inputs(name)
        xl = x.permute(0, 3, 1, 2).to(dtype).clone().requires_grad_(True)
        out, leaves, total = {}, [], None
        for i, ((w, b), gy, (_, _, act)) in enumerate(zip(params, gys, layers)):
            wl = w.to(dtype).clone().requires_grad_(True)
            bl = None if b is None else b.to(dtype).clone().requires_grad_(True)
            y = F.conv2d(xl, wl, bl, stride=stride, padding=w.shape[2] // 2)
            y = torch.tanh(y) if act == 'tanh' else y
            out['y%d' % i] = y.detach().permute(0, 2, 3, 1).double()
            t = (y * gy.permute(0, 3, 1, 2).to(dtype)).sum()
            total = t if total is None else total + t
            leaves.append((wl, bl))
        total.backward()
        out['dx'] = xl.grad.permute(0, 2, 3, 1).double()
        for i, (wl, bl) in enumerate(leaves):
            out['w%d' % i] = wl.grad.double()
            if bl is not None:
                out['b%d' % i] = bl.grad.double()
        _CACHE[key] = out
    return _CACHE[key]


# ---- the range cases -----------------------------------------------------------------------------------------------------------------
RANGE_SHAPE = ((2, 5, 7, 64), (40, 64, 3, 3))                             # a plain 3x3 / pad 1 / stride 1, K = 576
RANGE = ('pow2', 'tiny', 'huge')


def range_inputs(kind):
    """-> (x, w, gy): operands 2^U(-20, 20) with random signs, all of magnitude 2^-60, or all 2^50; gy is drawn as x is."""
    key = ('range', kind)
    if key not in _CACHE:
        gen = _gen('range_' + kind)
        xs, ws = RANGE_SHAPE
        gs = (xs[0], xs[1], xs[2], ws[0])

        def draw(shape):
            t = torch.randn(*shape, generator=gen)
            if kind == 'pow2':
                return torch.sign(t) * torch.exp2(torch.rand(*shape, generator=gen) * 40 - 20)
            return t * (2.0 ** -60 if kind == 'tiny' else 2.0 ** 50)
        _CACHE[key] = tuple(draw(s).contiguous() for s in (xs, ws, gs))
    return _CACHE[key]
