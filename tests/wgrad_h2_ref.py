"""Oracles of ymi_conv_wgrad_nhwc_h2 (csrc/conv_wgrad_h2.hip), shared by tests/test_wgrad_h2_host.py and tests/test_gpu_wgrad_h2.py.

    oracle(x, g, k, stride, dtype)      dw [k*k*Cin, Cout] and db [Cout] by torch autograd through F.conv2d in `dtype` (fp64: the truth;
                                        fp32: what sets the bar)
    restate(x, g, k, stride, ...)       the kernel's arithmetic in numpy: one power-of-two scale per tensor by ymi_h2_scale's rule, from
                                        max |x| and max |g| (the caller passes g without its padding channels), t = fp32(v s),
                                        h = fp16(t), l = fp16(t - h) by np.float16's round to nearest even, and the three products
                                        hh + hl + lh summed in fp64, so that what remains is the error of the split alone.
                                        drop_lh: without the x_l g_h product.  drop_block: one block of 32 channels of g reads as zero.
    error_bound(x, g, k, stride)        E [k*k*Cin, Cout] of the range cases (the derivation is in tests/test_gpu_wgrad_h2.py)
    CASES                               every case of the GPU test: name -> (B, H, W, Cin, Cout, ldg, k, stride, kind); inputs(name)
                                        builds x [B,H,W,Cin] and g [B,Ho,Wo,Cout] in fp32 from the name's own seed.
"""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

EXACT_BAR = 8e-6                # tests/test_gpu_class_loss.py


def out_size(n, k, stride):
    return (n + 2 * (k // 2) - k) // stride + 1


def oracle(x, g, k, stride, dtype=torch.float64):
    """x [B,H,W,Cin], g [B,Ho,Wo,Cout] (fp32 tensors) -> (dw [k*k*Cin, Cout], db [Cout]) in dtype, rows (ky*k + kx)*Cin + ci."""
    Cin, Cout = x.shape[3], g.shape[3]
    w = torch.zeros(Cout, Cin, k, k, dtype=dtype, requires_grad=True)
    b = torch.zeros(Cout, dtype=dtype, requires_grad=True)
    y = F.conv2d(x.permute(0, 3, 1, 2).to(dtype), w, b, stride=stride, padding=k // 2)
    y.backward(g.permute(0, 3, 1, 2).to(dtype))
    return w.grad.permute(2, 3, 1, 0).reshape(k * k * Cin, Cout).contiguous(), b.grad


def im2col(x, k, stride):
    """x [B,H,W,Cin] numpy fp64 -> [P, k*k*Cin] over the positions (n, oy, ox) of the output map, zeros outside the input."""
    B, H, W, Cin = x.shape
    pad = k // 2
    Ho, Wo = out_size(H, k, stride), out_size(W, k, stride)
    xp = np.zeros((B, H + 2 * pad + 2, W + 2 * pad + 2, Cin), dtype=x.dtype)
    xp[:, pad:pad + H, pad:pad + W] = x
    cols = [xp[:, ky:ky + stride * Ho:stride, kx:kx + stride * Wo:stride] for ky in range(k) for kx in range(k)]
    return np.concatenate(cols, axis=3).reshape(B * Ho * Wo, k * k * Cin)


def h2_scale(amax):
    """ymi_h2_scale (csrc/common.h) on an fp32 bound -> s as a Python float (a power of two)."""
    u = int(np.float32(amax).view(np.uint32))
    eb = (u >> 23) & 0xff
    es = 127 if eb in (0, 255) else 267 - eb
    es = min(max(es, 2), 252)
    return 2.0 ** (es - 127)


def split(v, s):
    """fp32 array v, scale s -> (h, l) as fp64 arrays holding fp16 values."""
    with np.errstate(over='ignore', invalid='ignore', under='ignore'):
        t = (v.astype(np.float32) * np.float32(s)).astype(np.float32)
        h = t.astype(np.float16)
        l = (t - h.astype(np.float32)).astype(np.float32).astype(np.float16)
    return h.astype(np.float64), l.astype(np.float64)


def restate(x, g, k, stride, drop_lh=False, drop_block=None):
    """x [B,H,W,Cin], g [B,Ho,Wo,Cout] fp32 tensors -> dw [k*k*Cin, Cout] as an fp64 tensor: the kernel's split, exact sums."""
    xn, gn = x.numpy(), g.numpy().reshape(-1, g.shape[3])
    sx, sg = h2_scale(np.abs(xn).max()), h2_scale(np.abs(gn).max())
    xh, xl = split(xn, sx)
    gh, gl = split(gn, sg)
    if drop_block is not None:
        gh[:, 32 * drop_block:32 * drop_block + 32] = 0
        gl[:, 32 * drop_block:32 * drop_block + 32] = 0
    ah, al = im2col(xh, k, stride), im2col(xl, k, stride)
    acc = ah.T @ gh + ah.T @ gl
    if not drop_lh:
        acc = acc + al.T @ gh
    return torch.from_numpy(acc / sx / sg)


def error_bound(x, g, k, stride):
    """E[k,co] = (3 * 2^-22 + P * 2^-24) * sum |a| |g| + 2^-38 * (amax_x * sum |g| + amax_g * sum |a|), the sums in fp64 over the
    positions the element reads (a tap outside the map reads nothing)."""
    xn, gn = x.numpy().astype(np.float64), g.numpy().astype(np.float64).reshape(-1, g.shape[3])
    a = np.abs(im2col(xn, k, stride))
    reads = im2col(np.ones_like(xn), k, stride)
    P = gn.shape[0]
    sab = a.T @ np.abs(gn)
    sg_, sa_ = reads.T @ np.abs(gn), a.T @ np.ones_like(gn)
    E = (3 * 2.0 ** -22 + P * 2.0 ** -24) * sab + 2.0 ** -38 * (np.abs(xn).max() * sg_ + np.abs(gn).max() * sa_)
    return torch.from_numpy(E)


# name -> (B, H, W, Cin, Cout, ldg, k, stride, kind).  kind: 'shape' (N(0,1), the bar on dw and db) or a range case on the 5 x 7 shape.
S57 = (2, 5, 7, 64, 40, 64, 3, 1)
CASES = {
    '1x1_full_k_step': (1, 4, 4, 32, 32, 32, 1, 1, 'shape'),            # P = 16: one full K-step
    '1x1_ragged_k_step': (1, 1, 17, 32, 32, 32, 1, 1, 'shape'),         # P = 17
    '3x3_5x7': S57 + ('shape',),                                        # every tap crosses a border, 8 positions straddle rows and images
    '3x3_s2_7x6': (2, 7, 6, 32, 32, 32, 3, 2, 'shape'),
    '3x3_s2_6x7': (2, 6, 7, 32, 32, 32, 3, 2, 'shape'),
    '1x1_s2_5x5': (2, 5, 5, 32, 32, 32, 1, 2, 'shape'),
    'cout160': (1, 3, 3, 32, 160, 160, 3, 1, 'shape'),                  # five column tiles: wave 0 holds two, the others one
    'cout288': (1, 3, 3, 32, 288, 288, 3, 1, 'shape'),                  # two groups of 256 output channels, one tile in the second
    'chunks': (1, 9, 11, 32, 32, 32, 1, 1, 'shape'),                    # P = 99: chunks of 32, the fourth holds 3 positions
    'range_x_pow2': S57 + ('x_pow2',),
    'range_tiny': S57 + ('tiny',),
    'range_huge': S57 + ('huge',),
    'range_g_zero': S57 + ('g_zero',),
    'range_x_zero': S57 + ('x_zero',),
    'range_inf': S57 + ('inf',),
}
INF_AT = (1, 2, 3, 7)           # range_inf: g[INF_AT] = +Inf, column co* = 7
RANGE_FINITE = ('x_pow2', 'tiny', 'huge')
_CACHE = {}


def inputs(name):
    """-> (x [B,H,W,Cin], g [B,Ho,Wo,Cout]) fp32, seeded by the name; cached and never written to."""
    if name not in _CACHE:
        B, H, W, Cin, Cout, ldg, k, stride, kind = CASES[name]
        gen = torch.Generator().manual_seed(zlib.crc32(name.encode()))
        x = torch.randn(B, H, W, Cin, generator=gen)
        g = torch.randn(B, out_size(H, k, stride), out_size(W, k, stride), Cout, generator=gen)
        if kind == 'x_pow2':
            x = torch.sign(x) * torch.exp2(torch.rand(B, H, W, Cin, generator=gen) * 40 - 20)
        elif kind == 'tiny':
            x, g = x * 2.0 ** -60, g * 2.0 ** -60
        elif kind == 'huge':
            x, g = x * 2.0 ** 50, g * 2.0 ** 50
        elif kind == 'g_zero':
            g = torch.zeros_like(g)
        elif kind == 'x_zero':
            x = torch.zeros_like(x)
        elif kind == 'inf':
            g[INF_AT] = float('inf')
        _CACHE[name] = (x.contiguous(), g.contiguous())
    return _CACHE[name]


def references(name):
    """-> dict(dw64, db64, dw32, db32) by oracle(), cached."""
    key = ('ref', name)
    if key not in _CACHE:
        x, g = inputs(name)
        k, stride = CASES[name][6:8]
        dw64, db64 = oracle(x, g, k, stride, torch.float64)
        dw32, db32 = oracle(x, g, k, stride, torch.float32)
        _CACHE[key] = dict(dw64=dw64, db64=db64, dw32=dw32.double(), db32=db32.double())
    return _CACHE[key]


def bar(got32, want64):
    """The project's bar (tests/test_gpu_class_loss.py): max(4 * rel_err(CPU fp32, fp64), 8e-6)."""
    from gpu_utils import rel_err
    return max(4 * rel_err(got32, want64), EXACT_BAR)
