"""An independent fp64 reference for the DCNv2 forward (modulated deformable 3x3 convolution, one deformable group), built from
torch primitives only — no code of oracle/ and nothing of the original implementation — and closed-form known answers for it.

The operation (external/DCNv2/src/cuda/dcn_v2_im2col_cuda.cu:143-193 describes it; nothing of it is used here): for output pixel
(oy, ox) and tap k = i*3 + j the sample point is
    h = (oy*stride - pad + i) + offset[:, 2k],    w = (ox*stride - pad + j) + offset[:, 2k+1]
formed in fp32 (the kernels and the original add an int and a float in fp32), the sample is the zero-padded bilinear
interpolation of x at (h, w), times mask[:, k], and the output is  sum_k sum_c weight[o, c, i, j] * sample_k[c] + bias[o].

A zero-padded bilinear sample is exactly F.grid_sample(mode='bilinear', padding_mode='zeros', align_corners=False) at the
normalised point gx = (2w + 1)/W - 1, gy = (2h + 1)/H - 1; it is zero wherever h <= -1 or h >= H (every corner outside), so the
original's `-1 < h < H` gate is implied and needs no code of its own.

shifted_conv_ref gives the same operation in closed form when every tap has a CONSTANT offset: an integer offset is a
zero-filled shift of x, a fractional one is the bilinear combination of the four integer shifts around it — exact in fp64 when
the fractions are dyadic (halves, quarters, 2^-10), because then the weights are exact.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F


def out_hw(H, W, stride, pad):
    return (H + 2 * pad - 3) // stride + 1, (W + 2 * pad - 3) // stride + 1


def sample_points(H, W, offset, stride, pad):
    """fp32 sample coordinates (h, w), each [B, 9, Ho, Wo], of a 3x3 deformable conv with offset [B, 18, Ho, Wo]."""
    B, _, Ho, Wo = offset.shape
    off = offset.float()
    oy = (torch.arange(Ho) * stride - pad).float().view(1, Ho, 1)
    ox = (torch.arange(Wo) * stride - pad).float().view(1, 1, Wo)
    hs, ws = [], []
    for k in range(9):
        i, j = divmod(k, 3)
        hs.append((oy + i) + off[:, 2 * k])          # one fp32 rounding, as in the kernels (int + float in fp32)
        ws.append((ox + j) + off[:, 2 * k + 1])
    return torch.stack(hs, 1), torch.stack(ws, 1)


def fp32_point_offsets(offset, H, W, stride, pad):
    """fp64 offsets with which an implementation that forms h = base + offset in fp64 samples the same points as one that
    forms it in fp32 (sample_points): offset'_k = h32_k - base_k, exact in fp64."""
    B, _, Ho, Wo = offset.shape
    h32, w32 = sample_points(H, W, offset, stride, pad)
    oy = (torch.arange(Ho) * stride - pad).double().view(1, 1, Ho, 1)
    ox = (torch.arange(Wo) * stride - pad).double().view(1, 1, 1, Wo)
    ki = torch.arange(9).double().view(1, 9, 1, 1)
    dh, dw = h32.double() - (oy + torch.div(ki, 3, rounding_mode='floor')), w32.double() - (ox + ki % 3)
    return torch.stack([dh, dw], 2).reshape(B, 18, Ho, Wo)


def dcn_ref(x, offset, mask, weight, bias=None, stride=1, pad=1, *, padding_mode='zeros', align_corners=False, gate_min=None):
    """fp64 DCNv2 forward.  x [B,C,H,W]; offset [B,18,Ho,Wo] (ch 2k = dh_k, 2k+1 = dw_k); mask [B,9,Ho,Wo] (the modulation itself,
    already in [0, 1]); weight [Co,C,3,3]; bias [Co] or None.  Returns [B,Co,Ho,Wo] float64.

    The keyword arguments exist only to build deliberately wrong variants (tests/test_dcn_kat_host.py shows the known-answer
    tests reject them): `padding_mode` / `align_corners` of the grid sample (the point is still normalised for
    align_corners=False), and `gate_min`: zero every sample whose point has h < gate_min or w < gate_min (the correct operation
    has no such gate)."""
    B, C, H, W = x.shape
    Co = weight.shape[0]
    assert weight.shape[1:] == (C, 3, 3) and offset.shape[1] == 18 and mask.shape[1] == 9
    Ho, Wo = out_hw(H, W, stride, pad)
    assert offset.shape[2:] == (Ho, Wo) and mask.shape[2:] == (Ho, Wo)
    h32, w32 = sample_points(H, W, offset, stride, pad)
    h, w = h32.double(), w32.double()
    xd, wd, md = x.double(), weight.double(), mask.double()
    out = torch.zeros(B, Co, Ho, Wo, dtype=torch.float64)
    for k in range(9):
        i, j = divmod(k, 3)
        hk, wk = h[:, k], w[:, k]
        grid = torch.stack([(2 * wk + 1) / W - 1, (2 * hk + 1) / H - 1], -1)
        s = F.grid_sample(xd, grid, mode='bilinear', padding_mode=padding_mode, align_corners=align_corners)   # [B,C,Ho,Wo]
        s = s * md[:, k].unsqueeze(1)
        if gate_min is not None:
            s = s * ((hk >= gate_min) & (wk >= gate_min)).unsqueeze(1).to(s.dtype)
        out += torch.einsum('oc,bchw->bohw', wd[:, :, i, j], s)
    if bias is not None:
        out += bias.double().view(1, Co, 1, 1)
    return out


def _shift(xp, P, dh, dw, i, j, stride, pad, Ho, Wo):
    """Rows oy*stride - pad + i + dh (oy < Ho), columns likewise, of x zero-padded by P on every side (xp)."""
    r0, c0 = P - pad + i + dh, P - pad + j + dw
    return xp[:, :, r0:r0 + stride * (Ho - 1) + 1:stride, c0:c0 + stride * (Wo - 1) + 1:stride]


def shifted_conv_ref(x, taps, weight, bias=None, stride=1, pad=1, tap_mask=None):
    """Closed-form DCNv2 forward in fp64 for CONSTANT per-tap offsets: taps = 9 pairs (dh_k, dw_k), tap_mask = 9 modulation
    values (default 1).  Tap k contributes weight[:, :, i, j] applied to the bilinear combination of the integer shifts of x
    (zero fill) around (dh_k, dw_k)."""
    B, C, H, W = x.shape
    Co = weight.shape[0]
    Ho, Wo = out_hw(H, W, stride, pad)
    tap_mask = [1.0] * 9 if tap_mask is None else list(tap_mask)
    P = pad + 2 + max(int(math.ceil(abs(v))) for t in taps for v in t)
    xp = F.pad(x.double(), (P, P, P, P))
    wd = weight.double()
    out = torch.zeros(B, Co, Ho, Wo, dtype=torch.float64)
    for k, (dh, dw) in enumerate(taps):
        i, j = divmod(k, 3)
        hl, wl = math.floor(dh), math.floor(dw)
        fh, fw = dh - hl, dw - wl
        s = torch.zeros(B, C, Ho, Wo, dtype=torch.float64)
        for a, ca in ((0, 1 - fh), (1, fh)):
            for b, cb in ((0, 1 - fw), (1, fw)):
                if ca * cb != 0:
                    s += (ca * cb) * _shift(xp, P, hl + a, wl + b, i, j, stride, pad, Ho, Wo)
        out += tap_mask[k] * torch.einsum('oc,bchw->bohw', wd[:, :, i, j], s)
    if bias is not None:
        out += bias.double().view(1, Co, 1, 1)
    return out


def const_offmask(B, Ho, Wo, taps, tap_mask=None):
    """offset [B,18,Ho,Wo] and mask [B,9,Ho,Wo] (fp32) holding the constant per-tap values of shifted_conv_ref."""
    off = torch.tensor([v for t in taps for v in t], dtype=torch.float32).view(1, 18, 1, 1).expand(B, 18, Ho, Wo).contiguous()
    m = torch.tensor([1.0] * 9 if tap_mask is None else list(tap_mask), dtype=torch.float32)
    return off, m.view(1, 9, 1, 1).expand(B, 9, Ho, Wo).contiguous()


def integer_taps(H, W):
    """Nine distinct integer offsets (dh_k, dw_k) from {0, +-1, +-2, +-H, +-W}, dh_k != dw_k on every tap, no two taps alike:
    swapping dh / dw, flipping a sign or transposing the taps changes which pixel each tap reads."""
    return [(0, 1), (1, -2), (-1, 2), (2, 0), (-2, -1), (H, 1), (-1, -W), (2, W), (-H, -2)]


def fractional_taps():
    """Nine half- and quarter-integer offsets (exact dyadic bilinear weights), dh_k != dw_k, every quadrant."""
    return [(0.5, -0.25), (-0.5, 1.75), (1.25, 0.0), (-1.75, -0.5), (0.25, 2.5), (-2.25, 0.75), (1.5, -1.25), (0.75, 0.5),
            (-0.25, -2.75)]


EDGE_LO = (-1.0, -1.0 + 2.0 ** -10, -0.5, 0.0)       # sample coordinates at the low edge of an axis


def edge_hi(n):
    """Sample coordinates at the high edge of an axis of n pixels."""
    return (n - 1.0, n - 0.5, n - 2.0 ** -10, float(n))


def edge_taps(H, W, stride, pad, lo, which):
    """Constant per-tap offsets that put the sample coordinate of the FIRST (lo=True) or LAST output row and column exactly on
    the edge values EDGE_LO / edge_hi: tap k lands on value (k + which) % 4 in h and (k + which + 1) % 4 in w."""
    Ho, Wo = out_hw(H, W, stride, pad)
    taps = []
    for k in range(9):
        i, j = divmod(k, 3)
        th = (EDGE_LO if lo else edge_hi(H))[(k + which) % 4]
        tw = (EDGE_LO if lo else edge_hi(W))[(k + which + 1) % 4]
        oy, ox = (0, 0) if lo else (Ho - 1, Wo - 1)
        taps.append((th - (oy * stride - pad + i), tw - (ox * stride - pad + j)))
    return taps


def edge_offsets(B, H, W, stride, pad, gen, spread=1.0):
    """Per-pixel offsets [B,18,Ho,Wo] (fp32): N(0, spread^2) in the interior; on the first / last output rows the h coordinate
    of every tap is exactly one of EDGE_LO / edge_hi(H) and on the first / last columns the w coordinate one of EDGE_LO /
    edge_hi(W), chosen per (image, pixel, tap) so that every value occurs at every edge."""
    Ho, Wo = out_hw(H, W, stride, pad)
    off = torch.randn(B, 18, Ho, Wo, generator=gen) * spread
    for b in range(B):
        for k in range(9):
            i, j = divmod(k, 3)
            for ox in range(Wo):
                q = (b + k + ox) % 4
                off[b, 2 * k, 0, ox] = EDGE_LO[q] - (0 * stride - pad + i)
                off[b, 2 * k, Ho - 1, ox] = edge_hi(H)[q] - ((Ho - 1) * stride - pad + i)
            for oy in range(Ho):
                q = (b + k + oy + 1) % 4
                off[b, 2 * k + 1, oy, 0] = EDGE_LO[q] - (0 * stride - pad + j)
                off[b, 2 * k + 1, oy, Wo - 1] = edge_hi(W)[q] - ((Wo - 1) * stride - pad + j)
    return off
