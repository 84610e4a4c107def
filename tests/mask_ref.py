"""Restatements of the mask assembly behind postprocess() (csrc/mask.hip, mask_upsample_bits_k of csrc/metrics.hip, csrc/upsample_math.h)
for tests/test_mask_kat_host.py and tests/test_gpu_mask_kat.py.

The upsample, the crop window, boxes_to_pixels and the bit packing are plain fp32 without contraction in the kernels, so numpy
fp32 restates them operation by operation (every intermediate below is a float32 array or scalar: numpy rounds after each
operation, as the device does) and the GPU tests compare BIT FOR BIT.  Only the logits (MFMA summation order, the device's expf)
are held to a tolerance, against the fp64 / fp32 torch statements at the bottom.
"""
import numpy as np
import torch

F = np.float32
ONE, HALF, ZERO = F(1), F(0.5), F(0)


# ---- csrc/upsample_math.h --------------------------------------------------------------------------------------------------------

def up_coord(n_out, n_in):
    """up_coord for dst = 0 .. n_out - 1 with the launcher's scale (float)n_in / (float)n_out -> (i0, i1 int64, l1 fp32)."""
    scale = F(n_in) / F(n_out)
    dst = np.arange(n_out, dtype=np.int32).astype(F)
    src = scale * (dst + HALF) - HALF
    src = np.where(src < ZERO, ZERO, src)
    i0 = np.minimum(src.astype(np.int32), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = src - i0.astype(F)
    assert src.dtype == F and l1.dtype == F
    return i0.astype(np.int64), i1.astype(np.int64), l1


def upsample_lerp2(lo, h, w):
    """mask_upsample_k / mask_upsample_band_k / mask_upsample_bits_k: four corners per pixel, then up_lerp2:
    (1 - ly) * ((1 - lx) * v00 + lx * v01) + ly * ((1 - lx) * v10 + lx * v11).  lo [N,ph,pw] fp32 -> [N,h,w] fp32."""
    lo = np.ascontiguousarray(lo, F)
    _, ph, pw = lo.shape
    y0, y1, ly = up_coord(h, ph)
    x0, x1, lx = up_coord(w, pw)
    ly, lx = ly[None, :, None], lx[None, None, :]
    r0, r1 = lo[:, y0], lo[:, y1]
    v00, v01, v10, v11 = r0[:, :, x0], r0[:, :, x1], r1[:, :, x0], r1[:, :, x1]
    out = (ONE - ly) * ((ONE - lx) * v00 + lx * v01) + ly * ((ONE - lx) * v10 + lx * v11)
    assert out.dtype == F
    return out


def upsample_rows(lo, h, w):
    """mask_upsample_rows_k's order: every source row interpolated along x once, omx * a + lx * b with omx = 1 - lx, then per output
    row oml * top + ly * bot with oml = 1 - ly.  The same operations on the same values as upsample_lerp2 (asserted on the CPU in
    tests/test_mask_kat_host.py), at a quarter of the gathers: the form the GPU tests use."""
    lo = np.ascontiguousarray(lo, F)
    _, ph, pw = lo.shape
    y0, y1, ly = up_coord(h, ph)
    x0, x1, lx = up_coord(w, pw)
    lx = lx[None, None, :]
    omx = ONE - lx
    hs = omx * lo[:, :, x0] + lx * lo[:, :, x1]                  # [N, ph, w]
    ly = ly[None, :, None]
    oml = ONE - ly
    out = oml * hs[:, y0] + ly * hs[:, y1]
    assert out.dtype == F
    return out


def binarise(soft, thresh):
    """thresh < 0: the soft values; else v > thresh ? 1 : 0."""
    return soft if thresh < 0 else (soft > F(thresh)).astype(F)


def pack_bits(hard):
    """[N, n] bool -> [N, ceil(n / 64)] uint64: bit i of word j is pixel 64 j + i, tail bits zero (ymi_mask_bits_f32 /
    ymi_mask_upsample_bits)."""
    hard = np.asarray(hard, bool)
    N, n = hard.shape
    W64 = (n + 63) // 64
    padded = np.zeros((N, W64 * 64), bool)
    padded[:, :n] = hard
    return np.packbits(padded.reshape(N, W64, 64), axis=2, bitorder='little').view('<u8').reshape(N, W64)


# ---- sanitize_coordinates (box_utils.py:327-346, cast=False) as lincomb_crop_k and boxes_to_pixels_k evaluate it -----------------

def _sanitize(lo_c, hi_c, size, padding):
    a, b = lo_c * F(size), hi_c * F(size)
    c1 = np.minimum(a, b)
    c2 = np.maximum(a, b)
    if padding:
        c1, c2 = c1 - F(padding), c2 + F(padding)
    c1 = np.where(c1 < ZERO, ZERO, c1)
    c2 = np.where(c2 > F(size), F(size), c2)
    assert c1.dtype == F and c2.dtype == F
    return c1, c2


def crop_window(box, ph, pw, crop=True):
    """lincomb_crop_k's window: box [N,4] fp32 relative -> bool [N,ph,pw]; padding 1; crop False = everything."""
    box = np.asarray(box, F)
    N = box.shape[0]
    if not crop:
        return np.ones((N, ph, pw), bool)
    x1, x2 = _sanitize(box[:, 0], box[:, 2], pw, 1)
    y1, y2 = _sanitize(box[:, 1], box[:, 3], ph, 1)
    fx = np.arange(pw, dtype=np.int32).astype(F)[None, None, :]
    fy = np.arange(ph, dtype=np.int32).astype(F)[None, :, None]
    x1, x2, y1, y2 = (v[:, None, None] for v in (x1, x2, y1, y2))
    return (fx >= x1) & (fx < x2) & (fy >= y1) & (fy < y2)


def boxes_to_pixels(box, w, h):
    """boxes_to_pixels_k: padding 0, then truncation -> int64 [N,4] (x1, y1, x2, y2)."""
    box = np.asarray(box, F)
    x1, x2 = _sanitize(box[:, 0], box[:, 2], w, 0)
    y1, y2 = _sanitize(box[:, 1], box[:, 3], h, 0)
    return np.stack([x1, y1, x2, y2], 1).astype(np.int64)


def hand_boxes(pw, ph):
    """The boxes a crop can get wrong: reversed corners, < 0, > 1, zero width / height, edges exactly at k / pw and k / ph, whole
    image, empty after clamping (both corners outside on the same side)."""
    k = max(1, pw // 3)
    m = max(1, ph // 2)
    rows = [
        (0.1, 0.2, 0.7, 0.9), (0.7, 0.9, 0.1, 0.2), (0.7, 0.2, 0.1, 0.9),          # plain, both reversed, x reversed
        (-0.3, -0.2, 0.4, 0.5), (0.5, 0.4, 1.3, 1.7), (-1.0, -2.0, 3.0, 2.0),        # < 0, > 1, both
        (0.4, 0.1, 0.4, 0.8), (0.2, 0.6, 0.9, 0.6), (0.5, 0.5, 0.5, 0.5),            # zero width, zero height, a point
        (k / pw, m / ph, (k + 1) / pw, (m + 1) / ph), ((k + 1) / pw, 0.0, k / pw, 1.0),   # edges at k / pw, k / ph
        (1 / pw, 1 / ph, (pw - 1) / pw, (ph - 1) / ph),
        (0.0, 0.0, 1.0, 1.0), (1.0, 1.0, 0.0, 0.0),                                  # whole image, reversed
        (-0.5, 0.2, -0.1, 0.8), (1.2, 0.2, 1.6, 0.8), (0.2, 1.5, 0.8, 1.1),          # outside on one side
    ]
    return np.array(rows, np.float64).astype(F)


def boxes_for(N, pw, ph, seed):
    """N boxes [N,4] fp32: the hand-made set first (its first N when N is smaller), then random ones, some of them with reversed
    corners and some reaching outside [0, 1]."""
    rng = np.random.default_rng(seed)
    rnd = (rng.random((N, 4)) * 1.4 - 0.2).astype(F)
    return np.ascontiguousarray(np.concatenate([hand_boxes(pw, ph), rnd])[:N], F)


# ---- logits ----------------------------------------------------------------------------------------------------------------------

def masks_lo_torch(proto, coef, dtype):
    """sigmoid(proto @ coef.T) in `dtype` -> [N,ph,pw] (output_utils.py:69-72 before the crop).  proto [ph,pw,D], coef [N,D] (torch)."""
    return torch.sigmoid(proto.to(dtype) @ coef.to(dtype).t()).permute(2, 0, 1).contiguous()


def logits64(proto, coef):
    return (proto.double() @ coef.double().t()).permute(2, 0, 1).contiguous()


# ---- inputs of the upsample tests ------------------------------------------------------------------------------------------------

UP_INPUTS = ('uniform', 'edges', 'ulp')


def up_input(kind, N, ph, pw, seed):
    """uniform: U[0,1).  edges: a {0,1} map of random rectangles (sharp edges: every interpolated value between two different
    pixels crosses the threshold somewhere).  ulp: 0.5 + k * 2^-24, k in -6 .. 6 (every value is within a few ulp of the threshold:
    a lerp rounded differently flips the decision)."""
    rng = np.random.default_rng(seed)
    if kind == 'uniform':
        return rng.random((N, ph, pw), dtype=F)
    if kind == 'edges':
        m = rng.random((N, ph, pw)) < 0.5
        m[:, ph // 3: ph // 3 + max(1, ph // 2), pw // 4: pw // 4 + max(1, pw // 2)] = (np.arange(N) % 2 == 0)[:, None, None]
        return m.astype(F)
    if kind == 'ulp':
        k = rng.integers(-6, 7, (N, ph, pw))
        v = (0.5 + k * 2.0 ** -24).astype(F)
        assert np.array_equal(v.astype(np.float64), 0.5 + k * 2.0 ** -24)          # representable
        return v
    raise ValueError(kind)
