"""numpy restatement of the reference's SSDAugmentation pixel pipeline (utils/augmentations.py:667-688), STEP BY STEP as the reference
runs it, not as csrc/augment.hip computes it: PhotometricDistort over the whole image, Expand into a really allocated canvas filled
with the mean, the crop as a slice, the mirror as a reversed view, a separable resize (horizontal pass, then vertical), the backbone
transform.  Test infrastructure.

cv2 is not installed: the OpenCV rules (float BGR <-> HSV, float INTER_LINEAR, the 8-bit INTER_LINEAR of the masks as the integer rule
of include/yolact_amd.h) are restated from OpenCV's documentation and are unpinned against OpenCV itself.  `dtype` selects the
arithmetic of the photometric chain, the resize and the normalisation: float64 is the reference the kernel is compared with, float32
its own rounding, whose distance from float64 sets the test's bound.  The sample coordinate and its fraction are cv2's float in both
(they are part of the rule, not of the rounding), and so are the parameters, which the kernel receives as float32.
"""
import numpy as np

EPS = float(np.finfo(np.float32).eps)          # FLT_EPSILON


def _f(x, dtype):
    """A parameter as the kernel receives it (float32), in the arithmetic's type."""
    return dtype(np.float32(x))


def bgr_to_hsv(img, dtype):
    b, g, r = img[..., 0], img[..., 1], img[..., 2]
    v = np.maximum(np.maximum(r, g), b)
    diff = v - np.minimum(np.minimum(r, g), b)
    s = diff / (np.abs(v) + dtype(EPS))
    k = dtype(60) / (diff + dtype(EPS))
    h = np.where(v == r, (g - b) * k, np.where(v == g, (b - r) * k + dtype(120), (r - g) * k + dtype(240)))
    h = np.where(h < 0, h + dtype(360), h)
    return np.stack([h, s, v], axis=-1).astype(dtype)


def hsv_to_bgr(img, dtype):
    h, s, v = img[..., 0], img[..., 1], img[..., 2]
    h = h * (dtype(6) / dtype(360))
    h = np.where(h < 0, h + dtype(6), np.where(h >= 6, h - dtype(6), h))
    sector = np.floor(h).astype(np.int64)
    f = h - sector.astype(dtype)
    bad = (sector < 0) | (sector >= 6)
    sector = np.where(bad, 0, sector)
    f = np.where(bad, dtype(0), f)
    one = dtype(1)
    tab = np.stack([v, v * (one - s), v * (one - s * f), v * (one - s * (one - f))], axis=-1)
    table = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])
    return np.take_along_axis(tab, table[sector], axis=-1).astype(dtype)


def photometric(img, p, dtype):
    """PhotometricDistort.__call__ with the draws of AugmentParams `p`; a stage that was not drawn does not run."""
    im = img.copy()
    if p.brightness is not None:
        im = im + _f(p.brightness, dtype)
    if p.contrast is not None and not p.contrast_last:
        im = im * _f(p.contrast, dtype)
    im = bgr_to_hsv(im, dtype)
    if p.saturation is not None:
        im[..., 1] = im[..., 1] * _f(p.saturation, dtype)
    if p.hue is not None:
        h = im[..., 0] + _f(p.hue, dtype)
        h = np.where(h > 360, h - dtype(360), h)
        im[..., 0] = np.where(h < 0, h + dtype(360), h)
    im = hsv_to_bgr(im, dtype)
    if p.contrast is not None and p.contrast_last:
        im = im * _f(p.contrast, dtype)
    return im.astype(dtype)


def resize_coords(n_out, n_in):
    """cv2.resize INTER_LINEAR: (first tap, second tap, float32 fraction) per output index."""
    f = ((np.arange(n_out, dtype=np.float64) + 0.5) * (n_in / n_out) - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    lo, hi = s < 0, s >= n_in - 1
    s[lo], f[lo] = 0, 0
    s[hi], f[hi] = n_in - 1, 0
    return s, np.minimum(s + 1, n_in - 1), f


def resize_linear(img, ow, oh, dtype):
    """[h,w,c] -> [oh,ow,c]: the horizontal pass over every source row, then the vertical pass, in `dtype`."""
    h, w = img.shape[:2]
    x0, x1, fx = resize_coords(ow, w)
    y0, y1, fy = resize_coords(oh, h)
    fx, fy = fx.astype(dtype), fy.astype(dtype)
    src = img.astype(dtype)
    rows = src[:, x0] * (dtype(1) - fx)[None, :, None] + src[:, x1] * fx[None, :, None]
    return (rows[y0] * (dtype(1) - fy)[:, None, None] + rows[y1] * fy[:, None, None]).astype(dtype)


def resize_mask_u8(mask, ow, oh):
    """[h,w] uint8 -> [oh,ow] uint8 by the integer rule: 11-bit coefficients, one rounding shift."""
    h, w = mask.shape
    x0, x1, fx = resize_coords(ow, w)
    y0, y1, fy = resize_coords(oh, h)
    ax1 = np.rint(fx * np.float32(2048)).astype(np.int64)
    ay1 = np.rint(fy * np.float32(2048)).astype(np.int64)
    ax0, ay0 = 2048 - ax1, 2048 - ay1
    m = mask.astype(np.int64)
    rows = m[:, x0] * ax0[None, :] + m[:, x1] * ax1[None, :]
    return ((rows[y0] * ay0[:, None] + rows[y1] * ay1[:, None] + (1 << 21)) >> 22).astype(np.uint8)


def _geometry(arr, p, fill):
    """Expand -> crop -> mirror on [h,w,...]: a canvas of p.canvas_h x p.canvas_w filled with `fill`, the source at the offset."""
    canvas = np.empty((p.canvas_h, p.canvas_w) + arr.shape[2:], dtype=arr.dtype)
    canvas[...] = fill
    canvas[p.off_y:p.off_y + p.height, p.off_x:p.off_x + p.width] = arr
    x0, y0, x1, y1 = p.crop
    out = canvas[y0:y1, x0:x1]
    return out[:, ::-1] if p.mirror else out


def augment_image(img, p, S, mean, std, mode, dtype=np.float64):
    """img [h,w,3] BGR uint8 / float -> [S,S,3] RGB, the reference's pipeline in `dtype`.  mode as ymi_fast_base_transform_f32."""
    im = img.astype(np.float32).astype(dtype)                       # ConvertFromInts
    if p.photometric:
        im = photometric(im, p, dtype)
    mean_t = np.array(mean, dtype=np.float32).astype(dtype)
    std_t = np.array(std, dtype=np.float32).astype(dtype)
    im = _geometry(im, p, mean_t)                                   # the canvas is filled with the mean, not distorted
    im = resize_linear(im, S, S, dtype)
    if mode == 0:
        im = (im - mean_t) / std_t
    elif mode == 1:
        im = im - mean_t
    elif mode == 2:
        im = im / dtype(255)
    return im[:, :, ::-1].astype(dtype)


def augment_masks(masks, p, S):
    """masks [n,h,w] uint8 -> [len(p.keep),S,S] uint8: the kept instances, in p.keep's order."""
    out = np.zeros((len(p.keep), S, S), dtype=np.uint8)
    for j, k in enumerate(p.keep):
        out[j] = resize_mask_u8(np.ascontiguousarray(_geometry(masks[int(k)], p, 0)), S, S)
    return out
