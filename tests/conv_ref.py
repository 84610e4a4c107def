"""Independent fp64 reference of the direct convolution engine (ymi_conv2d_nhwc_f32: csrc/conv_igemm.hip, and the kernels the
tuning table installs for ordinary convolutions: the pipelined gather-GEMM of csrc/dcn.hip, csrc/wstat.hip, csrc/patch.hip,
csrc/patch2.hip), built from torch alone: no engine code, no oracle.

  conv_ref        F.conv2d in float64 at any kh x kw / stride / pad, the BatchNorm folded in fp64 (wino_ref.epilogue, the fold
                  engine.Packed makes), then the residual and the activation in either order: RES_ADD with the residual before
                  (bottleneck: act(conv + res)) or after the activation (darknet unit: act(conv) + res), RES_BILINEAR (FPN lateral:
                  the coarser level upsampled to the output size and added)
  bilinear_ref    torch's align_corners=False upsampling with the SOURCE COORDINATES formed in fp32 exactly as the kernel's
                  bilin_coord / torch form them (scale = fp32(res_H) / fp32(Ho), src = max(scale (dst + 0.5) - 0.5, 0), clamped),
                  the interpolation itself in fp64 (dcn_ref forms its sample points the same way)
  band_ref        conv_ref on sets of output rows: each band reads only the input rows it needs (zero padding only at the true
                  image edges), so the shipped batch-16 138^2 and 550^2 launches stay cheap on the CPU
  launch_bands    the output rows a launch is checked on: the first and last rows of every image (M = B Ho Wo is flattened, so
                  those are where an M tile straddles two images; the last image's last row holds the ragged last M tile) and one
                  interior band; the whole map below FULL_FLOPS
  weights / head_weights / head_segments   filters as the GPU tests build them; the concatenated prediction-head filters
                  loc (4A) | coef (32A, tanh) | conf (84A, 3 zero rows per prior) and their segments, as engine.Plan builds them

The residual / activation forms and head scatter reuse wino_ref (act_ref, epilogue, head_scatter_ref).
"""
import numpy as np
import torch
import torch.nn.functional as F

from wino_ref import ACT_LEAKY01, ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH, act_ref, epilogue, head_scatter_ref  # noqa: F401

RES_NONE, RES_ADD, RES_BILINEAR = 0, 1, 2
_D = torch.float64
# GPU bars of tests/test_gpu_conv_kat.py, one per family (exact fp32 / bf16x3 / fp16x2): see that file's docstring
BARS = {'f32': 9e-6, 'x3': 1e-5, 'h2': 6e-6}
FULL_FLOPS = 2e9          # fp64 reference on the whole output below this many multiply-adds x 2, on row bands above


def out_size(n, k, s, p):
    return (n + 2 * p - k) // s + 1


# ---- bilinear residual ------------------------------------------------------------------------------------------------------------
def bilin_coords(src_n, dst_n, fp64=False, align_corners=False, clamp=True):
    """(i0, i1, l1) per destination index: torch's area_pixel_compute_source_index for align_corners=False, in fp32 (the
    kernel's bilin_coord).  fp64 / align_corners / clamp=False: the wrong variants of the host test."""
    dt = np.float64 if fp64 else np.float32
    dst = np.arange(dst_n).astype(dt)
    if align_corners:
        scale = dt(src_n - 1) / dt(dst_n - 1) if dst_n > 1 else dt(0)
        src = (scale * dst).astype(dt)
    else:
        scale = dt(src_n) / dt(dst_n)
        src = (scale * (dst + dt(0.5)) - dt(0.5)).astype(dt)
    if clamp:
        src = np.maximum(src, dt(0))
    i0 = np.minimum(np.trunc(src).astype(np.int64), src_n - 1)
    i0 = np.maximum(i0, 0)
    i1 = i0 + (i0 < src_n - 1)
    l1 = (src - i0.astype(dt)).astype(dt)
    return torch.from_numpy(i0), torch.from_numpy(i1), torch.from_numpy(l1.astype(np.float64))


def bilinear_ref(src, Ho, Wo, rows=None, **kw):
    """[B,C,h,w] -> [B,C,Ho,Wo] (or the output rows [r0, r1) only): bilinear with fp32 coordinates, fp64 interpolation."""
    s = src.double()
    y0, y1, ly = bilin_coords(src.shape[2], Ho, **kw)
    x0, x1, lx = bilin_coords(src.shape[3], Wo, **kw)
    if rows is not None:
        y0, y1, ly = y0[rows[0]:rows[1]], y1[rows[0]:rows[1]], ly[rows[0]:rows[1]]
    ly, lx = ly.view(1, 1, -1, 1), lx.view(1, 1, 1, -1)
    top = s[:, :, y0][:, :, :, x0] * (1 - lx) + s[:, :, y0][:, :, :, x1] * lx
    bot = s[:, :, y1][:, :, :, x0] * (1 - lx) + s[:, :, y1][:, :, :, x1] * lx
    return top * (1 - ly) + bot * ly


# ---- the convolution ----------------------------------------------------------------------------------------------------------------
def _finish(y, bias, bn, act, res, res_mode, res_after_act, Ho, rows, bn_on_res=False):
    sc, sh = epilogue(bias, bn, y.shape[1])
    sc, sh = sc.view(1, -1, 1, 1), sh.view(1, -1, 1, 1)
    r = None
    if res_mode == RES_ADD:
        r = res.double() if rows is None else res[:, :, rows[0]:rows[1]].double()
    elif res_mode == RES_BILINEAR:
        r = bilinear_ref(res, Ho, y.shape[3], rows)
    else:
        assert res_mode == RES_NONE, res_mode
    if r is None:
        return act_ref(y * sc + sh, act)
    if bn_on_res:                                                  # wrong variant: the BN scale also multiplies the residual
        return act_ref((y + r) * sc + sh, act) if not res_after_act else act_ref(y * sc + sh, act) + r * sc
    if res_after_act:
        return act_ref(y * sc + sh, act) + r
    return act_ref(y * sc + sh + r, act)


def conv_ref(x, w, bias=None, bn=None, stride=1, pad=0, act=ACT_NONE, res=None, res_mode=RES_NONE, res_after_act=0, **kw):
    """x [B,Cin,H,W], w [Cout,Cin,kh,kw] -> the fused convolution of ymi_conv_desc in fp64 [B,Cout,Ho,Wo]:
    act(scale * conv + shift + res) (res_after_act 0) or act(scale * conv + shift) + res (1), res = the residual (RES_ADD) or
    bilinear_ref(res, Ho, Wo) (RES_BILINEAR)."""
    y = F.conv2d(x.double(), w.double(), None, stride, pad)
    return _finish(y, bias, bn, act, res, res_mode, res_after_act, y.shape[2], None, **kw)


def band_ref(x, w, bias, bn, stride, pad, act, bands, res=None, res_mode=RES_NONE, res_after_act=0, **kw):
    """conv_ref restricted to output rows: bands = [(r0, r1), ...] half-open output row ranges.  Returns one [B,Cout,r1-r0,Wo]
    tensor per band; band k equals conv_ref(...)[:, :, r0:r1] (tests/test_conv_kat_host.py)."""
    H = x.shape[2]
    kh = w.shape[2]
    Ho = out_size(H, kh, stride, pad)
    out = []
    for r0, r1 in bands:
        assert 0 <= r0 < r1 <= Ho, (r0, r1, Ho)
        lo, hi = r0 * stride - pad, (r1 - 1) * stride - pad + kh          # input rows [lo, hi) of this band
        xs = x[:, :, max(lo, 0):min(hi, H)].double()
        xs = F.pad(xs, (0, 0, max(-lo, 0), max(hi - H, 0)))             # zero rows only at the true image edges
        y = F.conv2d(xs, w.double(), None, stride, (0, pad))
        assert y.shape[2] == r1 - r0
        out.append(_finish(y, bias, bn, act, res, res_mode, res_after_act, Ho, (r0, r1), **kw))
    return out


def launch_bands(B, Ho, Wo, Cout, Kpad, rows=2):
    """Output rows checked for a launch of M = B Ho Wo rows and K = Kpad: the whole map when 2 M Cout Kpad <= FULL_FLOPS or the
    map is short, else the first and last `rows` rows (of every image: the bands apply to the whole batch) and one interior band
    at 0.55 Ho, off any power-of-two row alignment."""
    if 2.0 * B * Ho * Wo * Cout * Kpad <= FULL_FLOPS or Ho <= 4 * rows + 2:
        return [(0, Ho)]
    mid = int(0.55 * Ho) | 1
    return sorted({(0, rows), (mid, mid + rows), (Ho - rows, Ho)})


# ---- filters as the tests build them ------------------------------------------------------------------------------------------------
def weights(Co, C, g, k=3):
    """He-scaled random filters [Co, C, k, k] and a small bias [Co]."""
    return torch.randn(Co, C, k, k, generator=g) / (k * k * C) ** 0.5, 0.1 * torch.randn(Co, generator=g)


def batchnorm(Co, g):
    import torch.nn as nn
    bn = nn.BatchNorm2d(Co).eval()
    with torch.no_grad():
        bn.weight.copy_(1 + 0.2 * torch.randn(Co, generator=g))
        bn.bias.copy_(0.2 * torch.randn(Co, generator=g))
        bn.running_mean.copy_(0.2 * torch.randn(Co, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(Co, generator=g))
    return bn


HEAD_D, HEAD_CLS, HEAD_CP = 32, 81, 84          # coefficients, classes, class row padded to a multiple of 4


def head_weights(A, C, g, k=3):
    """The concatenated head filters as engine.Plan builds them: loc (4A) | coef (32A) | conf (84A, 3 zero rows per prior)."""
    wl, bl = weights(4 * A, C, g, k)
    wm, bm = weights(HEAD_D * A, C, g, k)
    wc, bc = weights(HEAD_CLS * A, C, g, k)
    pad = HEAD_CP - HEAD_CLS
    wc = F.pad(wc.view(A, HEAD_CLS, C, k, k), (0, 0, 0, 0, 0, 0, 0, pad)).reshape(A * HEAD_CP, C, k, k)
    bc = F.pad(bc.view(A, HEAD_CLS), (0, pad)).reshape(A * HEAD_CP)
    return torch.cat([wl, wm, wc]), torch.cat([bl, bm, bc])


def head_segments(A):
    """[(n0, n1, act)] of a head launch with A priors per pixel: loc | coef (tanh) | conf."""
    n1, n2 = 4 * A, (4 + HEAD_D) * A
    return [(0, n1, ACT_NONE), (n1, n2, ACT_TANH), (n2, n2 + HEAD_CP * A, ACT_NONE)]


def head_priors(Co):
    A = Co // (4 + HEAD_D + HEAD_CP)
    assert A * (4 + HEAD_D + HEAD_CP) == Co, Co
    return A
