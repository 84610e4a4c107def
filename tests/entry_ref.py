"""References for the code in front of and between the matrix kernels (csrc/stem.hip, csrc/layout.hip, csrc/preprocess.hip, the
magnitude-bound slots of csrc/common.h), for tests/test_entry_kat_host.py, tests/test_gpu_entry_kat.py and
tests/test_gpu_layout_kat.py.  numpy and torch only: no engine code.

  * stem_fp64: conv 7x7 / 2 / 3 -> folded eval BatchNorm -> ReLU -> max-pool 3x3 / 2 / 1 -> NHWC in float64, written out tap by tap
    (no torch.nn), with three deliberately wrong variants (`wrong=`) the GPU result must NOT agree with;
  * fp32 restatements, one numpy operation per device operation (every intermediate a float32 array: numpy rounds after each
    operation, as the device does without contraction), built on mask_ref.up_coord: the kernels are held to them BIT FOR BIT;
  * the case tables and their input builders, shared by the host file and the GPU files.
"""
import numpy as np
import torch

import mask_ref as MR

F = np.float32
ONE, HALF, ZERO = F(1), F(0.5), F(0)


def bits(a):
    """fp32 array (numpy or torch) -> its bit patterns (int32 numpy): -0.0 is not +0.0, NaN compares by payload."""
    if torch.is_tensor(a):
        a = a.detach().cpu().contiguous().numpy()
    a = np.ascontiguousarray(a)
    assert a.dtype == F, a.dtype
    return a.view(np.int32)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and bool(np.array_equal(a, b))


def ulp_distance(a, b):
    """Largest distance in units of the last place between two finite fp32 arrays, and how many elements differ."""
    def key(v):
        i = bits(v).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    d = np.abs(key(a) - key(b))
    return int(d.max()), int((d != 0).sum())


# ---- the stem oracle (csrc/stem.hip) -----------------------------------------------------------------------------------------------

WRONG = ('taps_transposed', 'stem_short', 'batch_stride')
BN_EPS = 1e-5
# The stem's bar (max|y - stem_fp64| / max|stem_fp64| per launch): see the table in tests/test_gpu_entry_kat.py.
STEM_BAR = 1e-6
SCALE_EXPONENTS = (-100, 100)


def out_size(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def stem_fp64(x, w, bn, wrong=None):
    """x [B,3,H,W], w [64,3,7,7], bn = (gamma, beta, running_mean, running_var) (torch, any float type) -> [B,Hp,Wp,64] float64.
    wrong: None, or one of WRONG: 'taps_transposed' ky and kx swapped; 'stem_short' the last stem row and column dropped before
    pooling (they become the pool's padding); 'batch_stride' image b read as image b - 1 for b > 0."""
    assert wrong is None or wrong in WRONG
    x, w = x.double(), w.double()
    gamma, beta, mean, var = (t.double() for t in bn)
    if wrong == 'taps_transposed':
        w = w.transpose(2, 3)
    if wrong == 'batch_stride' and x.shape[0] > 1:
        x = torch.cat([x[:1], x[:-1]])
    B, _, H, W = x.shape
    Hs, Ws = out_size(H, 7, 2, 3), out_size(W, 7, 2, 3)
    xp = torch.zeros(B, 3, H + 6, W + 6, dtype=torch.float64)
    xp[:, :, 3:3 + H, 3:3 + W] = x
    t = torch.zeros(B, 64, Hs, Ws, dtype=torch.float64)
    for ky in range(7):
        for kx in range(7):
            t += torch.einsum('oc,bchw->bohw', w[:, :, ky, kx], xp[:, :, ky:ky + 2 * Hs - 1:2, kx:kx + 2 * Ws - 1:2])
    alpha = gamma / torch.sqrt(var + BN_EPS)
    t = t * alpha.view(1, -1, 1, 1) + (beta - mean * alpha).view(1, -1, 1, 1)
    t = torch.clamp_min(t, 0.0)
    if wrong == 'stem_short':
        t = t[:, :, :Hs - 1, :Ws - 1]
    Hp, Wp = out_size(Hs, 3, 2, 1), out_size(Ws, 3, 2, 1)
    tp = torch.full((B, 64, 2 * Hp + 1, 2 * Wp + 1), -float('inf'), dtype=torch.float64)
    tp[:, :, 1:1 + t.shape[2], 1:1 + t.shape[3]] = t
    y = torch.full((B, 64, Hp, Wp), -float('inf'), dtype=torch.float64)
    for dy in range(3):
        for dx in range(3):
            y = torch.maximum(y, tp[:, :, dy:dy + 2 * Hp - 1:2, dx:dx + 2 * Wp - 1:2])
    return y.permute(0, 2, 3, 1).contiguous()


def stem_weights(seed=7):
    """The filters and BatchNorm statistics of tests/test_gpu_kernels.py's stem test."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(64, 3, 7, 7, generator=g) * 0.08
    gamma = torch.rand(64, generator=g) + 0.5
    beta = torch.randn(64, generator=g) * 0.2
    mean = torch.randn(64, generator=g) * 0.1
    var = torch.rand(64, generator=g) + 0.5
    return w, (gamma, beta, mean, var)


def folded_bias(bn):
    """fp32 folded shift as engine.Packed computes it: beta - mean * (gamma / sqrt(var + eps))."""
    gamma, beta, mean, var = (t.float() for t in bn)
    scale = gamma * (1.0 / torch.sqrt(var + BN_EPS))
    return beta - mean * scale


# The zero region of the 'zero_region' case: rows [11, 51) x columns [19, 59) of image 0 are zero; tile (1, 1)'s 23 x 31 patch
# (rows 11 .. 33, columns 19 .. 49) lies inside it, next to loud tiles (asserted from stem.hip's constants on the host).
ZERO_REGION = (11, 51, 19, 59)
CUS_DEFAULT = 256            # what the host file assumes for the persistent-loop case; the GPU file asks the device


def _ragged_shapes():
    """One shape per pair (Hp % 4, Wp % 6) in {1,2,3} x {1..5}: under 100 pixels a side, odd and even H and W."""
    out = []
    for rh in (1, 2, 3):
        for rw in (1, 2, 3, 4, 5):
            Hp, Wp = 4 * (1 + rw % 2) + rh, 6 * (1 + rh % 2) + rw
            H, W = 4 * (Hp - 1) + 1 + (rh + rw) % 4, 4 * (Wp - 1) + 1 + (rh + 2 * rw) % 4
            out.append((H, W))
    return out


RAGGED = _ragged_shapes()
# name -> (kind, B, H, W); B None = chosen from the CU count (persistent_B)
STEM_CASES = {'one_tile_7x7': ('plain', 1, 7, 7), 'batch3_7x7': ('plain', 3, 7, 7)}
for _H, _W in RAGGED:
    STEM_CASES['ragged_%dx%d' % (_H, _W)] = ('plain', 2, _H, _W)
STEM_CASES.update({
    'persistent_200x300': ('plain', None, 200, 300),
    'zero_image_between_loud': ('zero_image', 3, 45, 58),
    'zero_region_in_loud': ('zero_region', 1, 70, 90),
    'negative_bias': ('negbias', 2, 33, 47),
    'hot_patch_61x77': ('hot', 2, 61, 77),
    'scale_invariance': ('scale', 2, 37, 50),
})


def persistent_B(cus):
    """Smallest batch with ntiles >= 3 * CUs + 1 at 200 x 300 (169 tiles an image)."""
    return -(-(3 * cus + 1) // 169)


def stem_case(name, cus=CUS_DEFAULT):
    """-> dict(x [B,3,H,W] fp32, w, bn, kind).  Every image differs (one generator stream)."""
    kind, B, H, W = STEM_CASES[name]
    if B is None:
        B = persistent_B(cus)
    w, bn = stem_weights()
    g = torch.Generator().manual_seed(1000 + H * 7 + W)
    x = torch.randn(B, 3, H, W, generator=g) * 1.3
    if kind == 'zero_image':
        x *= 40.0
        x[1] = 0
    elif kind == 'zero_region':
        x *= 40.0
        r0, r1, c0, c1 = ZERO_REGION
        x[0, :, r0:r1, c0:c1] = 0
    elif kind == 'negbias':
        gamma, beta, mean, var = bn
        bn = (gamma, torch.full_like(beta, -1000.0), torch.zeros_like(mean), var)   # |conv| * alpha << 1000: every value < 0 before ReLU
    elif kind == 'hot':
        x[-1, :, H // 2:H // 2 + 4, W // 2:W // 2 + 4] *= 30.0
    elif kind == 'scale':
        gamma, beta, mean, var = bn
        bn = (gamma, torch.zeros_like(beta), torch.zeros_like(mean), var)          # folded bias 0: the result is linear in x
    return dict(x=x.contiguous(), w=w, bn=bn, kind=kind, name=name)


def zero_field(x):
    """[B,Hp,Wp] bool: pooled pixels whose receptive field (input rows 4 py - 5 .. 4 py + 5, the same columns, inside the image)
    holds only zeros: there the stem is ReLU(bias), whatever the filters."""
    a = x.abs().amax(1, keepdim=True)
    return torch.nn.functional.max_pool2d(a, 11, 4, 5)[:, 0] == 0


def wrong_applies(case, variant):
    """Whether a wrong= variant changes the oracle of this case at all: 'batch_stride' needs a second image, and with the negative
    bias every output is 0 whatever the taps, the edge or the image."""
    if case['kind'] == 'negbias':
        return False
    if variant == 'batch_stride':
        return case['x'].shape[0] > 1
    return True


def wrong_region(ref, variant):
    """The outputs a variant concerns, as an index into [B,Hp,Wp,64]: the last pooled row and column for 'stem_short', images
    b > 0 for 'batch_stride', everything for 'taps_transposed'."""
    m = torch.zeros(ref.shape[:3], dtype=torch.bool)
    if variant == 'stem_short':
        m[:, -1, :] = True
        m[:, :, -1] = True
    elif variant == 'batch_stride':
        m[1:] = True
    else:
        m[:] = True
    return m


# ---- fp32 restatements -------------------------------------------------------------------------------------------------------------

def up_coord_scale(n_out, n_in, scale):
    """upsample_math.h up_coord with an explicit fp32 scale (ymi_bilinear_nhwc_f32 accepts one); mask_ref.up_coord is this with
    scale = (float)n_in / (float)n_out (asserted on the host)."""
    scale = F(scale)
    dst = np.arange(n_out, dtype=np.int32).astype(F)
    src = scale * (dst + HALF) - HALF
    src = np.where(src < ZERO, ZERO, src)
    i0 = np.minimum(src.astype(np.int32), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = src - i0.astype(F)
    assert src.dtype == F and l1.dtype == F
    return i0.astype(np.int64), i1.astype(np.int64), l1


def _coords(n_out, n_in, scale):
    return MR.up_coord(n_out, n_in) if scale is None or scale <= 0 else up_coord_scale(n_out, n_in, scale)


def _lerp_nhwc(x, Ho, Wo, sh=None, sw=None):
    """(1 - ly) * ((1 - lx) * v00 + lx * v01) + ly * ((1 - lx) * v10 + lx * v11) on [B,H,W,C] fp32."""
    x = np.ascontiguousarray(x, F)
    _, Hi, Wi, _ = x.shape
    y0, y1, ly = _coords(Ho, Hi, sh)
    x0, x1, lx = _coords(Wo, Wi, sw)
    ly, lx = ly[None, :, None, None], lx[None, None, :, None]
    hy, hx = ONE - ly, ONE - lx
    r0, r1 = x[:, y0], x[:, y1]
    out = hy * (hx * r0[:, :, x0] + lx * r0[:, :, x1]) + ly * (hx * r1[:, :, x0] + lx * r1[:, :, x1])
    assert out.dtype == F
    return out


def bilinear_nhwc(x, Ho, Wo, sh=None, sw=None, relu=False):
    """bilinear_nhwc_k: the lerp, then (relu && v < 0) ? +0 : v  (-0.0 is not < 0: it stays -0.0)."""
    out = _lerp_nhwc(x, Ho, Wo, sh, sw)
    if relu:
        out = np.where(out < ZERO, ZERO, out)
    assert out.dtype == F
    return out


def bilinear_add(x, y):
    """bilinear_add_k: y + lerp(x -> y's size), derived scales."""
    y = np.ascontiguousarray(y, F)
    out = y + _lerp_nhwc(x, y.shape[1], y.shape[2])
    assert out.dtype == F
    return out


MEANS = (103.94, 116.78, 123.68)     # BGR order, applied before the channel swap
STD = (57.38, 57.12, 58.40)


def fast_base_transform(img, oh, ow, mode, nhwc4, means=MEANS, std=STD):
    """fast_base_transform_k: img [N,H,W,3] fp32 BGR -> lerp to (oh, ow) -> mode 0 (t - mean) / std, 1 t - mean, 2 t / 255, 3 t
    (means / std per BGR channel, as fp32) -> RGB; [N,3,oh,ow], or [N,oh,ow,4] with a +0.0 fourth channel."""
    t = _lerp_nhwc(img, oh, ow)
    m = np.array(means, np.float64).astype(F)[None, None, None, :]
    s = np.array(std, np.float64).astype(F)[None, None, None, :]
    if mode == 0:
        t = (t - m) / s
    elif mode == 1:
        t = t - m
    elif mode == 2:
        t = t / F(255)
    else:
        assert mode == 3
    assert t.dtype == F
    rgb = t[..., ::-1]
    if nhwc4:
        out = np.zeros(t.shape[:3] + (4,), F)
        out[..., :3] = rgb
        return out
    return np.ascontiguousarray(rgb.transpose(0, 3, 1, 2))


def maxpool3x3s2(x):
    """maxpool3x3s2_k: [B,H,W,C] -> [B,Ho,Wo,C], -inf padding, m = v > m ? v : m."""
    x = np.ascontiguousarray(x, F)
    B, H, W, C = x.shape
    Ho, Wo = out_size(H, 3, 2, 1), out_size(W, 3, 2, 1)
    xp = np.full((B, 2 * Ho + 1, 2 * Wo + 1, C), -np.inf, F)
    xp[:, 1:1 + H, 1:1 + W] = x
    out = np.full((B, Ho, Wo, C), -np.inf, F)
    for dy in range(3):
        for dx in range(3):
            v = xp[:, dy:dy + 2 * Ho - 1:2, dx:dx + 2 * Wo - 1:2]
            out = np.where(v > out, v, out)
    assert out.dtype == F
    return out


def nchw_to_nhwc4(x):
    """[B,C,H,W], C <= 4 -> [B,H,W,4], the pad channels +0.0."""
    x = np.ascontiguousarray(x, F)
    B, C, H, W = x.shape
    out = np.zeros((B, H, W, 4), F)
    out[..., :C] = x.transpose(0, 2, 3, 1)
    return out


def nhwc_to_nchw(x):
    return np.ascontiguousarray(np.ascontiguousarray(x, F).transpose(0, 3, 1, 2))


def global_max(x):
    """global_max_k: [B,HW,C] -> [B,C], m = v > m ? v : m from -inf."""
    x = np.ascontiguousarray(x, F)
    out = np.full((x.shape[0], x.shape[2]), -np.inf, F)
    for p in range(x.shape[1]):
        out = np.where(x[:, p] > out, x[:, p], out)
    return out


def amax(x):
    """The magnitude bound: max |x| from 0 with NaN elements ignored (fmaxf returns the other operand) -> fp32 scalar."""
    a = np.abs(np.ascontiguousarray(x, F)).reshape(-1)
    r = np.fmax.reduce(a, initial=ZERO)
    r = F(0) if np.isnan(r) else F(r)
    return r


def conv_direct_fp64(x, w, b, stride, pad, relu):
    """ymi_conv2d_direct_nhwc_f32's operation in float64: x [B,Cin,H,W], w [Cout,Cin,kh,kw], b [Cout] or None -> [B,Ho,Wo,Cout]."""
    y = torch.nn.functional.conv2d(x.double(), w.double(), None if b is None else b.double(), stride, pad)
    if relu:
        y = torch.relu(y)
    return y.permute(0, 2, 3, 1).contiguous()


def pack_direct(w):
    """[Cout,Cin,kh,kw] -> [kh*kw*Cin, ceil4(Cout)] fp32 with k = (ky*kw + kx)*Cin + c (the layout the direct kernels read)."""
    Cout, Cin, kh, kw = w.shape
    co4 = (Cout + 3) // 4 * 4
    wp = torch.zeros(kh * kw * Cin, co4)
    wp[:, :Cout] = w.permute(2, 3, 1, 0).reshape(kh * kw * Cin, Cout)
    return wp


# ---- case tables of the layout passes ------------------------------------------------------------------------------------------------

GRID_CAP_THREADS = 2048 * 256        # csrc/layout.hip grid_for: above this many work items a launch grid-strides

# ymi_bilinear_nhwc_f32: (B, Hi, Wi, C, Ho, Wo, explicit scale or None, relu)
BILINEAR_CASES = [
    (2, 13, 11, 4, 26, 22, 0.5, 1),          # x2, explicit scale
    (2, 13, 11, 256, 26, 22, 0.5, 1),        # protonet's form: 256 channels, explicit 0.5, relu
    (1, 9, 7, 256, 18, 14, 0.5, 0),
    (2, 13, 11, 4, 30, 17, None, 0),         # to-size, derived scales
    (1, 13, 11, 256, 30, 17, None, 1),
    (2, 21, 19, 4, 8, 5, None, 1),           # downsample
    (1, 21, 19, 256, 8, 5, None, 0),
    (2, 6, 5, 4, 6, 5, None, 0),             # identity
    (3, 1, 1, 4, 5, 7, None, 1),             # 1x1 source
    (1, 1, 1, 256, 2, 2, 0.5, 0),
    (1, 6, 5, 4, 12, 10, 0.5, 0),
    (1, 46, 46, 256, 92, 92, 0.5, 1),        # 541 696 work items: above the grid cap
]
# ymi_maxpool3x3s2_nhwc_f32: (B, H, W, C, kind)
MAXPOOL_CASES = [(2, 1, 1, 4, 'randn'), (2, 2, 2, 4, 'randn'), (1, 1, 2, 64, 'randn'), (2, 2, 1, 64, 'neg'), (3, 23, 31, 64, 'neg'),
                 (2, 24, 30, 4, 'randn'), (1, 23, 30, 4, 'ninf'), (2, 24, 31, 64, 'ninf'), (1, 365, 365, 64, 'randn')]
# ymi_bilinear_add_nhwc_f32: (B, Hi, Wi, C, Ho, Wo)
ADD_CASES = [(2, 18, 18, 256, 35, 35), (3, 5, 7, 8, 9, 13), (1, 1, 1, 4, 3, 2), (2, 9, 13, 8, 9, 13), (2, 35, 35, 256, 69, 69)]
# ymi_nchw_to_nhwc4[_amax]_f32: (B, C, H, W)
NHWC4_CASES = [(3, 1, 5, 7), (3, 2, 9, 4), (3, 3, 37, 29), (3, 4, 6, 11), (1, 3, 725, 725)]
# ymi_nhwc_to_nchw_f32: (B, C, H, W)
NCHW_CASES = [(3, 1, 1, 1), (3, 33, 1, 1), (3, 40, 3, 11), (3, 1, 3, 11), (3, 33, 3, 11), (2, 40, 21, 19)]
# ymi_global_maxpool_nhwc_f32: (B, HW, C, kind)
GLOBAL_CASES = [(3, 1, 1, 'randn'), (3, 1, 129, 'neg'), (3, 36, 129, 'randn'), (3, 35, 1, 'neg'), (1, 289, 128, 'randn')]
# ymi_fast_base_transform_f32: (N, H, W, oh, ow); every mode and both layouts run on each
FBT_CASES = [(3, 9, 13, 31, 40), (3, 40, 52, 17, 23), (3, 12, 15, 12, 15), (3, 1, 9, 6, 20), (3, 7, 1, 15, 4), (8, 16, 16, 550, 550)]
FBT_GRID_CAP = 8192 * 256
# ymi_conv2d_direct_nhwc_f32: (N, Cin, Cout, H, W, stride, pad); the first three take conv_direct_small_k, the fourth conv_direct_k
DIRECT_CASES = [(3, 1, 8, 21, 19, 2, 0), (2, 8, 16, 18, 15, 2, 0), (2, 16, 32, 11, 9, 2, 0), (2, 4, 12, 7, 9, 1, 1)]
DIRECT_VARIANTS = ('norelu', 'nobias', 'ragged_cout')
AMAX_SIZES = (4, 1024, 4 * (256 * 2048 + 1))


def layer_input(kind, shape, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape, dtype=F)
    if kind == 'neg':
        x = -np.abs(x) - ONE
    elif kind == 'ninf':
        x[rng.random(shape) < 0.3] = -np.inf
        x[:, :2, :2] = -np.inf                        # the first output's whole window: a result that is -inf
    assert x.dtype == F
    return x


def bilinear_input(case, seed=0):
    """randn with exact -0.0 and +0.0 planted (the relu flag must keep -0.0) and one constant-negative pixel block."""
    B, Hi, Wi, Cc = case[:4]
    rng = np.random.default_rng(100 + seed)
    x = rng.standard_normal((B, Hi, Wi, Cc), dtype=F)
    x[..., 0] = F(-0.0)
    x[..., 1] = ZERO
    return x


def fbt_input(case, seed=0):
    N, H, W = case[:3]
    rng = np.random.default_rng(200 + seed)
    return (rng.random((N, H, W, 3), dtype=F) * F(255)).astype(F)


def covered_forms():
    """The forms of the entry / layout ops this suite pins (tests/test_gpu_entry_kat.py's coverage check): kernel, channel count,
    explicit or derived scale, relu flag, whether a bound slot is handed in."""
    forms = {('stem', 64, None, None, True), ('stem', 64, None, None, False),
             ('input', 3, None, None, True), ('input', 3, None, None, False)}
    for c in BILINEAR_CASES:
        forms.add(('bilinear', c[3], c[6] is not None, bool(c[7]), False))
    for c in MAXPOOL_CASES:
        forms.add(('maxpool', c[3], None, None, False))
    for c in ADD_CASES:
        forms.add(('bilinear_add', c[3], None, None, True))
        forms.add(('bilinear_add', c[3], None, None, False))
    return forms
