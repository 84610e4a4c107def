"""The layout passes of csrc/layout.hip and the magnitude-bound slots of csrc/common.h, through the C ABI, BIT FOR BIT against the
fp32 restatements of tests/entry_ref.py (pinned on the CPU by tests/test_entry_kat_host.py); only ymi_conv2d_direct_nhwc_f32, a
summation, is held to a tolerance against float64.  Every output is prefilled with NaN between NaN guards and compared whole.

  * ymi_amax_f32: n = 4, 1024 and 4 * (256 * 2048 + 1) (the first size above the 2048-block grid: the last float4 is reached by
    the grid stride only); the maximum planted first, last, in the middle and at the head of the strided tail, as a negative value,
    a denormal and +inf; -0.0 gives +0; NaN elements are ignored; misaligned x and n % 4 != 0 are refused with YMI_ESHAPE; only
    floats [64 k], k < 16, of a slot are ever written (the others hold a sentinel); a launch only raises: larger values already in
    the slot, in whichever sub-slot, survive, lower ones in the sub-slot a launch targets are raised to the maximum;
  * the slot reader: one fp16x2 ymi_conv2d_nhwc_f32 launch (1x1, 64 -> 64, 16 pixels) gives identical bits whichever of the 16
    sub-slots holds the bound, and other bits with the bound 2^10 larger (the slot is read);
  * ymi_nchw_to_nhwc4[_amax]_f32 (C = 1 .. 4, pad channels +0.0, B = 3, 1x3x725x725 above the grid cap, the bound exact),
    ymi_nhwc_to_nchw_f32 (C = 1, 33, 40; HW = 1, 33), ymi_maxpool3x3s2_nhwc_f32 (H, W in {1, 2, odd, even}, C = 4 and 64,
    all-negative and -inf inputs, one case above the cap, wrong Ho / Wo refused), ymi_global_maxpool_nhwc_f32 (HW = 1, all-negative,
    C = 1 and 129), ymi_bilinear_nhwc_f32 (explicit 0.5 and derived scales, up / down / identity / 1x1 source, the relu flag with
    negative values and -0.0, C = 4 and 256, one case above the cap), ymi_bilinear_add_nhwc_f32 (y + lerp, the bound max|sum|,
    y_amax = NULL, C % 4 refused, one case above the cap, and lateral 1x1 conv + this pass == the conv with YMI_RES_BILINEAR on
    one forced tile);
  * ymi_conv2d_direct_nhwc_f32 against float64: the three conv_direct_small_k shapes and one general shape, each also with
    relu = 0, bias = NULL and a Cout that is no multiple of 4, and 8 -> 16 with x offset by 4 bytes (the general kernel) against the
    aligned launch.  Bar DIRECT_BAR of max(1, max|ref|): <= the earlier 2e-6 and <= 4x the largest measured on MI355X:

      measured max error, MI355X:  1 -> 8  1.33e-7   8 -> 16  2.65e-7   16 -> 32  5.65e-7   4 -> 12 (general)  2.22e-7
                                   8 -> 16 misaligned (general)  1.71e-7        largest 5.65e-7        DIRECT_BAR 2e-6

The whole file takes 3 s on an MI355X (72 tests; the slowest, 0.17 s, are the 8 MB amax tensors and the 34 MB max-pool).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import entry_ref as R

pytestmark = pytest.mark.gpu

from yolact_amd import _lib as L  # noqa: E402

DEV = 'cuda:0'
F = np.float32
GUARD = 64
ESHAPE = -2
SENTINEL = F(-123.0)
DIRECT_BAR = 2e-6
_MAX = {}


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    if _MAX:
        print('\ndirect conv KAT, max|y - ref| / max(1, max|ref|) (bar %.1e):' % DIRECT_BAR)
        for k, e in _MAX.items():
            print('    %-40s %.2e' % (k, e))
        print('    %-40s %.2e' % ('largest', max(_MAX.values())))


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Out:
    """n floats of NaN between two NaN guards; .ptr is 16-byte aligned."""

    def __init__(self, shape):
        self.shape, self.n = tuple(shape), int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * GUARD,), float('nan'), device=DEV)
        self.ptr = self.buf.data_ptr() + 4 * GUARD

    def get(self):
        torch.cuda.synchronize()
        assert bool(torch.isnan(self.buf[:GUARD]).all() and torch.isnan(self.buf[-GUARD:]).all()), 'a guard was written'
        return self.buf[GUARD:GUARD + self.n].view(self.shape).cpu().numpy()


def _slot(pre=None):
    """A slot whose floats [64 k] hold `pre` (default 0) and every other float the sentinel."""
    s = np.full((16, 64), SENTINEL, F)
    s[:, 0] = 0 if pre is None else pre
    return _d(s.reshape(-1))


def _slot_read(slot):
    """-> (the 16 sub-slot values, the reader's maximum over them); every other float must still hold the sentinel."""
    torch.cuda.synchronize()
    s = slot.cpu().numpy().reshape(16, 64)
    assert (R.bits(s[:, 1:]) == R.bits(np.array([SENTINEL]))[0]).all(), 'a float outside [64 k] of the slot was written'
    return s[:, 0].copy(), s[:, 0].max()


def _eq(got, want, what=''):
    if not R.same_bits(got, want):
        bad = R.bits(got) != R.bits(np.ascontiguousarray(want, F))
        i = tuple(int(v[0]) for v in np.nonzero(bad))
        pytest.fail('%s: %d of %d elements differ; first at %s: %r != %r' % (what, bad.sum(), bad.size, i, got[i], want[i]))


# ---- ymi_amax_f32 ----------------------------------------------------------------------------------------------------------------------

_BASE = {}


def _amax_base(n):
    if n not in _BASE:
        h = (np.random.default_rng(n).random(n, dtype=F) * F(2) - F(1)).astype(F)
        _BASE[n] = (h, _d(h))
    return _BASE[n]


def _amax_launch(xd, n, slot, ptr=None):
    return L.lib().ymi_amax_f32(xd.data_ptr() if ptr is None else ptr, n, slot.data_ptr(), L.stream_ptr())


@pytest.mark.parametrize('n', R.AMAX_SIZES)
def test_amax_planted_maxima(n):
    h, base = _amax_base(n)
    where = {'first': 0, 'last': n - 1, 'middle': (n // 2) | 1}
    if n > 4 * 256 * 2048:
        where['tail'] = 4 * 256 * 2048               # the first float only the grid stride reaches
        assert n // 4 > 256 * 2048
    for pos, i in where.items():
        for kind, v in (('plain', 9.25), ('negative', -7.5), ('inf', np.inf), ('denormal', 3e-44)):
            hx = h.copy() if kind != 'denormal' else np.where(np.arange(n) % 7 == 0, F(-1e-45), F(0)).astype(F)
            hx[i] = F(v)
            xd = _d(hx) if kind == 'denormal' else base.clone()
            xd[i] = float(F(v))
            assert R.same_bits(xd[i:i + 1], hx[i:i + 1])
            slot = _slot()
            L.check(_amax_launch(xd, n, slot), 'amax')
            sub, top = _slot_read(slot)
            want = R.amax(hx)
            assert want == np.abs(F(v)) and want > 0
            assert R.bits(np.array([top], F))[0] == R.bits(np.array([want], F))[0], (pos, kind, top, want)
            assert ((sub == 0) | (sub <= want)).all() and (sub >= 0).all()


def test_amax_negative_zero_and_nan():
    n = 1024
    slot = _slot()
    L.check(_amax_launch(_d(np.full(n, -0.0, F)), n, slot))
    sub, top = _slot_read(slot)
    assert (R.bits(sub) == 0).all()                                  # +0.0 in every sub-slot
    h = _amax_base(n)[0].copy()
    h[::3] = np.nan
    h[5] = F(-4.5)
    slot = _slot()
    L.check(_amax_launch(_d(h), n, slot))
    assert _slot_read(slot)[1] == F(4.5) == R.amax(h)
    slot = _slot()
    L.check(_amax_launch(_d(np.full(n, np.nan, F)), n, slot))
    assert (R.bits(_slot_read(slot)[0]) == 0).all()                  # all NaN: nothing to report


def test_amax_refuses_misaligned_and_ragged():
    xd = _d(np.ones(64, F))
    slot = _slot()
    assert _amax_launch(xd, 8, slot, ptr=xd.data_ptr() + 4) == ESHAPE
    assert _amax_launch(xd, 6, slot) == ESHAPE and _amax_launch(xd, 0, slot) == ESHAPE
    assert (_slot_read(slot)[0] == 0).all()


@pytest.mark.parametrize('n', R.AMAX_SIZES)
def test_amax_only_raises(n):
    h, xd = _amax_base(n)
    m = R.amax(h)
    assert 0 < m <= 1
    # larger values everywhere: nothing is lowered
    pre = (F(100) + np.arange(16)).astype(F)
    slot = _slot(pre)
    L.check(_amax_launch(xd, n, slot))
    assert R.same_bits(_slot_read(slot)[0], pre)
    # a larger value in every other sub-slot survives, whichever sub-slots the launch targets; the reader sees it
    pre = np.where(np.arange(16) % 2 == 0, F(100), F(0)).astype(F)
    slot = _slot(pre)
    L.check(_amax_launch(xd, n, slot))
    sub, top = _slot_read(slot)
    assert (sub[::2] == 100).all() and ((sub[1::2] >= 0) & (sub[1::2] <= m)).all() and top == 100
    # lower values: a targeted sub-slot is raised to the maximum of the waves that report to it (at most max|x|, and the reader's
    # maximum over the sub-slots IS max|x|), the others keep theirs
    pre = np.full(16, m / F(2), F)
    slot = _slot(pre)
    L.check(_amax_launch(xd, n, slot))
    sub, top = _slot_read(slot)
    assert ((sub >= pre) & (sub <= m)).all() and top == m
    # and from zero: the same maximum
    slot = _slot()
    L.check(_amax_launch(xd, n, slot))
    sub, top = _slot_read(slot)
    assert ((sub >= 0) & (sub <= m)).all() and top == m


# ---- the slot reader (ymi_amax_read) through one fp16x2 launch --------------------------------------------------------------------------

def test_conv_reads_the_maximum_over_the_sub_slots():
    from yolact_amd.engine import Packed
    g = torch.Generator().manual_seed(11)
    # mixed magnitudes: with a bound 2^10 too large the low pieces of the small values go subnormal and lose bits
    x = torch.randn(1, 4, 4, 64, generator=g) * torch.exp2(-torch.randint(0, 14, (1, 4, 4, 64), generator=g).float())
    w = torch.randn(64, 64, 1, 1, generator=g) / 8
    b = torch.randn(64, generator=g) * 0.1
    pk = Packed(w, b, None, 1, 0, None, DEV)
    hp, sc2, winv = pk.h2()
    xd = x.to(DEV)
    bound = x.abs().max().item()

    def launch(slot_values):
        out = Out((1, 4, 4, 64))
        sx, sy = _d(slot_values.reshape(-1)), torch.zeros(L.AMAX_SLOT_FLOATS, device=DEV)
        d = L.ConvDesc()
        d.x, d.w, d.bias = xd.data_ptr(), pk.w.data_ptr(), pk.bias.data_ptr()
        d.B, d.H, d.W, d.Cin, d.ldx, d.Ho, d.Wo, d.Cout = 1, 4, 4, 64, 64, 4, 4, 64
        d.kh, d.kw, d.stride, d.pad, d.Kpad, d.nseg, d.tile = 1, 1, 1, 0, pk.Kpad, 1, L.TILE_64x64 | L.TILE_H2
        d.seg[0] = L.ConvSeg(0, 64, L.ACT_NONE, 64, 16 * 64, out.ptr)
        d.w_h2, d.scale_h2, d.winv_h2 = hp.data_ptr(), sc2.data_ptr(), winv.data_ptr()
        d.x_amax, d.y_amax = sx.data_ptr(), sy.data_ptr()
        L.check(L.lib().ymi_conv2d_nhwc_f32(C.byref(d), L.stream_ptr()), 'conv')
        y = out.get()
        assert sy.max().item() == np.abs(y).max()
        return y

    def slot_with(k, v, rest=0.0):
        s = np.full((16, 64), rest, F)
        s[:, 1:] = 0
        s[k, 0] = v
        return s

    first = launch(slot_with(0, bound))
    ref = (x.double().view(16, 64) @ w.double().view(64, 64).t() + b.double()).view(1, 4, 4, 64)
    assert (torch.from_numpy(first).double() - ref).abs().max().item() < 2e-5 * ref.abs().max().item()
    for k in range(1, 16):
        _eq(launch(slot_with(k, bound)), first, 'bound in sub-slot %d' % k)
    _eq(launch(slot_with(9, bound, rest=bound / 4)), first, 'smaller values in the other sub-slots')
    for k in (0, 7, 15):
        assert not R.same_bits(launch(slot_with(k, bound * 1024.0)), first), 'the bound in sub-slot %d is not read' % k


# ---- layout changes ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', R.NHWC4_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_nchw_to_nhwc4(case):
    B, Cc, H, W = case
    x = R.layer_input('randn', case, seed=Cc + H)
    x[0, 0, 0, 0] = F(-37.5)                                          # the bound is a negative element's magnitude
    xd, want = _d(x), R.nchw_to_nhwc4(x)
    if B * H * W > R.GRID_CAP_THREADS:
        assert case == R.NHWC4_CASES[-1]
    out = Out((B, H, W, 4))
    L.check(L.lib().ymi_nchw_to_nhwc4_f32(xd.data_ptr(), out.ptr, B, Cc, H, W, L.stream_ptr()))
    y = out.get()
    _eq(y, want, 'nchw_to_nhwc4')
    assert (R.bits(y[..., Cc:]) == 0).all()                           # pad channels +0.0
    out2, slot = Out((B, H, W, 4)), _slot()
    L.check(L.lib().ymi_nchw_to_nhwc4_amax_f32(xd.data_ptr(), out2.ptr, B, Cc, H, W, slot.data_ptr(), L.stream_ptr()))
    _eq(out2.get(), want, 'nchw_to_nhwc4_amax')
    assert _slot_read(slot)[1] == R.amax(x) == F(37.5)


def test_nchw_to_nhwc4_cases_reach_the_grid_stride():
    assert max(c[0] * c[2] * c[3] for c in R.NHWC4_CASES) > R.GRID_CAP_THREADS
    assert max(c[0] * R.out_size(c[1], 3, 2, 1) * R.out_size(c[2], 3, 2, 1) * c[3] // 4 for c in R.MAXPOOL_CASES) > R.GRID_CAP_THREADS
    assert max(c[0] * c[4] * c[5] * c[3] // 4 for c in R.BILINEAR_CASES) > R.GRID_CAP_THREADS
    assert max(c[0] * c[4] * c[5] * c[3] // 4 for c in R.ADD_CASES) > R.GRID_CAP_THREADS


@pytest.mark.parametrize('case', R.NCHW_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_nhwc_to_nchw(case):
    B, Cc, H, W = case
    x = R.layer_input('randn', (B, H, W, Cc), seed=Cc * 3 + H)
    out = Out((B, Cc, H, W))
    L.check(L.lib().ymi_nhwc_to_nchw_f32(_d(x).data_ptr(), out.ptr, B, Cc, H, W, L.stream_ptr()))
    _eq(out.get(), R.nhwc_to_nchw(x), 'nhwc_to_nchw')


# ---- pooling -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', R.MAXPOOL_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_maxpool3x3s2(case):
    B, H, W, Cc, kind = case
    x = R.layer_input(kind, (B, H, W, Cc), seed=H * 31 + W)
    Ho, Wo = R.out_size(H, 3, 2, 1), R.out_size(W, 3, 2, 1)
    out = Out((B, Ho, Wo, Cc))
    L.check(L.lib().ymi_maxpool3x3s2_nhwc_f32(_d(x).data_ptr(), out.ptr, B, H, W, Cc, Ho, Wo, L.stream_ptr()))
    y = out.get()
    _eq(y, R.maxpool3x3s2(x), 'maxpool')
    if kind == 'neg':
        assert (y < 0).all()                                          # the padding is -inf, not 0
    if kind == 'ninf' and H > 2:
        assert np.isneginf(y).any()


def test_maxpool_refuses_wrong_output_sizes():
    x, out = _d(np.zeros((1, 9, 8, 4), F)), Out((1, 5, 5, 4))
    lib, s = L.lib(), L.stream_ptr()
    assert lib.ymi_maxpool3x3s2_nhwc_f32(x.data_ptr(), out.ptr, 1, 9, 8, 4, 4, 4, s) == ESHAPE      # Ho is 5
    assert lib.ymi_maxpool3x3s2_nhwc_f32(x.data_ptr(), out.ptr, 1, 9, 8, 4, 5, 5, s) == ESHAPE      # Wo is 4
    assert lib.ymi_maxpool3x3s2_nhwc_f32(x.data_ptr(), out.ptr, 1, 9, 8, 3, 5, 4, s) == ESHAPE      # C % 4
    assert np.isnan(out.get()).all()


@pytest.mark.parametrize('case', R.GLOBAL_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_global_maxpool(case):
    B, HW, Cc, kind = case
    x = R.layer_input(kind, (B, HW, Cc), seed=HW + Cc)
    out = Out((B, Cc))
    L.check(L.lib().ymi_global_maxpool_nhwc_f32(_d(x).data_ptr(), out.ptr, B, HW, Cc, L.stream_ptr()))
    y = out.get()
    _eq(y, R.global_max(x), 'global max')
    if kind == 'neg':
        assert (y < 0).all()


# ---- bilinear ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', R.BILINEAR_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_bilinear(case):
    B, Hi, Wi, Cc, Ho, Wo, scale, relu = case
    x = R.bilinear_input(case)
    out = Out((B, Ho, Wo, Cc))
    sc = C.c_float(scale if scale is not None else 0.0)
    L.check(L.lib().ymi_bilinear_nhwc_f32(_d(x).data_ptr(), out.ptr, B, Hi, Wi, Cc, Ho, Wo, sc, sc, relu, L.stream_ptr()))
    y = out.get()
    _eq(y, R.bilinear_nhwc(x, Ho, Wo, scale, scale, bool(relu)), 'bilinear')
    assert (R.bits(y[..., 0]) == R.bits(np.array([-0.0], F))[0]).all()          # -0.0 stays -0.0, with and without the relu flag
    assert (y < 0).any() != bool(relu)


def test_bilinear_refuses_ragged_channels():
    x, out = _d(np.zeros((1, 3, 3, 6), F)), Out((1, 6, 6, 6))
    z = C.c_float(0.0)
    assert L.lib().ymi_bilinear_nhwc_f32(x.data_ptr(), out.ptr, 1, 3, 3, 6, 6, 6, z, z, 0, L.stream_ptr()) == ESHAPE
    assert L.lib().ymi_bilinear_add_nhwc_f32(x.data_ptr(), out.ptr, 1, 3, 3, 6, 6, 6, None, L.stream_ptr()) == ESHAPE
    assert np.isnan(out.get()).all()


@pytest.mark.parametrize('case', R.ADD_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_bilinear_add(case):
    B, Hi, Wi, Cc, Ho, Wo = case
    x = R.layer_input('randn', (B, Hi, Wi, Cc), seed=1)
    y0 = R.layer_input('randn', (B, Ho, Wo, Cc), seed=2)
    want = R.bilinear_add(x, y0)
    xd = _d(x)
    for with_slot in (True, False):
        out, slot = Out((B, Ho, Wo, Cc)), _slot()
        out.buf[GUARD:GUARD + out.n] = _d(y0).reshape(-1)
        L.check(L.lib().ymi_bilinear_add_nhwc_f32(xd.data_ptr(), out.ptr, B, Hi, Wi, Cc, Ho, Wo, slot.data_ptr() if with_slot else None,
                                                  L.stream_ptr()))
        _eq(out.get(), want, 'bilinear_add')
        sub, top = _slot_read(slot)
        if with_slot:
            assert top == R.amax(want)
        else:
            assert (sub == 0).all()


def test_lateral_conv_then_bilinear_add_equals_the_fused_epilogue():
    """The kernel's comment: lateral-conv launch + this pass == the launch with YMI_RES_BILINEAR (same coordinates, same expression),
    with the tile forced so that both convolutions sum in the same order."""
    from gpu_utils import run_conv, nhwc
    g = torch.Generator().manual_seed(23)
    x = torch.randn(2, 64, 9, 13, generator=g)
    w = torch.randn(64, 64, 1, 1, generator=g) / 8
    b = torch.randn(64, generator=g) * 0.3
    prev = torch.randn(2, 64, 5, 7, generator=g)
    for tile in (L.TILE_64x64, L.TILE_64x64 | L.TILE_H2):
        fused = run_conv(x, w, b, None, 1, 0, res=prev, res_mode=L.RES_BILINEAR, tile=tile)
        plain = run_conv(x, w, b, None, 1, 0, tile=tile)
        out = Out((2, 9, 13, 64))
        out.buf[GUARD:GUARD + out.n] = nhwc(plain).to(DEV).reshape(-1)
        L.check(L.lib().ymi_bilinear_add_nhwc_f32(nhwc(prev).to(DEV).data_ptr(), out.ptr, 2, 5, 7, 64, 9, 13, None, L.stream_ptr()))
        _eq(out.get(), nhwc(fused).numpy(), 'conv + bilinear_add against RES_BILINEAR, tile %s' % L.TILE_NAMES[tile])


# ---- ymi_conv2d_direct_nhwc_f32 ----------------------------------------------------------------------------------------------------------

def _direct(x, w, b, stride, pad, relu, x_offset=0):
    """x [N,Cin,H,W], w [Cout,Cin,3,3] CPU -> [N,Ho,Wo,Cout] numpy; x_offset: floats by which the input pointer is shifted."""
    N, Cin, H, W = x.shape
    Cout = w.shape[0]
    Ho, Wo = R.out_size(H, 3, stride, pad), R.out_size(W, 3, stride, pad)
    xh = torch.cat([torch.zeros(x_offset), x.permute(0, 2, 3, 1).reshape(-1)]).to(DEV)
    wd = R.pack_direct(w).to(DEV)
    bd = b.to(DEV) if b is not None else None
    out = Out((N, Ho, Wo, Cout))
    L.check(L.lib().ymi_conv2d_direct_nhwc_f32(xh.data_ptr() + 4 * x_offset, wd.data_ptr(), bd.data_ptr() if b is not None else None,
                                               out.ptr, N, H, W, Cin, Ho, Wo, Cout, 3, 3, stride, pad, 1 if relu else 0, L.stream_ptr()))
    return out.get()


def _direct_inputs(case, cout=None):
    N, Cin, Cout, H, W, stride, pad = case
    Cout = cout or Cout
    g = torch.Generator().manual_seed(Cin * 100 + Cout)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (3.0 * Cin ** 0.5)
    b = torch.randn(Cout, generator=g)
    return x, w, b


def _direct_err(y, ref, key):
    assert np.isfinite(y).all()
    e = (torch.from_numpy(y).double() - ref).abs().max().item() / max(1.0, ref.abs().max().item())
    _MAX[key] = e
    return e


@pytest.mark.parametrize('variant', ('plain',) + R.DIRECT_VARIANTS)
@pytest.mark.parametrize('case', R.DIRECT_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_direct_conv_against_fp64(case, variant):
    N, Cin, Cout, H, W, stride, pad = case
    relu, cout = variant != 'norelu', Cout - 2 if variant == 'ragged_cout' else Cout
    x, w, b = _direct_inputs(case, cout)
    if variant == 'nobias':
        b = None
    ref = R.conv_direct_fp64(x, w, b, stride, pad, relu)
    y = _direct(x, w, b, stride, pad, relu)
    if not relu:
        assert (y < 0).any()
    e = _direct_err(y, ref, '%s %s' % ('x'.join(map(str, case)), variant))
    assert e < DIRECT_BAR, e


def test_direct_conv_misaligned_input_takes_the_general_kernel():
    case = R.DIRECT_CASES[1]
    assert case[1:3] == (8, 16)
    x, w, b = _direct_inputs(case)
    ref = R.conv_direct_fp64(x, w, b, case[5], case[6], True)
    ya = _direct(x, w, b, case[5], case[6], True)
    ym = _direct(x, w, b, case[5], case[6], True, x_offset=1)
    assert _direct_err(ym, ref, '8->16 x + 4 bytes') < DIRECT_BAR
    assert np.abs(ya.astype(np.float64) - ym).max() / max(1.0, ref.abs().max().item()) < DIRECT_BAR
