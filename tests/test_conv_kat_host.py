"""Known answers for the direct convolution engine's reference, on the CPU.

tests/conv_ref.py is pinned here before the GPU file (tests/test_gpu_conv_kat.py) trusts it: a 1x1 convolution is a matmul, a one-hot
input gives the flipped filter at every stride / pad, the stride-2 output geometry of the odd shipped sizes (275 -> 138, 69 -> 35,
35 -> 18) matches explicit tap loops, the row bands equal the full reference, and the bilinear residual equals F.interpolate at
every shipped (res_H -> Ho) pair.  Then the GPU file's bars are shown to discriminate: each wrong variant (the errors a kernel and a
restatement could share) misses the largest family bar by at least 10x on the GPU file's own inputs.
"""
import pytest
import torch
import torch.nn.functional as F

import conv_ref as R
import test_gpu_conv_kat as K

BAR = max(R.BARS.values())


def _rel(a, b):
    a, b = a.double(), b.double()
    if not torch.isfinite(a).all():
        return float('inf')
    return float((a - b).abs().max() / b.abs().max())


def _miss(wrong, right):
    e = _rel(wrong, right)
    assert e >= 10 * BAR, (e, BAR)
    return e


def _pick(pred):
    """The cheapest shipped launch satisfying pred(key, val, form) (so the CPU reference stays small)."""
    def cost(k):
        Ho, Wo = K.geometry(k)
        return k[0] * Ho * Wo * k[4] * k[11]
    return min(((cost(k), k, v, f) for k, _, v, f in K.LAUNCHES if pred(k, v, f)))[1:]


# ---- the reference is right ----------------------------------------------------------------------------------------------------
def test_1x1_is_a_matmul():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 40, 5, 7, generator=g, dtype=torch.float64)
    w = torch.randn(24, 40, 1, 1, generator=g, dtype=torch.float64)
    mm = (x.permute(0, 2, 3, 1).reshape(-1, 40) @ w.view(24, 40).t()).view(2, 5, 7, 24).permute(0, 3, 1, 2)
    assert _rel(R.conv_ref(x, w), mm) < 1e-15
    s2 = (x[:, :, ::2, ::2].permute(0, 2, 3, 1).reshape(-1, 40) @ w.view(24, 40).t()).view(2, 3, 4, 24).permute(0, 3, 1, 2)
    assert _rel(R.conv_ref(x, w, stride=2), s2) < 1e-15


@pytest.mark.parametrize('k,s,p', [(3, 1, 1), (3, 2, 1), (1, 2, 0), (7, 2, 3)])
def test_one_hot_gives_the_flipped_filter(k, s, p):
    """An impulse at (c, py, px) gives out[n, oy, ox] = w[n, c, py - oy s + p, px - ox s + p] (correlation): every output pixel
    whose window covers the impulse holds the filter tap it lands on, every other is zero."""
    H, W = 11, 9
    g = torch.Generator().manual_seed(k * 10 + s)
    w = torch.randn(5, 3, k, k, generator=g, dtype=torch.float64)
    Ho, Wo = R.out_size(H, k, s, p), R.out_size(W, k, s, p)
    for c, py, px in ((0, 0, 0), (1, H - 1, W - 1), (2, 5, 4), (0, 3, 8)):
        x = torch.zeros(1, 3, H, W, dtype=torch.float64)
        x[0, c, py, px] = 1.0
        y = R.conv_ref(x, w, stride=s, pad=p)
        exp = torch.zeros(5, Ho, Wo, dtype=torch.float64)
        for oy in range(Ho):
            for ox in range(Wo):
                ky, kx = py - oy * s + p, px - ox * s + p
                if 0 <= ky < k and 0 <= kx < k:
                    exp[:, oy, ox] = w[:, c, ky, kx]
        assert torch.equal(y[0], exp), (c, py, px)


def _loops(x, w, s, p):
    """Direct tap loops: y[b, n, oy, ox] = sum_{c, ky, kx} xpad[b, c, oy s + ky, ox s + kx] w[n, c, ky, kx]."""
    B, C, H, W = x.shape
    k = w.shape[2]
    xp = F.pad(x, (p, p, p, p))
    Ho, Wo = R.out_size(H, k, s, p), R.out_size(W, k, s, p)
    y = torch.zeros(B, w.shape[0], Ho, Wo, dtype=torch.float64)
    for ky in range(k):
        for kx in range(k):
            patch = xp[:, :, ky:ky + s * (Ho - 1) + 1:s, kx:kx + s * (Wo - 1) + 1:s]
            y += torch.einsum('bchw,nc->bnhw', patch, w[:, :, ky, kx])
    return y


@pytest.mark.parametrize('H,Ho', [(275, 138), (69, 35), (35, 18)])
def test_stride2_geometry_at_odd_sizes(H, Ho):
    for k, p in ((3, 1), (1, 0)):
        assert R.out_size(H, k, 2, p) == Ho
    g = torch.Generator().manual_seed(H)
    x = torch.randn(1, 2, H, H + 2, generator=g, dtype=torch.float64)
    for k, p in ((3, 1), (1, 0), (7, 3)):
        w = torch.randn(3, 2, k, k, generator=g, dtype=torch.float64)
        y = R.conv_ref(x, w, stride=2, pad=p)
        assert y.shape[2] == R.out_size(H, k, 2, p)
        assert _rel(y, _loops(x, w, 2, p)) < 1e-14


@pytest.mark.parametrize('k,s,p,rm', [(3, 1, 1, 0), (3, 2, 1, 0), (1, 1, 0, 1), (1, 1, 0, 2), (7, 2, 3, 0), (1, 2, 0, 0)])
def test_band_ref_equals_the_full_reference(k, s, p, rm):
    g = torch.Generator().manual_seed(k * 100 + s * 10 + rm)
    B, H, W = 2, 23, 9
    x = torch.randn(B, 8, H, W, generator=g)
    w, b = R.weights(12, 8, g, k)
    bn = R.batchnorm(12, g)
    Ho, Wo = R.out_size(H, k, s, p), R.out_size(W, k, s, p)
    res = torch.randn(B, 12, Ho, Wo, generator=g) if rm == 1 else torch.randn(B, 12, (Ho + 1) // 2, (Wo + 1) // 2, generator=g)
    for raa in (0, 1):
        full = R.conv_ref(x, w, b, bn, s, p, R.ACT_LEAKY01, res, rm, raa)
        bands = [(0, 2), (5, 7), (Ho - 2, Ho), (0, Ho)]
        for (r0, r1), piece in zip(bands, R.band_ref(x, w, b, bn, s, p, R.ACT_LEAKY01, bands, res, rm, raa)):
            assert _rel(piece, full[:, :, r0:r1]) < 1e-14, (r0, r1)


def test_epilogue_and_residual_forms():
    """BN folded, residual before (bottleneck) / after (darknet) the activation, against torch modules in fp64."""
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 8, 6, 5, generator=g)
    w, b = R.weights(12, 8, g, 1)
    bn = R.batchnorm(12, g)
    res = torch.randn(2, 12, 6, 5, generator=g).double()
    with torch.no_grad():
        z = bn.double()(F.conv2d(x.double(), w.double(), b.double()))
    assert _rel(R.conv_ref(x, w, b, bn, 1, 0, R.ACT_RELU, res, R.RES_ADD, 0), torch.relu(z + res)) < 1e-14
    assert _rel(R.conv_ref(x, w, b, bn, 1, 0, R.ACT_LEAKY01, res, R.RES_ADD, 1), F.leaky_relu(z, 0.1) + res) < 1e-14


LATERAL_PAIRS = sorted({(K.res_size(k), K.geometry(k)) for k, _, _, f in K.LAUNCHES if f == 'lateral'})


@pytest.mark.parametrize('pair', LATERAL_PAIRS, ids=['%dto%d' % (a[0], b[0]) for a, b in LATERAL_PAIRS])
def test_bilinear_equals_interpolate_at_every_shipped_pair(pair):
    """conv_ref's residual interpolation (fp32 source coordinates, as the kernel's bilin_coord forms them) against
    F.interpolate(align_corners=False) on fp32 data, and against the same interpolation with fp64 coordinates.  The fp32 choice is
    MEASURABLE: at 13 -> 25, 18 -> 35 and 35 -> 69 the fp32 weights differ from the fp64 ones by up to 1.7e-6 (the corners never
    differ; 22 -> 44, 25 -> 50, 44 -> 88 are exact), i.e. up to 1.7e-6 of the residual's range — a fifth of the fp32 bar.  The CPU
    F.interpolate lies within that same coordinate difference of the reference plus fp32 rounding."""
    (rh, rw), (Ho, Wo) = pair
    g = torch.Generator().manual_seed(rh * 100 + Ho)
    src = torch.randn(2, 16, rh, rw, generator=g)
    ours = R.bilinear_ref(src, Ho, Wo)
    a, b = R.bilin_coords(rh, Ho), R.bilin_coords(rh, Ho, fp64=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    d = float((a[2] - b[2]).abs().max())
    assert d <= 2e-6, d
    span = float(src.abs().max()) / float(ours.abs().max())
    e64 = _rel(R.bilinear_ref(src, Ho, Wo, fp64=True), ours)
    assert e64 <= 2 * d * span + 1e-15, (e64, d)
    if Ho in (25, 35, 69):
        assert e64 > 1e-7, e64                               # the fp32 coordinates measurably differ here
    else:
        assert e64 == 0.0, e64
    ti = F.interpolate(src, size=(Ho, Wo), mode='bilinear', align_corners=False)
    assert _rel(ti, ours) < 4e-7 + 2 * d * span, (_rel(ti, ours), d)


# ---- wrong variants are rejected ------------------------------------------------------------------------------------------------
def _case(pred):
    k, v, f = _pick(pred)
    case = K.build_case(k, f)
    assert case['bands'] == [(0, K.geometry(k)[0])], 'host cases are small enough for the whole map'
    return k, v, f, case


def _ref(case, **kw):
    c = dict(case)
    c.update(kw)
    act = c['act'] if c['segs'] is None else R.ACT_NONE
    return R.conv_ref(c['x'], c['w'], c['b'], c['bn'], c['stride'], c['pad'], act, c['res'], c['res_mode'], c['res_after_act'])


def test_transposed_or_flipped_filter_is_rejected():
    _, _, _, c = _case(lambda k, v, f: f == 'plain' and k[5] == 3 and k[7] == 1)
    right = c['pre'][0]
    _miss(_ref(c, w=c['w'].transpose(2, 3)), right)
    _miss(_ref(c, w=c['w'].flip(2, 3)), right)


def test_pad_off_by_one_at_stride_2_is_rejected():
    key, _, _, c = _case(lambda k, v, f: f == 'plain' and k[5] == 3 and k[7] == 2 and k[1] % 2 == 1)
    right = c['pre'][0]
    p = c['pad']
    for sh in (1, -1):                                    # window origin moved by one pixel: oy s - p + ky -> oy s - p - sh + ky
        xs = F.pad(c['x'].double(), (p + sh, p - sh, p + sh, p - sh))
        y = F.conv2d(xs, c['w'].double(), None, 2, 0)
        sc, shf = R.epilogue(c['b'], c['bn'], y.shape[1])
        _miss(R.act_ref(y * sc.view(1, -1, 1, 1) + shf.view(1, -1, 1, 1), c['act']), right)


@pytest.mark.parametrize('wrong', ['align_corners', 'no_clamp'])
def test_wrong_bilinear_residual_is_rejected(wrong):
    key, _, _, c = _case(lambda k, v, f: f == 'lateral')
    right = c['pre'][0]
    Ho, Wo = K.geometry(key)
    conv = _ref(c, res=None, res_mode=R.RES_NONE)
    kw = {'align_corners': True} if wrong == 'align_corners' else {'clamp': False}
    _miss(conv + R.bilinear_ref(c['res'], Ho, Wo, **kw), right)


def test_residual_order_swapped_is_rejected():
    for form in ('bottleneck', 'darknet'):
        _, _, _, c = _case(lambda k, v, f: f == form)
        right = c['pre'][0]
        _miss(_ref(c, res_after_act=1 - c['res_after_act']), right)


def test_bn_scale_on_the_residual_is_rejected():
    for form in ('bottleneck', 'darknet'):
        _, _, _, c = _case(lambda k, v, f: f == form)
        right = c['pre'][0]
        wrong = R.conv_ref(c['x'], c['w'], c['b'], c['bn'], c['stride'], c['pad'], c['act'], c['res'], c['res_mode'],
                           c['res_after_act'], bn_on_res=True)
        _miss(wrong, right)


def _heads(A):
    key, _, _, c = _case(lambda k, v, f: f == 'heads' and k[4] == 120 * A)
    return key, c


@pytest.mark.parametrize('A', [3, 9])
@pytest.mark.parametrize('wrong', ['tanh_on_loc', 'tanh_on_conf', 'boundary_plus_4', 'boundary_minus_4'])
def test_wrong_head_segments_are_rejected(A, wrong):
    """Errors are relative to the launch's pre-activation scale, as in the GPU file."""
    key, c = _heads(A)
    B, H, W = key[:3]
    pre = c['pre'][0]
    scale = float(pre.abs().max())
    sdef = [(n0, n1, a) for n0, n1, a, _, _ in c['segs']]
    rows, off = c['segs'][0][3], c['segs'][0][4]
    right = R.head_scatter_ref(pre, sdef, rows, off)
    if wrong.startswith('tanh'):
        j = 0 if wrong == 'tanh_on_loc' else 2
        bad = [(a, z, R.ACT_TANH if i == j else R.ACT_NONE) for i, (a, z, _) in enumerate(sdef)]
    else:
        d = 4 if wrong.endswith('plus_4') else -4
        bad = [(sdef[0][0], sdef[0][1] + d, sdef[0][2]), (sdef[1][0] + d, sdef[1][1] + d, sdef[1][2]), (sdef[2][0] + d, sdef[2][1], sdef[2][2])]
        bad = [(a, z, s) for a, z, s in bad]
    got = R.head_scatter_ref(pre, bad, rows, off)
    errs = []
    for q, r in zip(got, right):
        if q.shape != r.shape:
            errs.append(float('inf'))              # a shifted boundary changes the row width: the scatter is garbled
            continue
        lv, rv = q[:, off:off + H * W], r[:, off:off + H * W]
        errs.append(float((lv - rv).abs().max()) / scale)
    assert max(errs) >= 10 * BAR, errs
    if not wrong.startswith('tanh'):        # same width, shifted channels: the level rows themselves disagree
        q = R.head_scatter_ref(pre, [(a + d, z + d, s) if 0 <= a + d and z + d <= pre.shape[1] else (a, z, s)
                                     for a, z, s in sdef], rows, off)
        assert max(float((x_[:, off:off + H * W] - r[:, off:off + H * W]).abs().max()) / scale
                   for x_, r in zip(q, right)) >= 10 * BAR


def test_conf_padding_rows_written_are_rejected():
    """The rows before / after the level (other levels' priors) must keep their NaN: a launch that writes its conf rows one level
    too far, or that writes the rows past its level, leaves finite values there, which the GPU file's sentinel check sees."""
    key, c = _heads(3)
    B, H, W = key[:3]
    sdef = [(n0, n1, a) for n0, n1, a, _, _ in c['segs']]
    rows, off = c['segs'][0][3], c['segs'][0][4]
    right = R.head_scatter_ref(c['pre'][0], sdef, rows, off)
    conf = right[2]
    assert torch.isnan(conf[:, :off]).all() and torch.isnan(conf[:, off + H * W:]).all()
    late = R.head_scatter_ref(c['pre'][0], sdef, rows, off + 1)[2]
    assert torch.isfinite(late[:, off + H * W:]).any()
    early = R.head_scatter_ref(c['pre'][0], sdef, rows, off - 1)[2]
    assert torch.isfinite(early[:, :off]).any()


def _dense_case():
    """A batched launch checked on bands (several images, first / last rows of each)."""
    k, v, f = _pick(lambda k, v, f: f == 'plain' and k[0] >= 2 and k[5] == 3 and k[1] >= 18)
    return k, K.build_case(k, f)


def test_first_rows_from_the_previous_image_are_rejected():
    key, c = _dense_case()
    right = torch.cat(c['pre'], 2)
    xs = c['x'].clone()
    xs[1:, :, 0] = c['x'][:-1, :, 0]                      # image b's first input row read from image b - 1
    ys = torch.cat(R.band_ref(xs, c['w'], c['b'], c['bn'], c['stride'], c['pad'], c['act'], c['bands']), 2)
    _miss(ys, right)


def test_ragged_last_m_tile_dropped_is_rejected():
    key, c = _dense_case()
    pieces = [p.clone() for p in c['pre']]
    pieces[-1][-1, :, -1] = 0                             # the last image's last output row (the ragged last M tile): never written
    _miss(torch.cat(pieces, 2), torch.cat(c['pre'], 2))
    pieces[-1][-1, :, -1] = float('nan')                  # (written as NaN, as the GPU file's outputs start: non-finite)
    assert _rel(torch.cat(pieces, 2), torch.cat(c['pre'], 2)) == float('inf')


@pytest.mark.parametrize('how', ['dropped', 'twice'])
def test_split_k_range_dropped_or_counted_twice_is_rejected(how):
    """The cheapest shipped split-K launch: its last K range (of the packed k = (ky kw + kx) Cin + c; the shortest one on the
    pipelined / weight-stationary tiles) dropped or added twice, before the epilogue."""
    keys = sorted({(k, v, f) for k, _, v, f in K.LAUNCHES if v >> 8 > 1})
    k, v, f = min(keys, key=lambda t: t[0][0] * t[0][1] * t[0][2] * t[0][4] * t[0][11])
    c = K.build_case(k, f)
    S, nk = v >> 8, k[11] // 32
    per = -(-nk // S) if (v & 128) else nk // S
    k0 = 32 * per * (S - 1)                               # first packed k of the last range
    w = c['w']
    Co, Ci, kh, kw = w.shape
    wp = w.permute(0, 2, 3, 1).reshape(Co, kh * kw * Ci).clone()
    wp[:, :k0] = 0
    w_last = wp.view(Co, kh, kw, Ci).permute(0, 3, 1, 2)
    sc, _ = R.epilogue(c['b'], c['bn'], Co)
    part = R.conv_ref(c['x'], w_last, stride=c['stride'], pad=c['pad']) * sc.view(1, -1, 1, 1)
    full = _ref(c, act=R.ACT_NONE)                        # (dense: no residual on the split launches the table ships)
    assert c['res_mode'] == R.RES_NONE and float(part.abs().max()) > 0
    _miss(R.act_ref(full - part if how == 'dropped' else full + part, c['act']), c['pre'][0])


def test_channels_beyond_cin_read_are_rejected():
    """A kernel that reads the channels [Cin, ldx) of an ldx > Cin input: with the NaN the GPU file stores there the output is
    non-finite; with stale data (or reading [32, Cin + 32)) it is wrong by O(1)."""
    _, _, _, c = _case(lambda k, v, f: f == 'plain' and k[5] == 3 and k[7] == 1)
    right = c['pre'][0]
    x = c['x']
    pad = torch.full((x.shape[0], 32) + tuple(x.shape[2:]), float('nan'))
    xl = torch.cat([x, pad], 1)
    assert _rel(_ref(c, x=xl[:, 32:32 + x.shape[1]]), right) == float('inf')
    xl[:, x.shape[1]:] = torch.randn(pad.shape, generator=torch.Generator().manual_seed(4))
    _miss(_ref(c, x=xl[:, 32:32 + x.shape[1]]), right)
