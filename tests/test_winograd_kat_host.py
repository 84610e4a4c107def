"""Known answers for the Winograd path, on the CPU.

tests/wino_ref.py is pinned here before the GPU file (tests/test_gpu_winograd_kat.py) trusts it: its fp64 Winograd restatement
equals F.conv2d on ragged sizes, its row bands equal the full reference, its bilinear upsampling equals a hand-written one, and
max_gain_input reaches the stated gain on every interior tile.  Then the GPU file's bars are shown to discriminate: each wrong
variant of the reference (the errors a kernel and its restatement could share) misses the bar of that file by at least 10x on
that file's own inputs.  Last, a CPU emulation of the fp16x2 V planes shows that the shipped |B^T d B| <= gain max|d| bound
(4 / 100) keeps max_gain_input finite and fp32-class, while a bound 8x too small overflows on max_gain_input and still passes on
white noise — the suite needs the adversarial input to see it.
"""
import pytest
import torch
import torch.nn.functional as F

import wino_ref as R
import test_gpu_winograd_kat as K


def _rel(a, b):
    a, b = a.double(), b.double()
    if not torch.isfinite(a).all():
        return float('inf')
    return float((a - b).abs().max() / b.abs().max())


# ---- the reference is right ----------------------------------------------------------------------------------------------------
RAGGED = [(3, 5, 1, 1), (3, 5, 2, 3), (3, 6, 3, 11), (1, 4, 1, 23)]


@pytest.mark.parametrize('m', [2, 4])
@pytest.mark.parametrize('shape', RAGGED + [(3, 7, 'm+1', 11), (2, 8, 11, 'm+1'), (3, 4, 15, 7)])
def test_fp64_winograd_restatement_equals_conv2d(m, shape):
    B, C, H, W = (m + 1 if v == 'm+1' else v for v in shape)
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + W)
    x = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(6, C, 3, 3, generator=g, dtype=torch.float64)
    ref = F.conv2d(x, w, None, 1, 1)
    assert _rel(R.winograd_ref(x, w, m), ref) < 1e-12
    assert _rel(R.conv3x3_ref(x, w), ref) == 0.0
    e32 = _rel(R.winograd_ref(x, w, m, fp32=True), ref)      # what fp32 rounding of the algorithm alone costs
    assert 1e-9 < e32 < (2e-6 if m == 4 else 5e-7), e32


def test_epilogue_folds_batchnorm_and_activations():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 8, 5, 6, generator=g)
    w, b = K._weights(12, 8, g)
    bn = K._bn(12, g)
    conv = torch.nn.Conv2d(8, 12, 3, 1, 1).double()
    with torch.no_grad():
        conv.weight.copy_(w.double())
        conv.bias.copy_(b.double())
    bnd = bn.double()
    for act, fn in ((R.ACT_NONE, lambda t: t), (R.ACT_RELU, torch.relu), (R.ACT_LEAKY01, lambda t: F.leaky_relu(t, 0.1)),
                    (R.ACT_TANH, torch.tanh)):
        with torch.no_grad():
            exp = fn(bnd(conv(x.double())))
        assert _rel(R.conv3x3_ref(x, w, b, bn, act), exp) < 1e-14


@pytest.mark.parametrize('H', [1, 5, 11, 69])
def test_band_ref_equals_the_full_reference(H):
    g = torch.Generator().manual_seed(H)
    x = torch.randn(3, 16, H, 9, generator=g)
    w, b = K._weights(8, 16, g)
    bn = K._bn(8, g)
    full = R.conv3x3_ref(x, w, b, bn, R.ACT_RELU)
    bands = sorted({(0, min(H, 5)), (max(H - 5, 0), H), (H // 2, H // 2 + 1), (0, H)} | (set(K._bands(H, 4)) if H > 20 else set()))
    for (r0, r1), got in zip(bands, R.band_ref(x, w, b, bn, R.ACT_RELU, bands)):
        assert got.shape == full[:, :, r0:r1].shape
        assert (got - full[:, :, r0:r1]).abs().max().item() <= 1e-13 * full.abs().max().item(), (r0, r1)


def BT_rowsums(m):
    return [int(v) for v in R.BT[m].abs().sum(1)]


def _bilinear(lo, align_corners=False, clamp=True):
    """2x bilinear upsampling written out: source coordinate per output row / column, the two neighbours and their weights.
    align_corners=True / clamp=False are the wrong variants."""
    def coords(n):
        o = torch.arange(2 * n, dtype=torch.float64)
        src = o * (n - 1) / (2 * n - 1) if align_corners else 0.5 * (o + 0.5) - 0.5
        if clamp:
            src = src.clamp(min=0)
        i0 = src.floor().clamp(0, n - 1).long() if clamp else src.trunc().long()
        i1 = (i0 + 1).clamp(max=n - 1)
        return i0, i1, src - i0.double()
    y0, y1, ly = coords(lo.shape[2])
    x0, x1, lx = coords(lo.shape[3])
    v = lo.double()
    rows = v[:, :, y0] * (1 - ly).view(-1, 1) + v[:, :, y1] * ly.view(-1, 1)
    return rows[:, :, :, x0] * (1 - lx) + rows[:, :, :, x1] * lx


@pytest.mark.parametrize('hw', [(1, 1), (5, 7), (9, 4)])
def test_upsample_ref_equals_the_written_out_bilinear(hw):
    lo = torch.randn(2, 3, *hw, generator=torch.Generator().manual_seed(hw[0]))
    assert _rel(R.upsample2x_ref(lo), _bilinear(lo)) < 1e-15
    assert torch.equal(R.upsample2x_ref(lo, relu=True), torch.relu(R.upsample2x_ref(lo)))


@pytest.mark.parametrize('m,ijs', [(2, [(1, 1), (1, 2), (2, 1), (2, 2)]), (4, [(i, j) for i in (0, 1, 2, 5) for j in (0, 1, 2, 5)])])
def test_max_gain_input_reaches_the_gain_on_every_interior_tile(m, ijs):
    H, W = 4 * m + 3, 6 * m + 1
    for i, j in ijs:
        x = R.max_gain_input(2, 3, H, W, m, (i, j), A=0.75)
        assert torch.equal(x.abs(), torch.full_like(x, 0.75))
        V = R.input_transform(x, m)
        a = m + 2
        ty, tx = R.interior_tiles(H, W, m)
        assert len(ty) >= 2 and len(tx) >= 3
        comp = V[i * a + j][:, ty][:, :, tx]
        assert torch.equal(comp.abs(), torch.full_like(comp, R.GAIN[m] * 0.75)), (i, j)
        assert V.abs().max().item() == R.GAIN[m] * 0.75                    # ... and nothing anywhere exceeds the bound
    if m == 2:
        with pytest.raises(AssertionError):                                # rows 0 / 3 of B^T: no tile-consistent pattern
            R.max_gain_input(1, 1, H, W, m, (0, 0))
    else:
        assert BT_rowsums(m) == [10, 10, 10, 6, 6, 10]


# ---- the GPU file's bars discriminate ------------------------------------------------------------------------------------------
def _edge_case(H, W, m=4):
    """The input of test_winograd_edge_geometries at (H, W)."""
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(3, 64, H, W, generator=g)
    w, b = K._weights(44, 64, g)
    return x, w, b


def _miss(wrong, right, m, family='f32'):
    bar = min(K.BARS[m, f] for f in ('f32', 'x3', 'h2')) if family is None else K.BARS[m, family]
    e = _rel(wrong, right)
    assert e >= 10 * bar, (e, bar)
    return e


@pytest.mark.parametrize('m', [2, 4])
def test_flipped_filter_is_rejected(m):
    x, w, b = _edge_case(11, 15)
    right = R.conv3x3_ref(x, w, b, None, R.ACT_LEAKY01)
    _miss(R.conv3x3_ref(x, w.flip(2, 3), b, None, R.ACT_LEAKY01), right, m, None)


@pytest.mark.parametrize('m', [2, 4])
def test_ragged_last_tile_dropped_or_shifted_is_rejected(m):
    H, W = 4 * 2 + 3, 4 * 3 + 3                     # both ragged for m = 2 and 4
    x, w, b = _edge_case(H, W, m)
    right = R.conv3x3_ref(x, w, b, None, R.ACT_LEAKY01)
    r0, c0 = (H // m) * m, (W // m) * m             # first row / column of the last (partial) tile
    assert r0 < H and c0 < W
    for dim, k0 in ((2, r0), (3, c0)):
        dropped = right.clone()
        dropped.narrow(dim, k0, right.shape[dim] - k0).zero_()
        _miss(dropped, right, m, None)
        shifted = right.clone()
        n = right.shape[dim] - k0
        shifted.narrow(dim, k0, n).copy_(right.narrow(dim, k0 - 1, n))
        _miss(shifted, right, m, None)


@pytest.mark.parametrize('m', [2, 4])
def test_padding_from_the_neighbouring_image_is_rejected(m):
    x, w, b = _edge_case(11, 15, m)
    right = R.conv3x3_ref(x, w, b, None, R.ACT_LEAKY01)
    xd = x.double()
    top = torch.cat([torch.zeros_like(xd[:1, :, -1:]), xd[:-1, :, -1:]])      # image b's row -1 read from image b - 1
    bot = torch.cat([xd[1:, :, :1], torch.zeros_like(xd[:1, :, :1])])        # row H from image b + 1
    xp = torch.cat([top, xd, bot], 2)
    wrong = R.act_ref(F.conv2d(xp, w.double(), b.double(), 1, (0, 1)), R.ACT_LEAKY01)
    _miss(wrong, right, m, None)


@pytest.mark.parametrize('m', [2, 4])
def test_every_component_taken_from_its_neighbour_is_rejected(m):
    x, w, b = _edge_case(11, 15, m)
    right = R.conv3x3_ref(x, w)
    assert _rel(R.winograd_ref(x, w, m), right) < 1e-12
    for e in range((m + 2) ** 2):
        _miss(R.winograd_ref(x, w, m, swap=e), right, m, None)


@pytest.mark.parametrize('wrong', ['align_corners', 'no_clamp'])
def test_wrong_upsampling_is_rejected(wrong):
    key = K.FUSED_SMALL[0][0]
    assert key[1] == 10
    w, b, lo, xin, _ = K.fused_case(key, 'up', K.fused_seed(key))
    assert torch.equal(xin, R.upsample2x_ref(lo, relu=True))
    right = R.conv3x3_ref(xin, w, b, None, R.ACT_RELU)
    up = torch.relu(_bilinear(lo, align_corners=True) if wrong == 'align_corners' else _bilinear(lo, clamp=False))
    _miss(R.conv3x3_ref(up, w, b, None, R.ACT_RELU), right, 4, None)


@pytest.mark.parametrize('wrong', ['act2_before_bias', 'no_act_on_3x3'])
def test_wrong_projection_is_rejected(wrong):
    key = K.FUSED_SMALL[0][0]
    w, b, lo, xin, (pw, pb, act2) = K.fused_case(key, 'up+proj', K.fused_seed(key))
    y3 = R.conv3x3_ref(xin, w, b, None, R.ACT_RELU)
    right = R.proj_ref(y3, pw, pb, R.ACT_RELU)
    if wrong == 'act2_before_bias':
        bad = torch.relu(R.proj_ref(y3, pw)) + pb.double().view(1, -1, 1, 1)
    else:
        bad = R.proj_ref(R.conv3x3_ref(xin, w, b), pw, pb, R.ACT_RELU)
    _miss(bad, right, 4, None)


@pytest.mark.parametrize('wrong', ['coef_without_tanh', 'offset_off_by_one_prior'])
def test_wrong_head_scatter_is_rejected(wrong):
    key = next(k for k, _, _, _, _ in K.SHIPPED if k[6] == 3 and k[1] == 5)
    B, H, W, C, Co = key[:5]
    g = torch.Generator().manual_seed(K.shipped_seed(key))
    x = torch.randn(B, C, H, W, generator=g)
    w, b, sdef, rows, off = K.head_case(key, g)
    pre = R.conv3x3_ref(x, w, b)
    right = R.head_scatter_ref(pre, sdef, rows, off)
    if wrong == 'coef_without_tanh':
        bad = R.head_scatter_ref(pre, [(a, z, R.ACT_NONE) for a, z, _ in sdef], rows, off)
        errs = [_rel(q[:, off:off + H * W], r[:, off:off + H * W]) for q, r in zip(bad, right)]
        assert errs[0] == errs[2] == 0 and errs[1] >= 10 * K.BARS[2, 'f32'], errs
    else:
        A = Co // (4 + K.HEAD_D + K.HEAD_CP)
        for (a, z, _), r in zip(sdef, right):
            k = (z - a) // A                          # floats per prior of this segment
            bad = r.reshape(B, -1).roll(k, 1).view_as(r)
            lvl = bad[:, off:off + H * W]
            # the GPU file checks the level rows against fp64 AND that the rows before / after the level keep their NaN
            assert not torch.isfinite(lvl).all() or _rel(lvl, r[:, off:off + H * W]) >= 10 * K.BARS[2, 'f32']
            assert torch.isfinite(bad[:, off + H * W:]).any()


# ---- the fp16x2 V bound needs the adversarial input -----------------------------------------------------------------------------
GAIN_CASES = [(2, (1, 2)), (4, (0, 5)), (4, (5, 5))]


def _gain_inputs(m, ij, A=0.75):
    H, W = 4 * m + 3, 6 * m + 1
    x = R.max_gain_input(2, 64, H, W, m, ij, A=A, seed=ij[0] * 6 + ij[1])
    g = torch.Generator().manual_seed(11)
    w, _ = K._weights(132, 64, g)
    noise = torch.randn(2, 64, H, W, generator=torch.Generator().manual_seed(3)).double()
    return x, noise * (A / noise.abs().max()), w                 # white noise with the same max|x| = A


@pytest.mark.parametrize('m,ij', GAIN_CASES)
def test_shipped_gain_bound_is_finite_and_fp32_class_on_max_gain_input(m, ij):
    x, _, w = _gain_inputs(m, ij)
    ref = R.conv3x3_ref(x, w)
    y, finite = R.winograd_h2_emul(x, w, m, R.GAIN[m])
    assert finite
    bar, e32 = K.max_gain_bar(x, w, m, K.L.TILE_H2)
    e = _rel(y, ref)
    print('F%d %s: fp16x2 emulation %.2e, fp32 emulation %.2e, GPU bar %.1e' % (m, ij, e, e32, bar))
    assert e < bar and e < 4 * e32 + 1e-7


@pytest.mark.parametrize('A', [0.75, 1.0, 0.5001])
@pytest.mark.parametrize('m,ij', GAIN_CASES)
def test_too_small_gain_bound_overflows_only_on_max_gain_input(m, ij, A):
    """gain / 8 maps max|x| * gain / 8 into [2^13, 2^14): the true V maximum gain * max|x| lands at or above 2^16 -> inf in fp16,
    for every max|x|.  White noise with the same max|x| never gets near the bound, stays finite and passes the GPU file's bar."""
    x, noise, w = _gain_inputs(m, ij, A)
    _, finite = R.winograd_h2_emul(x, w, m, R.GAIN[m] / 8)
    assert not finite
    yn, finite_n = R.winograd_h2_emul(noise, w, m, R.GAIN[m] / 8)
    assert finite_n
    assert _rel(yn, R.conv3x3_ref(noise, w)) < K.BARS[m, 'h2']
