"""The Winograd path (ymi_conv3x3_winograd_f32: csrc/winograd.hip, csrc/wgemm.hip, the grouped GEMM of csrc/conv_igemm.hip)
against the independent fp64 reference of tests/wino_ref.py (torch only: no engine code, no oracle).

  * every wino(...) launch of yolact_amd/tune/gfx950.json, read from the table at test time and rebuilt as engine.Plan builds it
    (_wino_op, _tune_winograd): its exact (B, H, W, C, Cout, act, nseg), its m, its GEMM tile (value & 255), V planes
    (WINO_PLANES) and precision (plain / x3 / h2).  nseg = 3: the prediction heads scattered into level-concatenated loc / coef
    (tanh) / conf tensors at a non-zero prior offset, class rows padded 81 -> 84; nseg = 2: the merged head0.up0 + proto.0 launch,
    its second half 2^10 louder; nseg = 0: dense with a folded BatchNorm.  Small launches are compared on the whole tensor, large
    ones on row bands (first / last 2m + 1 rows, one tile-aligned and one misaligned interior band; every column, image and
    channel).  The reported bound slots must equal max|y| of the launch's own output, and a second launch must be bit-identical;
  * the fused forms the plan installs on protonet's last 3x3: x_up (2x bilinear + ReLU read from the half-size tensor), proj (the
    1x1 256 -> 32 + ReLU inside the output transform) and both, at the shipped 69^2 -> 138^2 and 88^2 -> 176^2 shapes with every
    tile the table ships for them, and at small odd low-resolution sizes;
  * a coverage check: every Winograd launch of the batch-8 timed plan of configs[1] is one of this file's parametrisations;
  * edges: H, W in {1, 2, 3, m + 1, 4k + 3}, a zero image between two loud ones, one-hot inputs, max_gain_input on every fp16x2
    family, a 2^10 hot patch.

Bars (rel_err = max|y - ref| / max|ref|; for the heads max|y - ref| of each segment over max|conv + bias| of the launch, since
tanh compresses the coefficients' scale but not their error), one per (m, family): exact fp32 tiles, bf16x3 (| YMI_TILE_X3),
fp16x2 (| YMI_TILE_H2, with or without V planes, and the persistent wg128x256 GEMM).  Each is <= 4x the largest error this file
measured on MI355X and never above the earlier 2e-5 (F(2x2)) / 5e-5 (F(4x4)); the maxima are printed at the end of the module.

  measured max rel_err   exact fp32   bf16x3    fp16x2      bar: exact fp32   bf16x3   fp16x2
  F(2x2)                 1.37e-6      9.4e-7    5.8e-7           5e-6         3.5e-6   2.2e-6
  F(4x4)                 1.68e-5      1.70e-5   1.10e-5          5e-5         5e-5     4e-5

F(4x4) is an order of magnitude above F(2x2) on every family: the transform's coefficients (up to 8 in A^T, |B^T d B| up to
100 max|d|) amplify the fp32 accumulation of the grouped GEMM; the algorithm's own fp32 rounding (wino_ref.winograd_ref with
fp32=True, no accumulation error) is ~1.5e-6 on the same launches.  On the prediction heads the largest coefficient error is
7.6e-5 absolute (exact-fp32 64x64 tile, F(4x4)), inside the 1e-4 absolute bar of tests/test_gpu_batch_parity.py.
"""
import json
import os

import pytest
import torch

import wino_ref as R

pytestmark = pytest.mark.gpu

from yolact_amd import _lib as L  # noqa: E402
from yolact_amd import tune_table as TT  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# largest rel_err over this file on MI355X: F(2x2) 1.37e-6 / 9.4e-7 / 5.8e-7, F(4x4) 1.68e-5 / 1.70e-5 / 1.10e-5 (exact / x3 / h2)
BARS = {(2, 'f32'): 5e-6, (2, 'x3'): 3.5e-6, (2, 'h2'): 2.2e-6,
        (4, 'f32'): 5e-5, (4, 'x3'): 5e-5, (4, 'h2'): 4e-5}
_MAX = {}                 # largest rel_err per (m, family, test group), printed at the end of the module


def family(tile):
    return 'x3' if tile & L.TILE_X3 else 'h2' if tile & L.TILE_H2 else 'f32'


def _sub(tile, planes):
    if (tile & 31) == L.TILE_WG_128x256:
        return 'wg'
    return family(tile) + ('p' if planes else '')


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    print('\nWinograd KAT largest rel_err per (m, family): ' + ', '.join(
        'F%d/%s %.2e (bar %.0e)' % (m, f, max(e for (mm, ff, _, _), e in _MAX.items() if (mm, ff) == (m, f)), BARS[m, f])
        for m, f in sorted({k[:2] for k in _MAX})))
    for k, e in sorted(_MAX.items()):
        print('    F%d %-4s %-5s %-28s %.2e' % (k + (e,)))


def _record(err, m, tile, planes, test):
    key = (m, family(tile), _sub(tile, planes), test)
    _MAX[key] = max(_MAX.get(key, 0.0), err)


def _rel(y, ref, scale=None):
    """max|y - ref| / max|ref| over a list of (kernel, reference) pieces (or / scale)."""
    num = max(float((a.double() - b).abs().max()) for a, b in zip(y, ref))
    den = max(float(b.abs().max()) for b in ref) if scale is None else scale
    return num / (den + 1e-30)


def _check(pieces, refs, m, tile, planes, test, what='', bar=None, scale=None):
    for p in pieces:
        assert torch.isfinite(p).all(), (what, 'non-finite output')
    e = _rel(pieces, refs, scale)
    _record(e, m, tile, planes, test)
    bar = BARS[m, family(tile)] if bar is None else bar
    assert e < bar, (what, L.TILE_NAMES.get(tile, tile), planes, e, bar)
    return e


# ---- the table ------------------------------------------------------------------------------------------------------------------
def _shipped():
    with open(os.path.join(ROOT, 'yolact_amd', 'tune', 'gfx950.json')) as f:
        entries = json.load(f)['entries']
    out = []
    for k, v in sorted(entries.items()):
        kind, key, mode = TT.parse(k)
        if kind == 'wino' and v[0]:
            out.append((key, mode, int(v[0])) + TT.wino_parts(v[1]))
    return out


SHIPPED = _shipped()


def _sid(key, mode, m, tile, planes):
    B, H, W, C, Co, act, nseg, _ = key
    return 'B%d-%dx%d-%dto%d-a%d-s%d-%s-F%d-%s%s' % (B, H, W, C, Co, act, nseg, mode or 'fp32', m, L.TILE_NAMES[tile],
                                                    'p' if planes else '')


def _bands(H, m):
    """Row bands of a large map: first and last 2m + 1 rows, one tile-aligned and one misaligned interior band of m + 1 rows."""
    a = m * (H // (3 * m))
    b = m * (2 * H // (3 * m)) + 1
    return sorted({(0, 2 * m + 1), (H - 2 * m - 1, H), (a, a + m + 1), (b, b + m + 1)})


FULL_FLOPS = 2e9          # fp64 reference on the whole tensor below this many multiply-adds x 2, on row bands above


def _ref_dense(x, w, bias, bn, act, m):
    """(list of output row ranges, list of fp64 references on them)."""
    B, C, H, W = x.shape
    if 18.0 * B * H * W * C * w.shape[0] <= FULL_FLOPS or H <= 4 * (2 * m + 1):
        return [(0, H)], [R.conv3x3_ref(x, w, bias, bn, act)]
    bands = _bands(H, m)
    return bands, R.band_ref(x, w, bias, bn, act, bands)


def _bn(Co, g):
    import torch.nn as nn
    bn = nn.BatchNorm2d(Co).eval()
    with torch.no_grad():
        bn.weight.copy_(1 + 0.2 * torch.randn(Co, generator=g))
        bn.bias.copy_(0.2 * torch.randn(Co, generator=g))
        bn.running_mean.copy_(0.2 * torch.randn(Co, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(Co, generator=g))
    return bn


def _weights(Co, C, g):
    return torch.randn(Co, C, 3, 3, generator=g) / (9 * C) ** 0.5, 0.1 * torch.randn(Co, generator=g)


HEAD_D, HEAD_CLS, HEAD_CP = 32, 81, 84          # coefficients, classes, class row padded to a multiple of 4


def _head_weights(A, C, g):
    """The concatenated head filters as engine.Plan builds them: loc (4A) | coef (32A) | conf (84A, 3 zero rows per prior)."""
    wl, bl = _weights(4 * A, C, g)
    wm, bm = _weights(HEAD_D * A, C, g)
    wc, bc = _weights(HEAD_CLS * A, C, g)
    pad = HEAD_CP - HEAD_CLS
    wc = torch.nn.functional.pad(wc.view(A, HEAD_CLS, C, 3, 3), (0, 0, 0, 0, 0, 0, 0, pad)).reshape(A * HEAD_CP, C, 3, 3)
    bc = torch.nn.functional.pad(bc.view(A, HEAD_CLS), (0, pad)).reshape(A * HEAD_CP)
    return torch.cat([wl, wm, wc]), torch.cat([bl, bm, bc])


def head_case(key, g):
    """Filters, bias, segments [(n0, n1, act)], rows of the level-concatenated tensors and the level's first row of a head launch."""
    B, H, W, C, Co, act, nseg, _ = key
    A = Co // (4 + HEAD_D + HEAD_CP)
    assert A * (4 + HEAD_D + HEAD_CP) == Co and act == 0 and nseg == 3, key
    w, b = _head_weights(A, C, g)
    off = 7 + H                                     # level offset in pixel rows (priors / A), sentinels before and after
    n1, n2 = 4 * A, (4 + HEAD_D) * A
    return w, b, [(0, n1, L.ACT_NONE), (n1, n2, L.ACT_TANH), (n2, Co, L.ACT_NONE)], off + H * W + 5, off


def run_launch(key, m, tile, planes, seed, test, twice=True):
    """One shipped launch against fp64; returns the rel_err."""
    from gpu_utils import run_wino
    B, H, W, C, Co, act, nseg, _ = key
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=g)
    what = str((key, m, tile, planes))
    if nseg == 3:                                   # prediction heads
        w, b, sdef, rows, off = head_case(key, g)
        segs = [(a, z, s, rows, off) for a, z, s in sdef]
        run = lambda: run_wino(x, w, b, None, L.ACT_NONE, tile, m, bool(planes), segs=segs)   # noqa: E731
        ys = run()
        if 18.0 * B * H * W * C * Co <= FULL_FLOPS or H <= 4 * (2 * m + 1):
            bands = [(0, H)]
            pre = [R.conv3x3_ref(x, w, b)]
        else:
            bands = _bands(H, m)
            pre = R.band_ref(x, w, b, None, R.ACT_NONE, bands)
        # every segment against fp64, relative to the scale of the launch's convolution (max|conv + bias| before any
        # activation, as for a dense launch): tanh is 1-Lipschitz, so a coefficient's error is at most its pre-activation error
        scale = max(float(p.abs().max()) for p in pre)
        for (a, z, s), yk in zip(sdef, ys):
            assert torch.isnan(yk[:, :off]).all() and torch.isnan(yk[:, off + H * W:]).all(), (what, 'wrote outside its level')
            got, ref = [], []
            for (r0, r1), p in zip(bands, pre):
                got.append(yk[:, off + r0 * W:off + r1 * W])
                ref.append(R.act_ref(p[:, a:z], s).permute(0, 2, 3, 1).reshape(B, (r1 - r0) * W, z - a))
            e = _check(got, ref, m, tile, planes, test, what + ' seg %d' % a, scale=scale)
        slots = run_wino.last_slots
        for k, yk in enumerate(ys):
            assert slots[1 + k] == yk[:, off:off + H * W].abs().max().item(), (what, k, slots)
    elif nseg == 2:                                 # merged head0.up0 + proto.0: two dense halves, one bound slot each
        assert act == 0 and Co % 2 == 0, key
        w, b = _weights(Co, C, g)
        h = Co // 2
        w[h:] *= 1024.0
        b[h:] *= 1024.0
        segs = [(0, h, L.ACT_RELU, H * W, 0), (h, Co, L.ACT_RELU, H * W, 0)]
        run = lambda: run_wino(x, w, b, None, L.ACT_NONE, tile, m, bool(planes), segs=segs)   # noqa: E731
        ys = run()
        bands, pre = _ref_dense(x, w, b, None, R.ACT_RELU, m)
        for k, (a, z) in enumerate(((0, h), (h, Co))):
            yk = ys[k].view(B, H, W, z - a).permute(0, 3, 1, 2)
            e = _check([yk[:, :, r0:r1] for r0, r1 in bands], [p[:, a:z] for p in pre], m, tile, planes, test, what + ' half %d' % k)
        slots = run_wino.last_slots
        assert slots[1] == ys[0].abs().max().item() and slots[2] == ys[1].abs().max().item(), (what, slots)
        assert slots[2] > 100 * slots[1]
    else:                                           # dense
        assert nseg == 0 and act in (0, 1), key
        w, b = _weights(Co, C, g)
        bn = _bn(Co, g)
        ract = R.ACT_RELU if act == 1 else R.ACT_NONE
        run = lambda: run_wino(x, w, b, bn, act, tile, m, bool(planes))   # noqa: E731
        y = run()
        bands, pre = _ref_dense(x, w, b, bn, ract, m)
        e = _check([y[:, :, r0:r1] for r0, r1 in bands], pre, m, tile, planes, test, what)
        assert run_wino.last_amax[1] == y.abs().max().item(), (what, run_wino.last_amax)
        ys = [y]
    if twice:
        ys2 = run()
        ys2 = ys2 if isinstance(ys2, list) else [ys2]
        for a, z in zip(ys, ys2):
            assert torch.equal(a.nan_to_num(7.0), z.nan_to_num(7.0)), (what, 'second launch differs')
    return e


def test_shipped_table_has_every_winograd_class():
    """The sweep below is read from the table: it must reach m = 2 and 4, exact / bf16x3 / fp16x2 / fp16x2 + V planes / the
    persistent wg GEMM, and nseg 0 / 2 / 3."""
    assert len(SHIPPED) >= 240
    ms = {m for _, _, m, _, _ in SHIPPED}
    subs = {_sub(t, p) for _, _, _, t, p in SHIPPED}
    nsegs = {k[6] for k, _, _, _, _ in SHIPPED}
    assert ms == {2, 4} and {'f32', 'x3', 'h2', 'h2p', 'wg'} <= subs and nsegs == {0, 2, 3}, (ms, subs, nsegs)
    for m in (2, 4):
        assert {family(t) for _, _, mm, t, _ in SHIPPED if mm == m} == {'f32', 'x3', 'h2'}, m


def shipped_seed(key):
    return 1000 + key[0] * 131 + key[1] * 7 + key[4]


@pytest.mark.parametrize('key,mode,m,tile,planes', SHIPPED, ids=[_sid(*s) for s in SHIPPED])
def test_winograd_shipped_launch(key, mode, m, tile, planes):
    """One Winograd launch of the table, as the plan makes it."""
    run_launch(key, m, tile, planes, shipped_seed(key), 'shipped ' + ('heads' if key[6] == 3 else 'merged' if key[6] == 2 else 'dense'))


# ---- the fused forms of protonet's last 3x3 -------------------------------------------------------------------------------------
FUSED_KEYS = sorted({(k, m, t, p) for k, _, m, t, p in SHIPPED if k[1] in (138, 176) and k[3] == k[4] == 256 and m == 4 and k[6] == 0})
FUSED = [(k, m, t, p, f) for k, m, t, p in FUSED_KEYS for f in ('up', 'proj', 'up+proj')]
FUSED_SMALL = [((2, 2 * lo, 2 * lo, 256, 256, 1, 0, (2, 4)), 4, t, p, f) for lo in (5, 7, 9)
               for t, p in sorted({(t, p) for k, m, t, p in FUSED_KEYS if k[1] == 138}) for f in ('up', 'up+proj')]


def fused_case(key, form, seed, proj_cout=32):
    """(3x3 filters, bias, low-res input or None, the 3x3's fp64 input, (1x1 filters, bias, act2) or None)."""
    B, H, W, C, Co, act, nseg, _ = key
    g = torch.Generator().manual_seed(seed)
    w, b = _weights(Co, C, g)
    lo = None
    if 'up' in form:
        lo = torch.randn(B, C, H // 2, W // 2, generator=g)
        xin = R.upsample2x_ref(lo, relu=True)
    else:
        xin = torch.randn(B, C, H, W, generator=g).double()
    proj = None
    if 'proj' in form:
        pw = torch.randn(proj_cout, Co, 1, 1, generator=g) / Co ** 0.5
        pb = 0.1 * torch.randn(proj_cout, generator=g)
        proj = (pw, pb, L.ACT_RELU)
    return w, b, lo, xin, proj


def run_fused(key, m, tile, planes, form, seed, proj_cout=32, proj_ldy=None):
    """protonet's last 3x3 (256 -> 256 + ReLU) with its input interpolated from the half-size tensor (+ ReLU) and/or the 1x1
    256 -> proj_cout + ReLU fused into its output transform; compared on row bands against fp64."""
    from gpu_utils import run_wino
    w, b, lo, xin, proj = fused_case(key, form, seed, proj_cout)
    up = lo is not None
    run = lambda: run_wino(None if up else xin.float(), w, b, None, L.ACT_RELU, tile, m, bool(planes),   # noqa: E731
                           up_from=lo, up_relu=True, proj=proj, proj_ldy=proj_ldy)
    y = run()
    bands, pre = _ref_dense(xin, w, b, None, R.ACT_RELU, m)
    if proj is not None:
        pre = [R.proj_ref(p, proj[0], proj[1], R.ACT_RELU) for p in pre]
        n = proj_cout
        if proj_ldy and proj_ldy > n:
            assert torch.isnan(y[:, n:]).all(), 'fused projection wrote its padding channels'
        y = y[:, :n]
    what = str((key, tile, planes, form))
    e = _check([y[:, :, r0:r1] for r0, r1 in bands], pre, m, tile, planes, 'fused ' + form, what)
    assert run_wino.last_amax[1] == y.abs().max().item(), (what, run_wino.last_amax)
    y2 = run()
    assert torch.equal(y.nan_to_num(7.0), y2[:, :y.shape[1]].nan_to_num(7.0)), what
    return e


def _fid(s):
    key, m, tile, planes, form = s
    return 'B%d-%dx%d-F%d-%s%s-%s' % (key[0], key[1], key[2], m, L.TILE_NAMES[tile], 'p' if planes else '', form)


def fused_seed(key):
    return 3000 + key[0] + key[1]


@pytest.mark.parametrize('key,m,tile,planes,form', FUSED + FUSED_SMALL, ids=[_fid(s) for s in FUSED + FUSED_SMALL])
def test_winograd_fused_forms(key, m, tile, planes, form):
    run_fused(key, m, tile, planes, form, fused_seed(key))


@pytest.mark.parametrize('tile,planes', [(65, 1), (33, 0), (2, 0)], ids=['128x128h2p', '128x128x3', '128x64'])
def test_winograd_fused_projection_keeps_padding_channels(tile, planes):
    """proj_cout 20 < proj_ldy 32: channels 20 .. 31 of every output pixel keep their NaN."""
    run_fused((2, 18, 22, 256, 256, 1, 0, (2, 4)), 4, tile, planes, 'up+proj', 77, proj_cout=20, proj_ldy=32)


def test_fused_sweep_covers_the_protonet_shapes():
    Bs = {k[0] for k, _, _, _, _ in FUSED if k[1] == 138}
    assert {1, 2, 4, 8, 16} <= Bs and any(k[1] == 176 for k, _, _, _, _ in FUSED), Bs


# ---- coverage of the timed plan -------------------------------------------------------------------------------------------------
def _params():
    out = {(k[0], k[1], k[2], k[3], k[4], m, t, p, False, False, k[6]) for k, _, m, t, p in SHIPPED}
    for k, m, t, p, f in FUSED:
        out.add((k[0], k[1], k[2], k[3], k[4], m, t, p, 'up' in f, 'proj' in f, k[6]))
    return out


def test_timed_plan_winograd_launches_are_all_covered():
    """Every Winograd op of the batch-8 timed plan of configs[1] (what bench.py times) is one of this file's parametrisations."""
    import yolact_amd
    from yolact_amd.utils.synth import synth_images, synth_state_dict
    yolact_amd.set_cfg('yolact_resnet50_config')
    from yolact_amd.yolact import Yolact
    net = Yolact()
    net.load_state_dict_compat(synth_state_dict([(k, tuple(v.shape)) for k, v in net.state_dict().items()], seed=0, conf_gain=0.04))
    net = net.to('cuda:0')
    x = synth_images(8, 550, 550, seed=1234).to('cuda:0')
    plan = net.plan_for(x)
    params = _params()
    found = []
    for fn, args, name, _ in plan.ops:
        if not (isinstance(name, str) and name.endswith('[wino]')):
            continue
        d = args.contents
        p = (d.B, d.H, d.W, d.C, d.Cout, d.m, d.tile & 255, d.v_planes, bool(d.x_up), bool(d.proj_w_h2), d.nseg)
        found.append((name, p))
        assert p in params, (name, p)
    print('timed plan: %d Winograd launches, all covered: %s' % (len(found), found))
    assert len(found) >= 15
    assert any(p[8] and p[9] for _, p in found) and any(p[10] == 2 for _, p in found) and any(p[10] == 3 for _, p in found)


# ---- edges ----------------------------------------------------------------------------------------------------------------------
EDGE_TILES = [L.TILE_128x64, L.TILE_128x128 | L.TILE_X3, L.TILE_32x64_K2 | L.TILE_H2, (L.TILE_128x128 | L.TILE_H2, 1),
              (L.TILE_WG_128x256 | L.TILE_H2, 1)]
EDGE_TILES = [t if isinstance(t, tuple) else (t, 0) for t in EDGE_TILES]
_EID = lambda tp: L.TILE_NAMES[tp[0]] + ('p' if tp[1] else '')   # noqa: E731


def _geoms(m):
    return sorted({(1, 1), (1, 37), (2, 3), (3, 2), (m + 1, m + 1), (4 * 2 + 3, 4 * 3 + 3), (m + 1, 4 * 4 + 3), (3, 1)})


@pytest.mark.parametrize('tp', EDGE_TILES, ids=_EID)
@pytest.mark.parametrize('m', [2, 4])
def test_winograd_edge_geometries(m, tp):
    """Every H, W in {1, 2, 3, m + 1, 4k + 3} combination of _geoms (H = 1 with a wide W included), batch 3, 44 ragged columns,
    LeakyReLU: against fp64 on the whole tensor."""
    from gpu_utils import run_wino
    tile, planes = tp
    for H, W in _geoms(m):
        g = torch.Generator().manual_seed(H * 100 + W)
        x = torch.randn(3, 64, H, W, generator=g)
        w, b = _weights(44, 64, g)
        y = run_wino(x, w, b, None, L.ACT_LEAKY01, tile, m, bool(planes))
        _check([y], [R.conv3x3_ref(x, w, b, None, R.ACT_LEAKY01)], m, tile, planes, 'edge geometry', (H, W))


@pytest.mark.parametrize('tp', EDGE_TILES, ids=_EID)
@pytest.mark.parametrize('m', [2, 4])
def test_winograd_zero_image_between_loud_ones(m, tp):
    """Image 1 of 3 is all zeros, images 0 and 2 are 2^10 loud: image 1 must be exactly ReLU(bias), to the bit."""
    from gpu_utils import run_wino
    tile, planes = tp
    g = torch.Generator().manual_seed(5)
    H, W = 4 * 3 + 3, 4 * 2 + 3
    x = 1024.0 * torch.randn(3, 64, H, W, generator=g)
    x[1] = 0
    w, b = _weights(44, 64, g)
    y = run_wino(x, w, b, None, L.ACT_RELU, tile, m, bool(planes))
    assert torch.equal(y[1], torch.relu(b).view(-1, 1, 1).expand(44, H, W)), (y[1] - torch.relu(b).view(-1, 1, 1)).abs().max()
    _check([y], [R.conv3x3_ref(x, w, b, None, R.ACT_RELU)], m, tile, planes, 'zero image')


@pytest.mark.parametrize('tp', EDGE_TILES, ids=_EID)
@pytest.mark.parametrize('m', [2, 4])
def test_winograd_one_hot_gives_the_flipped_filter(m, tp):
    """A unit impulse at (c, y, x) gives out[n, y - dy, x - dx] = w[n, c, 1 + dy, 1 + dx] (correlation, not convolution): at
    corners, edges and every tile phase of the interior."""
    from gpu_utils import run_wino
    tile, planes = tp
    H, W = 13, 11
    g = torch.Generator().manual_seed(9)
    w, _ = _weights(36, 64, g)
    pts = [(0, 0, 0), (1, H - 1, W - 1), (2, 0, W - 1), (3, H - 1, 0)] + [(4 + k, 4 + k, 3 + k) for k in range(5)]
    x = torch.zeros(len(pts), 64, H, W)
    for i, (c, py, px) in enumerate(pts):
        x[i, c, py, px] = 1.0
    y = run_wino(x, w, None, None, L.ACT_NONE, tile, m, bool(planes))
    ref = R.conv3x3_ref(x, w)
    for i, (c, py, px) in enumerate(pts):          # the reference itself: the flipped filter around the impulse, zero elsewhere
        exp = torch.zeros(36, H + 2, W + 2, dtype=torch.float64)
        exp[:, py:py + 3, px:px + 3] = w[:, c].double().flip(1, 2)
        assert torch.equal(ref[i], exp[:, 1:H + 1, 1:W + 1])
    _check([y], [ref], m, tile, planes, 'one-hot')


H2_FAMILIES = [(L.TILE_32x64_K2 | L.TILE_H2, 0), (L.TILE_128x128 | L.TILE_H2, 0), (L.TILE_32x64_K2 | L.TILE_H2, 1),
               (L.TILE_128x128 | L.TILE_H2, 1), (L.TILE_256x128_W8_S3 | L.TILE_H2, 1), (L.TILE_WG_128x256 | L.TILE_H2, 1)]
GAIN_IJ = {2: [(1, 1), (1, 2), (2, 2)], 4: [(0, 0), (0, 5), (1, 2), (5, 5)]}


def max_gain_bar(x, w, m, tile):
    """The bar on max_gain_input: the family's bar, or 4x what the algorithm itself adds in fp32 on this input if larger."""
    e32 = _rel([R.winograd_ref(x, w, m, fp32=True)], [R.conv3x3_ref(x, w)])
    return max(BARS[m, family(tile)], 4 * e32), e32


@pytest.mark.parametrize('tp', H2_FAMILIES, ids=_EID)
@pytest.mark.parametrize('m', [2, 4])
def test_winograd_max_gain_input_on_fp16x2(m, tp):
    """V component (i, j) at exactly gain * max|x| on every interior tile (wino_ref.max_gain_input): the V scale of the fp16x2
    GEMM (x_amax * 4 / * 100) must keep every piece finite and the result fp32-class."""
    from gpu_utils import run_wino
    tile, planes = tp
    for ij in GAIN_IJ[m]:
        x = R.max_gain_input(2, 64, 4 * m + 3, 6 * m + 1, m, ij, A=0.75, seed=ij[0] * 6 + ij[1]).float()
        g = torch.Generator().manual_seed(11)
        w, b = _weights(132, 64, g)
        y = run_wino(x, w, None, None, L.ACT_NONE, tile, m, bool(planes))
        bar, e32 = max_gain_bar(x, w, m, tile)
        _check([y], [R.conv3x3_ref(x, w)], m, tile, planes, 'max gain', (ij, e32), bar=bar)


@pytest.mark.parametrize('tp', EDGE_TILES, ids=_EID)
@pytest.mark.parametrize('m', [2, 4])
def test_winograd_hot_patch(m, tp):
    """A 5 x 5 patch of one image 2^10 louder than the rest (the fp16x2 scale follows the hot patch): bar relative to max|ref|."""
    from gpu_utils import run_wino
    tile, planes = tp
    g = torch.Generator().manual_seed(13)
    x = torch.randn(2, 128, 21, 19, generator=g)
    x[1, :, 7:12, 3:8] *= 1024.0
    w, b = _weights(64, 128, g)
    y = run_wino(x, w, b, None, L.ACT_NONE, tile, m, bool(planes))
    _check([y], [R.conv3x3_ref(x, w, b)], m, tile, planes, 'hot patch')
