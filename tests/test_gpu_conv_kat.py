"""The direct convolution engine (ymi_conv2d_nhwc_f32: csrc/conv_igemm.hip, and the kernels the table installs for ordinary
convolutions: the pipelined gather-GEMM of csrc/dcn.hip, csrc/wstat.hip, csrc/patch.hip, csrc/patch2.hip) against the independent
fp64 reference of tests/conv_ref.py (torch only: no engine code, no oracle).

  * every direct-convolution entry of yolact_amd/tune/gfx950.json (the 12-tuple keys without a 'dcn' tag), read from the table
    at test time and rebuilt as engine.Plan builds the launch: its exact (B, H, W, Cin, Cout, kh, kw, stride, pad, res_mode, nseg,
    Kpad), its tile (value & 255), its split-K (value >> 8, through engine.Plan._apply_choice itself: a split the plan refuses is
    asserted refused), its precision (the tile's: exact fp32, | X3 or | H2, which the key's plan mode plain / x3 / h2 admits), the act and residual its role carries: RES_ADD = the
    bottleneck conv3 (BatchNorm, ReLU, residual before the activation) and also the darknet unit (LeakyReLU, residual after it);
    RES_BILINEAR = the FPN lateral (bias, the coarser level (Ho + 1) / 2 upsampled and added); nseg 3 = the prediction heads scattered
    into level-concatenated loc / coef (tanh) / conf tensors at a non-zero prior offset with NaN before and after; nseg 2 = the
    merged head0.up0 + proto.0 launch, its second half 2^10 louder; Cin 4 = the stem with cin_pad 4; anything else BatchNorm + ReLU
    (a 1x1 stride-2 downsample: BatchNorm, no activation).  The fp16x2 bound x_amax comes from ymi_amax_f32.  Small launches are
    compared on the whole output, large ones on conv_ref.launch_bands (the first and last rows of every image, one interior band);
    input, reference and bands are built once per (shape, form) and shared by the plain / x3 / h2 entries of that shape;
  * per launch: every owned output finite, rel_err under the family bar, the NaN sentinels outside the segments intact, each
    y_amax slot equal to max|y| of its own segment, and a second launch bit-identical (split-K included);
  * edges: maps 1x1 / 2x3 / 3x1, batch 3 with H W no multiple of any block's rows, ragged Cout (351, 130, 36), the Cin 4 stem
    loader (the only Cin % 32 != 0 the engine takes: Cin 48 is refused), a split-K whose last range is one chunk, a zero image between two loud ones on fp16x2 tiles, an input with
    ldx > Cin whose ignored channels hold NaN, a residual with res_ld > Cout;
  * a coverage check: every ymi_conv2d_nhwc_f32 launch of the batch-8 timed plan of configs[1] is one of this file's launches.

Bars (rel_err = max|y - ref| / max|ref| per launch; for the heads max|y - ref| of each segment over max|conv + bias| of the launch,
since tanh compresses the coefficients' scale but not their error), one per family: exact fp32 tiles, bf16x3 (| YMI_TILE_X3),
fp16x2 (| YMI_TILE_H2, including the pipelined / weight-stationary / patch tiles).  Each is <= 4x the largest error this file
measured on MI355X and never above the earlier 2e-5; the maxima are printed at the end of the module.

  measured max rel_err   exact fp32   bf16x3    fp16x2      bar: exact fp32   bf16x3   fp16x2
                         2.30e-6      2.57e-6   1.58e-6          9e-6         1e-5     6e-6

The largest errors sit on the K = 2304 prediction heads and the merged P3 launch (relative to the launch's pre-activation scale) and
on the K = 2304 / 4608 dense 3x3s; the edges (1x1 maps, ragged Cout and M, ragged split-K, ldx > Cin, a zero image between loud
ones) stay below 1e-6.
"""
import collections
import ctypes as C
import json
import os

import pytest
import torch

import conv_ref as R

pytestmark = pytest.mark.gpu

from yolact_amd import _lib as L  # noqa: E402
from yolact_amd import tune_table as TT  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BARS = R.BARS
_MAX = {}                 # largest rel_err per (family, test group), printed at the end of the module


def family(tile):
    return 'x3' if tile & L.TILE_X3 else 'h2' if tile & L.TILE_H2 else 'f32'


def kernel_kind(tile):
    """Which kernel a tile id selects: 'igemm' (csrc/conv_igemm.hip), 'dcnp', 'wstat', 'patch', 'patch2'."""
    if not tile & L.TILE_DCNP:
        return 'igemm'
    b = tile & 31
    return 'wstat' if b in L.WS_TILES else 'patch' if b in L.PATCH_TILES else 'patch2' if b in L.PATCH2_TILES else \
        'pc' if b in L.PC_TILES else 'dcnp'


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    fams = sorted({k[0] for k in _MAX})
    print('\ndirect-conv KAT largest rel_err per family: ' + ', '.join(
        '%s %.2e (bar %.0e)' % (f, max(e for k, e in _MAX.items() if k[0] == f), BARS[f]) for f in fams))
    for k, e in sorted(_MAX.items()):
        print('    %-4s %-8s %-24s %.2e' % (k + (e,)))


def _record(err, tile, test):
    key = (family(tile), kernel_kind(tile), test)
    _MAX[key] = max(_MAX.get(key, 0.0), err)


def _rel(y, ref, scale=None):
    """max|y - ref| / max|ref| over a list of (kernel, reference) pieces (or / scale)."""
    num = max(float((a.double() - b).abs().max()) for a, b in zip(y, ref))
    den = max(float(b.abs().max()) for b in ref) if scale is None else scale
    return num / (den + 1e-30)


def _check(pieces, refs, tile, test, what='', scale=None):
    for p in pieces:
        assert torch.isfinite(p).all(), (what, 'non-finite output')
    e = _rel(pieces, refs, scale)
    _record(e, tile, test)
    assert e < BARS[family(tile)], (what, L.TILE_NAMES.get(tile, tile), e, BARS[family(tile)])
    return e


# ---- the table ------------------------------------------------------------------------------------------------------------------
def _shipped():
    with open(os.path.join(ROOT, 'yolact_amd', 'tune', 'gfx950.json')) as f:
        entries = json.load(f)['entries']
    out = []
    for k, v in entries.items():
        kind, key, mode = TT.parse(k)
        if kind == 'conv':                                  # ('dcn'-tagged keys: tests/test_gpu_dcn_kat.py)
            out.append((key, mode, int(v)))
    return sorted(out)


SHIPPED = _shipped()


def _sid(key, mode, val):
    B, H, W, Ci, Co, kh, kw, s, p, rm, ns, Kp = key
    return 'B%d-%dx%d-%dto%d-k%ds%d-r%d-n%d-%s-%s%s' % (B, H, W, Ci, Co, kh, s, rm, ns, mode or 'fp32', L.TILE_NAMES[val & 255],
                                                       '-k%d' % (val >> 8) if val >> 8 else '')


def geometry(key):
    B, H, W, Ci, Co, kh, kw, s, p, rm, ns, Kp = key
    return R.out_size(H, kh, s, p), R.out_size(W, kw, s, p)


def res_size(key):
    """Source size of an FPN lateral's bilinear residual: the next level, one stride-2 3x3 / pad 1 below (yolact.py:324-335)."""
    Ho, Wo = geometry(key)
    return (Ho + 1) // 2, (Wo + 1) // 2


def forms(key):
    """The activation / residual forms a key is run in: ('plain' | 'bottleneck' | 'darknet' | 'lateral' | 'heads' | 'merged' |
    'stem' | 'downsample')."""
    B, H, W, Ci, Co, kh, kw, s, p, rm, ns, Kp = key
    if rm == R.RES_ADD:
        return ['bottleneck', 'darknet']
    if rm == R.RES_BILINEAR:
        return ['lateral']
    if ns == 3:
        return ['heads']
    if ns == 2:
        return ['merged']
    if Ci == 4:
        return ['stem']
    if kh == 1 and s == 2:
        return ['downsample']
    return ['plain']


class _Desc:
    """Just enough of ymi_conv_desc for engine.Plan._apply_choice / _splitk_ok."""


def plan_split(key, form, val):
    """(tile, split_k) as engine.Plan._apply_choice installs `val` on this launch's descriptor, or None if it refuses it."""
    from yolact_amd.engine import Plan
    B, H, W, Ci, Co, kh, kw, s, p, rm, ns, Kp = key
    Ho, Wo = geometry(key)
    d = L.ConvDesc()
    d.B, d.H, d.W, d.Cin, d.ldx, d.Ho, d.Wo, d.Cout = B, H, W, Ci, Ci, Ho, Wo, Co
    d.kh, d.kw, d.stride, d.pad, d.Kpad, d.res_mode, d.nseg = kh, kw, s, p, Kp, rm, ns
    act = {'heads': L.ACT_NONE, 'merged': L.ACT_RELU, 'lateral': L.ACT_NONE, 'downsample': L.ACT_NONE,
           'darknet': L.ACT_LEAKY01}.get(form, L.ACT_RELU)
    d.seg[0] = L.ConvSeg(0, Co if ns == 1 else 4, act, Co, Ho * Wo * Co, None)
    fake = _Desc()
    fake.lib = _Desc()
    fake.lib.ymi_dcn_v2_forward_f32 = object()
    fake._splitk_ok = Plan._splitk_ok
    fake._splitk_ws = lambda where, n: torch.empty(1)
    ok = Plan._apply_choice(fake, lambda dp, st: 0, C.pointer(d), 0, val, None)
    return (d.tile, d.split_k) if ok == 0 else None


LAUNCHES = [(k, mode, v, f) for k, mode, v in SHIPPED for f in forms(k)]


def test_shipped_table_reaches_every_class():
    """The sweep below is read from the table: >= 670 entries reaching the three precisions, split-K, both residual modes,
    nseg 1 / 2 / 3, the stem and the pipelined / weight-stationary / patch / patch2 kernels; every precision suffix matches its tile."""
    assert len(SHIPPED) >= 670, len(SHIPPED)
    fams = collections.Counter(family(v & 255) for _, _, v in SHIPPED)
    for k, mode, v in SHIPPED:            # (a plan's candidates include the exact-fp32 tiles whatever its precision)
        assert family(v & 255) in ('f32', mode or 'f32'), (k, mode, v)
    assert set(fams) == {'f32', 'x3', 'h2'}, fams
    assert any(v >> 8 for _, _, v in SHIPPED)
    assert {k[9] for k, _, _ in SHIPPED} == {0, 1, 2} and {k[10] for k, _, _ in SHIPPED} == {1, 2, 3}
    assert any(k[3] == 4 and k[5] == 7 for k, _, _ in SHIPPED)
    kinds = {kernel_kind(v & 255) for _, _, v in SHIPPED}
    assert {'igemm', 'dcnp', 'wstat', 'patch', 'patch2'} <= kinds, kinds


# ---- one launch -------------------------------------------------------------------------------------------------------------------
def shipped_seed(key):
    return 2000 + key[0] * 131 + key[1] * 7 + key[3] * 3 + key[4] + key[5] * 11 + key[7] * 5 + key[9] * 17


_CACHE = collections.OrderedDict()        # (key, form) -> case: shared by the plain / x3 / h2 entries of one shape


def build_case(key, form):
    ck = (key, form)
    if ck in _CACHE:
        _CACHE.move_to_end(ck)
        return _CACHE[ck]
    B, H, W, Ci, Co, kh, kw, s, p, rm, ns, Kp = key
    Ho, Wo = geometry(key)
    g = torch.Generator().manual_seed(shipped_seed(key))
    cin = 3 if form == 'stem' else Ci
    x = torch.randn(B, cin, H, W, generator=g)
    case = dict(x=x, stride=s, pad=p, res=None, res_mode=R.RES_NONE, res_after_act=0, bn=None, cin_pad=None, segs=None)
    bands = R.launch_bands(B, Ho, Wo, Co, Kp)
    if form == 'heads':
        A = R.head_priors(Co)
        w, b = R.head_weights(A, Ci, g, kh)
        off = 7 + H
        rows = off + Ho * Wo + 5
        case.update(w=w, b=b, act=L.ACT_NONE, segs=[(n0, n1, a, rows, off) for n0, n1, a in R.head_segments(A)])
    elif form == 'merged':
        w, b = R.weights(Co, Ci, g, kh)
        h = Co // 2
        w[h:] *= 1024.0
        b[h:] *= 1024.0
        case.update(w=w, b=b, act=L.ACT_RELU, segs=[(0, h, L.ACT_RELU, Ho * Wo, 0), (h, Co, L.ACT_RELU, Ho * Wo, 0)])
    else:
        w, b = R.weights(Co, cin, g, kh)
        if form == 'lateral':
            rh, rw = res_size(key)
            case.update(act=L.ACT_NONE, res=torch.randn(B, Co, rh, rw, generator=g), res_mode=R.RES_BILINEAR)
        else:
            case['bn'] = R.batchnorm(Co, g)
            case['act'] = {'darknet': L.ACT_LEAKY01, 'downsample': L.ACT_NONE, 'stem': L.ACT_RELU if kh == 7 else L.ACT_LEAKY01}.get(form, L.ACT_RELU)
            if form in ('bottleneck', 'darknet'):
                case.update(res=torch.randn(B, Co, Ho, Wo, generator=g), res_mode=R.RES_ADD, res_after_act=int(form == 'darknet'))
            if form == 'stem':
                case['cin_pad'] = 4
        case.update(w=w, b=b)
    rs = None if case['segs'] is not None else case['act']
    pre = R.band_ref(x, case['w'], case['b'], case['bn'], s, p, rs if rs is not None else R.ACT_NONE, bands, case['res'],
                     case['res_mode'], case['res_after_act'])
    case.update(bands=bands, pre=pre)
    if torch.cuda.is_available():
        from gpu_utils import DEV, nhwc
        xn = nhwc(x)
        if case['cin_pad']:
            xn = torch.nn.functional.pad(xn, (0, case['cin_pad'] - cin))
        case['xd'] = xn.to(DEV)
    _CACHE[ck] = case
    while len(_CACHE) > 2:
        _CACHE.popitem(last=False)
    return case


def run_case(case, tile, split_k, test, what):
    """One launch of a case against its fp64 bands; returns the rel_err."""
    from gpu_utils import run_conv
    B = case['x'].shape[0]
    out = run_conv(case['x'], case['w'], case['b'], case['bn'], case['stride'], case['pad'], act=case['act'], res=case['res'],
                   res_mode=case['res_mode'], res_after_act=case['res_after_act'], tile=tile, cin_pad=case['cin_pad'],
                   split_k=split_k, segs=case['segs'], bands=case['bands'], twice=True, x_dev=case.get('xd'))
    slots, amax = run_conv.last_slots, run_conv.last_out_amax
    assert run_conv.last_finite, (what, 'non-finite output')
    assert run_conv.last_identical, (what, 'second launch differs')
    bands, pre = case['bands'], case['pre']
    if case['segs'] is None:
        e = _check(out, pre, tile, test, what)
        assert slots[1] == amax[0], (what, slots, amax)
        return e
    assert all(run_conv.last_sentinels), (what, 'wrote outside its level', run_conv.last_sentinels)
    scale = max(float(q.abs().max()) for q in pre) if len(case['segs']) == 3 else None
    e = 0.0
    for k, ((n0, n1, act, _, _), got) in enumerate(zip(case['segs'], out)):
        ref = [R.act_ref(q[:, n0:n1], act).permute(0, 2, 3, 1).reshape(B, -1, n1 - n0) for q in pre]
        e = max(e, _check(got, ref, tile, test, what + ' seg %d' % k, scale=scale))
        assert slots[1 + k] == amax[k], (what, k, slots, amax)
    if len(case['segs']) == 2:
        assert slots[2] > 100 * slots[1], slots
    return e


@pytest.mark.parametrize('key,mode,val,form', LAUNCHES, ids=[_sid(k, m, v) + '-' + f for k, m, v, f in LAUNCHES])
def test_conv_shipped_launch(key, mode, val, form):
    """One direct-convolution launch of the table, as the plan makes it."""
    choice = plan_split(key, form, val)
    if choice is None:                    # the plan refuses this entry (a tune miss): so must the launch rules it mirrors
        pytest.fail('the plan refuses shipped entry %s %s' % (key, val))
    tile, S = choice
    assert tile == val & 255 and S == (val >> 8 if val >> 8 > 1 else 0), (choice, val)
    case = build_case(key, form)
    run_case(case, tile, S, 'shipped ' + form, str((key, mode, val, form)))


# ---- edges ------------------------------------------------------------------------------------------------------------------------
EDGE_TILES = [L.TILE_128x128, L.TILE_32x32_K4, L.TILE_128x256_W8 | L.TILE_H2, L.TILE_64x64 | L.TILE_X3, L.TILE_32x64_K2_S3 | L.TILE_H2,
              L.TILE_128x128_W8_S4 | L.TILE_X3, L.DCNP_64x128 | L.TILE_H2 | L.TILE_DCNP, L.DCNP_PATCH2_192 | L.TILE_H2 | L.TILE_DCNP]
_EID = lambda t: L.TILE_NAMES[t]   # noqa: E731


def ws_split(tile, Kpad):
    """The fewest K ranges that fit a weight-stationary block's filters in its 64 KB of LDS (Plan.ws_candidates); 0 elsewhere."""
    if kernel_kind(tile) != 'wstat':
        return 0
    bn = int(L.WS_TILES[tile & 31][2:].split('w')[0].split('x')[1])
    nk, cap = Kpad // 32, (64 * 1024) // (bn * 128)
    S = -(-nk // cap)
    return S if S > 1 else 0


def _runs(tile, kh, s, p, Co, Ci=64):
    """Whether a tile takes this layer (the kernels' own launch rules: tests/test_gpu_kernels.py test_conv_plain)."""
    k = kernel_kind(tile)
    if k == 'patch2':
        return (kh, s, p) == (3, 1, 1) and Co >= 64 and Co % 4 == 0 and Ci % 32 == 0
    if k == 'dcnp':
        return (kh, p) in ((3, 1), (1, 0)) and Co % 4 == 0 and Ci % 32 == 0
    if tile & (L.TILE_X3 | L.TILE_H2):
        return Ci % 32 == 0
    return True


EDGE_SHAPES = [  # B, Cin, H, W, Cout, k, stride, pad
    (3, 64, 1, 1, 36, 3, 1, 1), (3, 64, 1, 1, 68, 3, 1, 1), (3, 64, 2, 3, 130, 3, 1, 1), (3, 64, 2, 3, 132, 3, 1, 1),
    (3, 64, 3, 1, 351, 3, 1, 1), (3, 64, 3, 1, 68, 3, 1, 1), (3, 64, 2, 3, 36, 1, 1, 0), (3, 64, 13, 11, 130, 3, 1, 1),
    (3, 64, 13, 11, 132, 3, 1, 1), (3, 64, 13, 11, 351, 3, 2, 1), (3, 96, 9, 7, 36, 1, 2, 0), (3, 64, 29, 23, 256, 1, 1, 0)]


@pytest.mark.parametrize('tile', EDGE_TILES, ids=_EID)
def test_conv_edge_geometries(tile):
    """Maps 1x1 / 2x3 / 3x1, batch 3 with H W no multiple of any block's rows (13 x 11, 29 x 23), ragged Cout 351 / 130 / 36,
    stride 2, BatchNorm + LeakyReLU: against fp64 on the whole tensor."""
    from gpu_utils import run_conv
    n = 0
    for B, Ci, H, W, Co, k, s, p in EDGE_SHAPES:
        if not _runs(tile, k, s, p, Co, Ci):
            continue
        g = torch.Generator().manual_seed(H * 100 + W + Co)
        x = torch.randn(B, Ci, H, W, generator=g)
        w, b = R.weights(Co, Ci, g, k)
        bn = R.batchnorm(Co, g)
        y = run_conv(x, w, b, bn, s, p, act=L.ACT_LEAKY01, tile=tile)
        _check([y], [R.conv_ref(x, w, b, bn, s, p, R.ACT_LEAKY01)], tile, 'edge geometry', (B, Ci, H, W, Co, k, s))
        n += 1
    assert n >= 3


@pytest.mark.parametrize('tile', [t | f for t in (L.TILE_64x64, L.TILE_128x64) for f in (0, L.TILE_X3, L.TILE_H2)], ids=_EID)
def test_conv_stem_loader_edges(tile):
    """The Cin 4 loader (3 real channels, cin_pad 4): 7x7 / s2 / p3 and 3x3 / s1 / p1 at odd sizes, batch 3."""
    from gpu_utils import run_conv
    for H, W, k, s, p in ((35, 27, 7, 2, 3), (9, 13, 3, 1, 1), (1, 2, 7, 2, 3)):
        g = torch.Generator().manual_seed(H + W + k)
        x = torch.randn(3, 3, H, W, generator=g)
        w, b = R.weights(64, 3, g, k)
        bn = R.batchnorm(64, g)
        y = run_conv(x, w, b, bn, s, p, act=L.ACT_RELU, tile=tile, cin_pad=4)
        _check([y], [R.conv_ref(x, w, b, bn, s, p, R.ACT_RELU)], tile, 'stem edge', (H, W, k))


def test_conv_cin_not_multiple_of_32_needs_the_stem_loader():
    """Cin % 32 != 0 is the Cin 4 stem loader's alone (include/yolact_amd.h, validate in csrc/conv_igemm.hip): Cin 48 is refused with
    YMI_ESHAPE on every family, not computed from a partial K chunk (test_conv_stem_loader_edges runs the 3 -> 4 channel case)."""
    from gpu_utils import run_conv
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 48, 7, 9, generator=g)
    w, b = R.weights(64, 48, g, 3)
    for tile in (L.TILE_128x128, L.TILE_64x64 | L.TILE_X3, L.TILE_64x64 | L.TILE_H2):
        with pytest.raises(RuntimeError, match='shape'):
            run_conv(x, w, b, None, 1, 1, tile=tile)


SPLIT_TILES = [L.DCNP_64x256_W8, L.DCNP_128x256_W16, L.DCNP_64x128, L.DCNP_128x64_W8]


@pytest.mark.parametrize('tile', [t | L.TILE_H2 | L.TILE_DCNP for t in SPLIT_TILES], ids=_EID)
def test_conv_split_k_last_range_one_chunk(tile):
    """1x1 with Kpad 320 = 10 chunks cut 4 ways: ranges 3 / 3 / 3 / 1 (and 5 ways: 2 / 2 / 2 / 2 / 2); 3x3 on 32 channels = 9
    chunks cut 3 ways: 4 / 4 / 1; with a residual, batch 2 at 9 x 7: against fp64, and bit-identical on a second launch."""
    from yolact_amd.engine import Plan
    for k, Ci, S in ((1, 320, 4), (1, 320, 5), (3, 32, 3)):
        nk = k * k * Ci // 32
        assert -(-nk // S) * (S - 1) < nk                 # the plan's rule (Plan.dcnp_candidates / _apply_choice) admits it
        g = torch.Generator().manual_seed(nk * 10 + S)
        x = torch.randn(2, Ci, 9, 7, generator=g)
        w, b = R.weights(256, Ci, g, k)
        bn = R.batchnorm(256, g)
        res = torch.randn(2, 256, 9, 7, generator=g)
        case = dict(x=x, w=w, b=b, bn=bn, stride=1, pad=k // 2, act=L.ACT_RELU, res=res, res_mode=R.RES_ADD, res_after_act=0,
                    cin_pad=None, segs=None, bands=[(0, 9)])
        case['pre'] = [R.conv_ref(x, w, b, bn, 1, k // 2, R.ACT_RELU, res, R.RES_ADD)]
        run_case(case, tile, S, 'split-K ragged', str((k, Ci, S)))
    assert Plan is not None


@pytest.mark.parametrize('tile', [L.TILE_64x64 | L.TILE_H2, L.TILE_32x32_K4 | L.TILE_H2, L.TILE_256x128_W8_S3 | L.TILE_H2,
                                  L.DCNP_128x128_W8 | L.TILE_H2 | L.TILE_DCNP, 25 | L.TILE_H2 | L.TILE_DCNP,
                                  L.DCNP_PATCH2_256 | L.TILE_H2 | L.TILE_DCNP], ids=_EID)
def test_conv_zero_image_between_loud_ones(tile):
    """Image 1 of 3 is all zeros, images 0 and 2 are 2^10 loud (the fp16x2 scale follows the loud ones): image 1 must be exactly
    act(bias), and the error is measured against the launch's max."""
    from gpu_utils import run_conv
    g = torch.Generator().manual_seed(5)
    Co = 64
    x = 1024.0 * torch.randn(3, 64, 15, 11, generator=g)
    x[1] = 0
    w, b = R.weights(Co, 64, g, 3)
    y = run_conv(x, w, b, None, 1, 1, act=L.ACT_RELU, tile=tile, split_k=ws_split(tile, 9 * 64))
    assert torch.equal(y[1], torch.relu(b).view(-1, 1, 1).expand(Co, 15, 11)), (y[1] - torch.relu(b).view(-1, 1, 1)).abs().max()
    _check([y], [R.conv_ref(x, w, b, None, 1, 1, R.ACT_RELU)], tile, 'zero image')


@pytest.mark.parametrize('tile', [L.TILE_128x64, L.TILE_64x128 | L.TILE_X3, L.TILE_32x64_K2 | L.TILE_H2,
                                  L.DCNP_64x128_W8 | L.TILE_H2 | L.TILE_DCNP, 24 | L.TILE_H2 | L.TILE_DCNP,
                                  L.DCNP_PATCH2_192 | L.TILE_H2 | L.TILE_DCNP], ids=_EID)
def test_conv_reads_only_channels_below_cin(tile):
    """x with ldx = Cin + 32 whose channels [Cin, ldx) hold NaN (include/yolact_amd.h: only [0, Cin) is read), and a residual with
    res_ld > Cout whose padding holds NaN (patch2 takes no residual: none there)."""
    from gpu_utils import run_conv
    g = torch.Generator().manual_seed(21)
    Co = 64
    for k, p in ((3, 1), (1, 0)):
        if not _runs(tile, k, 1, p, Co):
            continue
        x = torch.randn(2, 64, 13, 9, generator=g)
        w, b = R.weights(Co, 64, g, k)
        bn = R.batchnorm(Co, g)
        resid = kernel_kind(tile) not in ('patch2', 'wstat')
        res = torch.randn(2, Co, 13, 9, generator=g) if resid else None
        rm = R.RES_ADD if resid else R.RES_NONE
        y = run_conv(x, w, b, bn, 1, p, act=L.ACT_RELU, tile=tile, ldx=96, res=res, res_mode=rm, res_ld=Co + 4 if resid else None,
                     split_k=ws_split(tile, k * k * 64))
        _check([y], [R.conv_ref(x, w, b, bn, 1, p, R.ACT_RELU, res, rm)], tile, 'ldx > Cin', (k, tile))


# ---- coverage of the timed plan -------------------------------------------------------------------------------------------------
def _params():
    out = set()
    for k, _, v, f in LAUNCHES:
        if plan_split(k, f, v) is None:
            continue
        t, S = plan_split(k, f, v)
        out.add(k[:9] + (k[9], k[10], k[11], t, S))
    return out


def test_timed_plan_conv_launches_are_all_covered():
    """Every ymi_conv2d_nhwc_f32 op of the batch-8 timed plan of configs[1] (what bench.py times) is one of this file's
    parametrisations (ops the pointwise chain replaced are no longer conv launches); FPN laterals read the residual size
    res_size() assumes."""
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
    lib = L.lib()
    found = []
    for fn, args, name, _ in plan.ops:
        if fn is not lib.ymi_conv2d_nhwc_f32:
            continue
        d = args.contents
        p = (d.B, d.H, d.W, d.Cin, d.Cout, d.kh, d.kw, d.stride, d.pad, d.res_mode, d.nseg, d.Kpad, d.tile & 255,
             d.split_k if d.split_k > 1 else 0)
        found.append((name, p))
        assert p in params, (name, p)
        if d.res_mode == L.RES_BILINEAR:
            assert (d.res_H, d.res_W) == res_size(p[:12]), (name, d.res_H, d.res_W)
    print('timed plan: %d direct-conv launches, all covered: %s' % (len(found), found))
    assert len(found) >= 20
    assert {p[9] for _, p in found} >= {0, 1, 2}, found           # (its heads run on the Winograd path: tests/test_gpu_winograd_kat.py)
