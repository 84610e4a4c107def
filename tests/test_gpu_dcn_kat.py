"""Every DCNv2 kernel family against the independent fp64 reference of tests/dcn_ref.py (torch only: no oracle, no original code).

Families (ymi_dcn_v2_forward_f32):
  * the register-staged gather loader of csrc/conv_igemm.hip on its exact-fp32 basic tiles (what the outlier guard's `wide` path
    runs) and on their fp16x2 variants (| YMI_TILE_H2);
  * every block tile of the pipelined gather-GEMM of csrc/dcn.hip that takes a DCN (DCNP_ALL), unsplit and split-K.
Both offset / mask layouts: om_layout 0 (the reference's 18 offsets | 9 masks, ldo 27) and 1 (per tap [dh, dw, mask], ldo 32 with NaN
in the 5 padding channels, as engine.pack_offmask lays them out).

Known answers (shifted_conv_ref: per-tap integer shifts and their dyadic bilinear combinations), exact edge placements per pixel
with batch 3 (a read across an image boundary changes the answer by O(|x|)), sample points far outside, saturated and per-tap
modulation, ragged row / column tiles, split-K 2 / 3 / 6 / 9 with ranges that start inside a tap, and every DCN launch the tune
table ships (yolact_amd/tune/gfx950.json), rebuilt as the plan builds it.
"""
import json
import os

import pytest
import torch

from dcn_ref import const_offmask, dcn_ref, edge_offsets, fractional_taps, integer_taps, out_hw, shifted_conv_ref

pytestmark = pytest.mark.gpu

from yolact_amd import _lib as L  # noqa: E402
from yolact_amd import tune_table as TT  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RS_EXACT = sorted(L.BASIC_TILES)                                                   # register-staged loader, exact fp32
RS_H2 = [t | L.TILE_H2 for t in sorted(L.BASIC_TILES) if t in L.H2_BASE_TILES]   # ... its fp16x2 variants
DCNP_ALL = [t | L.TILE_H2 | L.TILE_DCNP for t in sorted(L.DCNP_TILES) if t not in L.DCNP_PLAIN_ONLY]   # csrc/dcn.hip
EXACT_BAR = 8e-6          # rel_err bar of the exact-fp32 tiles: ~4x the largest error measured over this file on MI355X (2.1e-6)
H2_BAR = 2e-5             # the suite's bar for the fp16x2 tiles
_MAX = {}                 # largest rel_err seen per (family, test) (printed at the end of the module)


def _family(tile):
    return 'dcnp' if tile & L.TILE_DCNP else 'rs_h2' if tile & L.TILE_H2 else 'rs_exact'


def _bar(tile):
    return H2_BAR if tile & L.TILE_H2 else EXACT_BAR


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    fams = sorted({f for f, _ in _MAX})
    print('\nDCN KAT largest rel_err per family: ' + ', '.join('%s %.2e' % (f, max(e for (g, _), e in _MAX.items() if g == f))
                                                              for f in fams))
    for (f, t), e in sorted(_MAX.items()):
        print('    %-8s %-40s %.2e' % (f, t, e))


def _check(y, ref, tile, test, what=''):
    from gpu_utils import rel_err
    assert y.shape == ref.shape
    assert torch.isfinite(y).all(), what
    e = rel_err(y.double(), ref)
    key = (_family(tile), test)
    _MAX[key] = max(_MAX.get(key, 0.0), e)
    assert e < _bar(tile), (what, L.TILE_NAMES.get(tile, tile), e)


def _launch(x, w, b, off, mask, stride, tile, layout, mask_is_prob=1, bn=None, act=L.ACT_NONE, split_k=0):
    """ymi_dcn_v2_forward_f32 through gpu_utils.run_conv with offsets [B,18,Ho,Wo] and mask channels [B,9,Ho,Wo] (probabilities
    or logits) laid out as om_layout `layout`."""
    from gpu_utils import run_conv
    if layout == 0:
        om = torch.cat([off, mask], 1)
    else:
        B, _, Ho, Wo = off.shape
        per_tap = torch.stack([off[:, 0::2], off[:, 1::2], mask], 2).reshape(B, 27, Ho, Wo)
        om = torch.cat([per_tap, torch.full((B, 5, Ho, Wo), float('nan'))], 1)
    return run_conv(x, w, b, bn, stride, 1, act=act, tile=tile, dcn_offmask=om, om_layout=layout, mask_is_prob=mask_is_prob,
                    split_k=split_k)


# ---- known answers on every tile of every family -----------------------------------------------------------------------------
SHAPES = {1: (3, 64, 13, 11, 36), 2: (3, 64, 14, 9, 36)}   # B, Cin, H, W, Cout: M = 429 / 105 rows, 36 columns: ragged for every tile
MASKS = (0.25, 1.0, 0.5, 0.0, 1.0, 0.25, 0.5, 1.0, 0.0)
FAR_TAPS = (0, 2, 4, 6, 8)                              # taps whose sample point is far outside in case 'far'


def _inputs(seed, stride):
    B, Cin, H, W, Co = SHAPES[stride]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Co, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5
    b = torch.randn(Co, generator=g) * 0.1
    return x, w, b, g, out_hw(H, W, stride, 1)


_CASES = {}


def _case(name):
    """(x, w, b, offset, mask channels, mask_is_prob, stride, expected fp64) of a named case, built once."""
    if name in _CASES:
        return _CASES[name]
    kind, stride = name.rsplit('/s', 1)
    stride = int(stride)
    x, w, b, g, (Ho, Wo) = _inputs(100 + CASES.index(name), stride)
    B, _, H, W = x.shape
    prob = 1
    if kind == 'integer':                 # a distinct (dh, dw) from {0, +-1, +-2, +-H, +-W} per tap, unit modulation
        taps = integer_taps(H, W)
        off, m = const_offmask(B, Ho, Wo, taps)
        ref = shifted_conv_ref(x, taps, w, b, stride, 1)
    elif kind == 'fractional':            # half- and quarter-integer offsets, per-tap modulation from {0, 0.25, 0.5, 1}
        taps = fractional_taps()
        off, m = const_offmask(B, Ho, Wo, taps, MASKS)
        ref = shifted_conv_ref(x, taps, w, b, stride, 1, MASKS)
    elif kind == 'edges':                 # per pixel: first / last rows and columns exactly on -1, -1+2^-10, -0.5, 0, n-1, ..., n
        off = edge_offsets(B, H, W, stride, 1, g, spread=1.5)
        m = torch.rand(B, 9, Ho, Wo, generator=g)
        ref = dcn_ref(x, off, m, w, b, stride, 1)
    elif kind == 'far':                   # +-1e4 and +-(H+W) on five taps: zero samples; the other taps integer shifts
        taps = integer_taps(H, W)
        far = dict(zip(FAR_TAPS, [(1e4, 0.0), (0.0, -1e4), (H + W, 1.0), (-1.0, -(H + W)), (-1e4, 1e4)]))
        off, m = const_offmask(B, Ho, Wo, [far.get(k, t) for k, t in enumerate(taps)])
        ref = shifted_conv_ref(x, [(0, 0) if k in far else t for k, t in enumerate(taps)], w, b, stride, 1,
                               [0.0 if k in far else 1.0 for k in range(9)])
    elif kind == 'logits':                # mask_is_prob = 0 with logits of +-40: the kernel's sigmoid saturates
        taps = fractional_taps()
        lg = [40.0, -40.0, 40.0, 40.0, -40.0, 40.0, -40.0, 40.0, 40.0]
        off, m = const_offmask(B, Ho, Wo, taps, lg)
        ref = shifted_conv_ref(x, taps, w, b, stride, 1, torch.sigmoid(torch.tensor(lg, dtype=torch.float64)).tolist())
        prob = 0
    else:
        raise KeyError(name)
    _CASES[name] = (x, w, b, off, m, prob, stride, ref)
    return _CASES[name]


CASES = ['integer/s1', 'integer/s2', 'fractional/s1', 'fractional/s2', 'edges/s1', 'edges/s2', 'far/s1', 'logits/s1']


@pytest.mark.parametrize('layout', [0, 1])
@pytest.mark.parametrize('tile', RS_EXACT + RS_H2 + DCNP_ALL, ids=lambda t: L.TILE_NAMES[t])
@pytest.mark.parametrize('case', CASES)
def test_dcn_kernel_known_answers(case, tile, layout):
    x, w, b, off, m, prob, stride, ref = _case(case)
    y = _launch(x, w, b, off, m, stride, tile, layout, mask_is_prob=prob)
    _check(y, ref, tile, 'known answers ' + case.split('/')[0], case)


# ---- split-K on the pipelined tiles --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('split', [2, 3, 6, 9])
@pytest.mark.parametrize('tile', DCNP_ALL, ids=lambda t: L.TILE_NAMES[t])
def test_dcn_pipelined_split_k_against_fp64(tile, split):
    """Cin = 160 (5 chunks per tap, 45 in all): the ranges of 23 / 15 / 8 / 5 chunks start inside a tap; random offsets of 2 to 4
    px, batch 2, 132 columns (ragged for 128- and 256-column tiles), layout 1 with NaN padding; bit-reproducible."""
    g = torch.Generator().manual_seed(7 + split)
    B, Cin, H, W, Co = 2, 160, 11, 13, 132
    Ho, Wo = out_hw(H, W, 1, 1)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Co, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5
    b = torch.randn(Co, generator=g) * 0.1
    sgn = torch.where(torch.rand(B, 18, Ho, Wo, generator=g) < 0.5, -1.0, 1.0)
    off = sgn * (2 + 2 * torch.rand(B, 18, Ho, Wo, generator=g))
    m = torch.rand(B, 9, Ho, Wo, generator=g)
    ref = torch.relu(dcn_ref(x, off, m, w, b, 1, 1))
    y = _launch(x, w, b, off, m, 1, tile, 1, act=L.ACT_RELU, split_k=split)
    _check(y, ref, tile, 'split-K', 'split %d' % split)
    from gpu_utils import run_conv
    amax = run_conv.last_amax[1]
    assert abs(amax - ref.abs().max().item()) <= H2_BAR * ref.abs().max().item()
    y2 = _launch(x, w, b, off, m, 1, tile, 1, act=L.ACT_RELU, split_k=split)
    assert torch.equal(y, y2)                                       # fixed summation order: bit-reproducible


# ---- every DCN launch the tune table ships ---------------------------------------------------------------------------------------
def _shipped():
    with open(os.path.join(ROOT, 'yolact_amd', 'tune', 'gfx950.json')) as f:
        entries = json.load(f)['entries']
    out = []
    for k, v in sorted(entries.items()):
        kind, key, mode = TT.parse(k)
        if kind == 'dcn' and mode == 'h2':
            out.append((key,) + TT.direct_parts(v))
    return out


SHIPPED = _shipped()
SHIPPED_SHAPES = sorted({key[1:] for key, _, _ in SHIPPED})


def _layer(key, seed):
    """A DCN layer of the plan (engine.Plan._resnet): DCN weight + bias, its BatchNorm folded by Packed, ReLU, with offsets of
    N(0, 2^2) px and mask logits of N(0, 1).  Returns (x, weight, bias, bn, offset, logits, stride, expected fp64)."""
    import torch.nn as nn
    B, H, W, Cin, Co, kh, kw, stride, pad, res_mode, nseg, Kpad, tag = key
    assert (kh, kw, pad, res_mode, nseg, Kpad, tag) == (3, 3, 1, 0, 1, 9 * Cin, 'dcn')
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Co, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5
    b = torch.randn(Co, generator=g) * 0.1
    bn = nn.BatchNorm2d(Co).eval()
    with torch.no_grad():
        bn.weight.copy_(1 + 0.2 * torch.randn(Co, generator=g))
        bn.bias.copy_(0.2 * torch.randn(Co, generator=g))
        bn.running_mean.copy_(0.2 * torch.randn(Co, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(Co, generator=g))
    Ho, Wo = out_hw(H, W, stride, 1)
    off = 2.0 * torch.randn(B, 18, Ho, Wo, generator=g)
    logits = torch.randn(B, 9, Ho, Wo, generator=g)
    y = dcn_ref(x, off, torch.sigmoid(logits.double()), w, b, stride, 1)
    sc = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
    y = (y - bn.running_mean.double().view(1, -1, 1, 1)) * sc.view(1, -1, 1, 1) + bn.bias.double().view(1, -1, 1, 1)
    return x, w, b, bn, off, logits, stride, torch.relu(y)


def _run_layer(key, tile, split_k, seed, test):
    from gpu_utils import run_conv
    x, w, b, bn, off, logits, stride, ref = _layer(key, seed)
    y = _launch(x, w, b, off, logits, stride, tile, 1, mask_is_prob=0, bn=bn, act=L.ACT_RELU, split_k=split_k)
    _check(y, ref, tile, test, str(key))
    amax = run_conv.last_amax[1]
    assert abs(amax - ref.abs().max().item()) <= _bar(tile) * ref.abs().max().item(), (amax, ref.abs().max().item())


def test_shipped_table_has_dcn_launches():
    """The sweep below is read from the table: it must find the DCN layers of YOLACT++ (6 shapes, each at B = 1, 2 and 8)."""
    assert len(SHIPPED) >= 18 and len(SHIPPED_SHAPES) >= 6


def _shape_id(key):
    B, H, W, Cin, Co, stride = key[:5] + key[7:8]
    return 'B%d-%dx%d-%dto%d-s%d' % (B, H, W, Cin, Co, stride)


@pytest.mark.parametrize('key,tile,split_k', SHIPPED, ids=['%s-%s-k%d' % (_shape_id(k), L.TILE_NAMES[t], s) for k, t, s in SHIPPED])
def test_dcn_shipped_launch(key, tile, split_k):
    """One DCN launch of the table, as the plan makes it: tile = value & 255, split_k = value >> 8, om_layout 1, ldo 32."""
    _run_layer(key, tile, split_k, 1000 + key[0] * 7 + key[3], 'shipped launches')


@pytest.mark.parametrize('tile', RS_EXACT, ids=lambda t: L.TILE_NAMES[t])
@pytest.mark.parametrize('shape', SHIPPED_SHAPES, ids=lambda s: _shape_id((2,) + s))
def test_dcn_shipped_shape_on_exact_tiles(shape, tile):
    """The outlier guard can move any DCN layer onto the exact-fp32 basic tiles of the register-staged loader: each shipped shape
    at B = 2 on every one of them."""
    _run_layer((2,) + shape, tile, 0, 2000 + shape[2], 'shipped shapes')
