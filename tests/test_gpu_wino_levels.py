"""ymi_wino_desc.nlev: one F(4x4) fp16x2 Winograd layer (input transform, grouped GEMM, output transform: three launches) for
several feature maps that share their filters — the P4..P7 prediction heads.

The level form promises to do, for every level, exactly what the single-level launch does for that level's geometry, so the kernel
tests here are BIT comparisons against the per-level launches with the same GEMM tile and the same magnitude bound; only the scale
test (levels of different magnitude under one power-of-two scale) compares against fp64, with the F(4x4) fp16x2 bar of
tests/test_gpu_winograd_kat.py.  Shapes: B = 2, C = 64 — partial tiles, a level smaller than one tile, level boundaries inside one
128-row GEMM tile, and (35 x 35, 18 x 18) for a 128-row boundary inside a level and T = 212 rows in all.

Scale test, measured on MI355X (max |y - fp64| / max |fp64| per level, levels 2^0, 2^-6, 2^-12, 2^-6 under one scale; bar 4e-5):
4.15e-6, 3.84e-6, 1.31e-6, 5.26e-7, the same on 128x128h2 with either V form and on wg128x256h2.  Plan test: loc / conf / coef of the
merged plan within 1.9e-6 / 1.9e-6 / 5.3e-6 of the per-level plan's maximum (bar 2e-5).
"""
import ctypes as C
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from yolact_amd import _lib as L  # noqa: E402

DEV = torch.device('cuda')
B, CIN = 2, 64
H2_128 = L.TILE_128x128 | L.TILE_H2
WG = L.TILE_WG_128x256 | L.TILE_H2
SLOT = L.AMAX_SLOT_FLOATS
EARG = -1
LEVELS = ((9, 9), (5, 5), (3, 3), (2, 2))


def _packed(weight, bias):
    from yolact_amd.engine import Packed, WinoPacked
    return Packed(weight, bias, None, 1, 1, None, DEV), WinoPacked(weight, DEV, 4)


def _inputs(levels, g, mags=None):
    xs = [torch.randn(B, h, w, CIN, generator=g) * (1.0 if mags is None else mags[i]) for i, (h, w) in enumerate(levels)]
    return [x.to(DEV).contiguous() for x in xs]


def _tiles(levels):
    return sum(B * ((h + 3) // 4) * ((w + 3) // 4) for h, w in levels)


class Launch:
    """One ymi_wino_desc over `levels` (one level: the plain launch, nlev = 0) with everything it points at kept alive."""

    def __init__(self, xs, levels, pk, wp, Cout, tile, planes, act=L.ACT_RELU, x_slots=None, segs=None, seg_bufs=None, seg_offs=None,
                 force_table=False):
        n = len(levels)
        T = _tiles(levels)
        self.V = torch.empty(36 * T * CIN, device=DEV)
        self.M = torch.empty(36 * T * ((Cout + 3) // 4 * 4), device=DEV)
        self.ys = [torch.full((B, h, w, Cout), float('nan'), device=DEV) for h, w in levels] if segs is None else None
        self.amax = torch.zeros((n + 4) * SLOT, device=DEV)          # [0..n): y_amax per level (dense) / per segment; [n+3]: lev_amax
        self.keep = (xs, pk, wp, x_slots, seg_bufs)
        d = self.d = L.WinoDesc()
        d.u, d.V, d.M = wp.u.data_ptr(), self.V.data_ptr(), self.M.data_ptr()
        d.scale = pk.scale.data_ptr() if pk.scale is not None else None
        d.bias = pk.bias.data_ptr() if pk.bias is not None else None
        up, uinv = wp.h2()
        d.u_h2, d.uinv_h2, d.v_planes = up.data_ptr(), uinv.data_ptr(), planes
        d.B, d.C, d.Cout, d.act, d.tile, d.m = B, CIN, Cout, act, tile, 4
        if segs is not None:
            d.nseg = len(segs)
            for k, ((n0, n1, sact), buf) in enumerate(zip(segs, seg_bufs)):
                d.seg[k] = L.ConvSeg(n0, n1, sact, n1 - n0, buf.shape[1] * buf.shape[2], buf.data_ptr())
            d.y_amax = self.amax.data_ptr()
        if n == 1 and not force_table:
            (h, w), = levels
            d.x, d.H, d.W, d.x_amax = xs[0].data_ptr(), h, w, x_slots[0].data_ptr()
            if segs is None:
                d.y, d.y_amax = self.ys[0].data_ptr(), self.amax.data_ptr()
            else:
                for k in range(d.nseg):
                    d.seg[k].ptr += seg_offs[0][k]
            return
        d.nlev = n
        d.lev_amax = self.amax.data_ptr() + (n + 3) * SLOT * 4
        for l, (h, w) in enumerate(levels):
            lv = d.lev[l]
            lv.x, lv.x_amax, lv.H, lv.W = xs[l].data_ptr(), x_slots[l].data_ptr(), h, w
            if segs is None:
                lv.y, lv.y_amax = self.ys[l].data_ptr(), self.amax.data_ptr() + l * SLOT * 4
            else:
                for k in range(d.nseg):
                    lv.seg_off[k] = seg_offs[l][k]

    def run(self):
        rc = L.lib().ymi_conv3x3_winograd_f32(C.byref(self.d), L.stream_ptr())
        torch.cuda.synchronize()
        return rc

    def bound(self, slot):
        return float(self.amax[slot * SLOT:(slot + 1) * SLOT].max())


def _slot(value):
    s = torch.zeros(SLOT, device=DEV)
    s[0] = value
    return s


def _bits(t):
    return t.contiguous().view(torch.int32)


def _dense_case(levels, Cout, tile, planes, seed):
    g = torch.Generator().manual_seed(seed)
    w, b = torch.randn(Cout, CIN, 3, 3, generator=g) * 0.05, torch.randn(Cout, generator=g) * 0.1
    pk, wp = _packed(w, b)
    xs = _inputs(levels, g)
    slot = _slot(max(float(x.abs().max()) for x in xs))          # every level names the same slot, holding the true maximum
    merged = Launch(xs, levels, pk, wp, Cout, tile, planes, x_slots=[slot] * len(levels))
    assert merged.run() == 0
    for l, lv in enumerate(levels):
        one = Launch([xs[l]], [lv], pk, wp, Cout, tile, planes, x_slots=[slot])
        assert one.run() == 0
        assert torch.isfinite(one.ys[0]).all()
        assert torch.equal(_bits(merged.ys[l]), _bits(one.ys[0])), (l, lv)
        assert merged.bound(l) == one.bound(0) > 0.0, (l, lv)
    return merged, xs, (w, b)


@pytest.mark.parametrize('tile,planes,Cout', [(H2_128, 1, 64), (H2_128, 0, 64), (WG, 1, 256)],
                         ids=['128x128h2-planes', '128x128h2-fp32V', 'wg128x256h2'])
def test_dense_levels_equal_the_single_launches(tile, planes, Cout):
    _dense_case(LEVELS, Cout, tile, planes, seed=1)


def test_levels_across_several_row_tiles():
    levels = ((35, 35), (18, 18))
    assert _tiles(levels) == 212
    _dense_case(levels, 64, H2_128, 1, seed=2)


def test_segment_levels_equal_the_single_launches_and_leave_the_guard_rows():
    A, D, Ccls = 3, 32, 84
    n_b, n_m, n_c = A * 4, A * D, A * Ccls
    Cout = n_b + n_m + n_c
    assert Cout == 360
    g = torch.Generator().manual_seed(3)
    w, b = torch.randn(Cout, CIN, 3, 3, generator=g) * 0.05, torch.randn(Cout, generator=g) * 0.1
    pk, wp = _packed(w, b)
    xs = _inputs(LEVELS, g)
    slot = _slot(max(float(x.abs().max()) for x in xs))
    guard = 5                                                     # rows (priors) before, between and after the levels
    offs, p = [], guard
    for h, w_ in LEVELS:
        offs.append(p)
        p += h * w_ * A + guard
    P = p
    widths = (4, D, Ccls)
    segs = [(0, n_b, L.ACT_NONE), (n_b, n_b + n_m, L.ACT_TANH), (n_b + n_m, Cout, L.ACT_NONE)]
    seg_offs = [[off * k * 4 for k in widths] for off in offs]    # bytes

    def bufs():
        return [torch.full((B, P, k), float('nan'), device=DEV) for k in widths]
    mb = bufs()
    merged = Launch(xs, LEVELS, pk, wp, Cout, H2_128, 1, x_slots=[slot] * 4, segs=segs, seg_bufs=mb, seg_offs=seg_offs)
    assert merged.run() == 0
    sb = bufs()
    amax = torch.zeros(3)
    for l, lv in enumerate(LEVELS):
        one = Launch([xs[l]], [lv], pk, wp, Cout, H2_128, 1, x_slots=[slot], segs=segs, seg_bufs=sb, seg_offs=[seg_offs[l]])
        assert one.run() == 0
        amax = torch.maximum(amax, torch.tensor([one.bound(k) for k in range(3)]))
    for k in range(3):
        assert torch.equal(_bits(mb[k]), _bits(sb[k])), k         # NaN guard rows included: same bits
        assert merged.bound(k) == float(amax[k]) > 0.0
        written = torch.zeros(P, dtype=torch.bool)
        for off, (h, w_) in zip(offs, LEVELS):
            written[off:off + h * w_ * A] = True
        rows = mb[k].cpu()
        assert torch.isfinite(rows[:, written]).all()
        assert torch.isnan(rows[:, ~written]).all() and int((~written).sum()) == 5 * guard


def test_no_table_is_the_plain_launch():
    g = torch.Generator().manual_seed(4)
    w, b = torch.randn(64, CIN, 3, 3, generator=g) * 0.05, torch.randn(64, generator=g) * 0.1
    pk, wp = _packed(w, b)
    xs = _inputs(((9, 9),), g)
    slot = _slot(float(xs[0].abs().max()))
    plain = Launch(xs, [(9, 9)], pk, wp, 64, H2_128, 1, x_slots=[slot])
    assert plain.run() == 0
    filled = Launch(xs, [(9, 9)], pk, wp, 64, H2_128, 1, x_slots=[slot])
    filled.d.lev[0].H = filled.d.lev[0].W = 7                     # nlev = 0: the table is not looked at
    filled.d.lev[0].x = filled.d.lev_amax = slot.data_ptr()
    assert filled.run() == 0
    assert torch.equal(_bits(plain.ys[0]), _bits(filled.ys[0])) and plain.bound(0) == filled.bound(0)
    from gpu_utils import run_wino, nchw
    y = run_wino(nchw(xs[0].cpu()), w, b, act=L.ACT_RELU, tile=H2_128, m=4, v_planes=True)
    assert torch.equal(_bits(nchw(plain.ys[0].cpu())), _bits(y))


def test_rejected_descriptors():
    g = torch.Generator().manual_seed(5)
    w, b = torch.randn(64, CIN, 3, 3, generator=g) * 0.05, None
    pk, wp = _packed(w, b)
    levels = LEVELS[:2]
    xs = _inputs(levels, g)
    slot = _slot(4.0)

    def fresh():
        return Launch(xs, levels, pk, wp, 64, H2_128, 1, x_slots=[slot] * 2)
    assert fresh().run() == 0
    for what in ('m2', 'x_up', 'proj', 'nlev1', 'nlev6', 'zero'):
        la = fresh()
        if what == 'm2':
            la.d.m = 2
        elif what == 'x_up':
            la.d.x_up = xs[0].data_ptr()
        elif what == 'proj':
            la.d.proj_w_h2 = xs[0].data_ptr()
        elif what == 'nlev1':
            la.d.nlev = 1
        elif what == 'nlev6':
            la.d.nlev = 6
        else:
            la.d.lev[1].H = 0
        assert la.run() == EARG, what
        assert all(torch.isnan(y).all() for y in la.ys), what


def test_levels_of_different_magnitude_under_one_scale():
    """Levels 2^6 apart, each with its own bound slot: the input transform takes the largest bound, publishes it, and the GEMM
    un-scales by the published value.  Bar: F(4x4) fp16x2 of the fp64 pin, per level, relative to that level's own maximum."""
    from test_gpu_winograd_kat import BARS
    bar = BARS[4, 'h2']
    mags = (1.0, 2.0 ** -6, 2.0 ** -12, 2.0 ** -6)
    g = torch.Generator().manual_seed(6)
    w = torch.randn(64, CIN, 3, 3, generator=g) * 0.05
    pk, wp = _packed(w, None)
    xs = _inputs(LEVELS, g, mags)
    slots = [_slot(float(x.abs().max())) for x in xs]
    for tile, planes in ((H2_128, 1), (H2_128, 0), (WG, 1)):
        la = Launch(xs, LEVELS, pk, wp, 64, tile, planes, act=L.ACT_NONE, x_slots=slots)
        assert la.run() == 0
        assert la.bound(len(LEVELS) + 3) == max(float(s.max()) for s in slots)       # the published bound
        errs = []
        for x, y in zip(xs, la.ys):
            ref = F.conv2d(x.cpu().double().permute(0, 3, 1, 2), w.double(), padding=1).permute(0, 2, 3, 1)
            errs.append(float((y.cpu().double() - ref).abs().max() / ref.abs().max()))
        print('wino levels scale test %s planes %d: max rel err per level %s (bar %.0e)'
              % (L.TILE_NAMES.get(tile), planes, ' '.join('%.2e' % e for e in errs), bar))
        assert max(errs) < bar, (L.TILE_NAMES.get(tile), planes, errs, bar)


# ---- the plan -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def plan_runs():
    """configs[1] at B = 2, 550 x 550: (loc, conf, coef, classes per image) with the merge installed (two runs) and without.
    Tiles come from the shipped table or, for this batch size, the library's heuristic (no measuring: the test is about results)."""
    import yolact_amd
    from yolact_amd.utils.synth import synth_images, synth_state_dict
    yolact_amd.set_cfg('yolact_resnet50_config')
    from yolact_amd.yolact import Yolact
    x = synth_images(2, 550, 550, seed=1234).to(DEV)
    out = {}
    names = ('YOLACT_AMD_MERGE_LEVELS', 'YOLACT_AMD_AUTOTUNE')
    old = {k: os.environ.get(k) for k in names}
    try:
        os.environ['YOLACT_AMD_AUTOTUNE'] = 'table'
        for mode in ('force', '0'):
            os.environ['YOLACT_AMD_MERGE_LEVELS'] = mode
            net = Yolact()
            net.load_state_dict_compat(synth_state_dict([(k, tuple(v.shape)) for k, v in net.state_dict().items()], seed=0,
                                                        conf_gain=0.04))
            net.detect.use_fast_nms = True
            net = net.to(DEV).eval()
            runs = []
            with torch.no_grad():
                for _ in range(2):
                    dets = net(x)
                    torch.cuda.synchronize()
                    plan = net.plan_for(x)
                    runs.append((plan.loc.clone().cpu(), plan.conf.clone().cpu(), plan.coef.clone().cpu(),
                                 [d['detection']['class'].cpu() if d['detection'] is not None else torch.zeros(0) for d in dets]))
            out[mode] = (runs, [(fn if isinstance(fn, str) else fn.__name__, name) for fn, _, name, _ in plan.ops], plan.merged_levels)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return out


def test_plan_with_merged_levels_matches_the_per_level_plan(plan_runs):
    (m1, m2), ops, merged = plan_runs['force']
    (p1, _), pops, pmerged = plan_runs['0']
    assert merged and not pmerged
    for a, b_, name in zip(m1[:3], p1[:3], ('loc', 'conf', 'coef')):
        e = float((a - b_).abs().max() / b_.abs().max())
        print('merged levels vs per-level plan: %s max diff / max = %.2e' % (name, e))
        assert e < 2e-5, (name, e)
    assert [len(c) for c in m1[3]] == [len(c) for c in p1[3]]
    assert all(torch.equal(a, b_) for a, b_ in zip(m1[3], p1[3]))
    for a, b_ in zip(m1[:3], m2[:3]):
        assert torch.equal(_bits(a), _bits(b_))                   # two runs: the same bits
    heads = [(fn, name) for fn, name in ops if name.startswith(('head1.', 'head2.', 'head3.', 'head4.'))]
    wino = [name for fn, name in heads if fn == 'ymi_conv3x3_winograd_f32']
    assert len(wino) == 2 and wino[0].startswith('head1.up0') and wino[1].startswith('head1.out'), heads
    assert all(fn == 'nop' for fn, name in heads if not name.startswith('head1.')), heads
    assert len([1 for fn, name in pops if name.startswith(('head2.', 'head3.', 'head4.')) and fn != 'nop']) == 6
