"""The lincomb mask loss on the GPU (csrc/mask_loss.hip, ymi_mask_loss_f32, yolact_amd/layers/mask_loss.py) against the fp64 oracle.

Oracle: tests/mask_loss_ref.py in fp64 (pinned to the reference's own result by tests/test_mask_loss_host.py).
Bar: per case and per tensor (loss, loss_inst, d_proto, d_coef), rel_err against the oracle <= max(4 * rel_err(the same formulation
in fp32 on the CPU, fp64), EXACT_BAR).  The factor 4 is for another reduction order and the device's exp / log; EXACT_BAR = 8e-6 is
the project's exact-fp32 bar (tests/test_gpu_dcn_kat.py).

Inputs are CONSTRUCTED off the discontinuities: every box edge times the mask size has a fractional part in [1/8, 7/8], the fp32
and fp64 crop windows are asserted equal for every instance, and the coefficients are scaled so that max |x| <= 12 (asserted).  No
element is excluded from any comparison.  The largest rel_err per case and tensor is printed at the end of the module (the table
of DESIGN.md 5.2).
"""
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gpu_utils import rel_err  # noqa: E402
from helpers import same_bits  # noqa: E402
from mask_loss_ref import inside_masks, logits, mask_loss_ref_grads  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EXACT_BAR = 8e-6
ALPHA = 6.125
NAMES = ('loss', 'loss_inst', 'd_proto', 'd_coef')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_MAX = {}
_REFS = {}


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    print('\nlincomb mask loss: rel_err against the fp64 oracle (bar)')
    for case in sorted(_MAX):
        print('  %-30s ' % case + '  '.join('%s %.2e (%.1e)' % (n, e, b) for n, (e, b) in _MAX[case].items()))


def _g(seed):
    return torch.Generator().manual_seed(seed)


def off_grid(v, size, g):
    """Relative coordinates whose product with `size` is (an integer) + a fraction in [1/4, 3/4]."""
    cell = torch.floor(v * size)
    return (cell + 0.25 + 0.5 * torch.rand(v.shape, generator=g)) / size


def assert_constructed(box, mh, mw):
    """Every edge off the pixel grid by at least 1/8 in fp32, and the fp32 and fp64 crop windows select the same pixels."""
    for cols, size in (((0, 2), mw), ((1, 3), mh)):
        prod = box[:, cols] * size                    # fp32, as the kernel forms it
        fr = prod - torch.floor(prod)
        assert fr.min().item() >= 1 / 8 and fr.max().item() <= 7 / 8
    assert torch.equal(inside_masks(box, mh, mw, torch.float32), inside_masks(box, mh, mw, torch.float64))


def scale_logits(proto, coef, img_off, xmax):
    x = logits(proto, coef, img_off)
    coef = coef * (xmax / x.abs().max().item())
    return coef, logits(proto, coef, img_off).abs().max().item()


def make_case(mh, mw, ns, seed, xmax=10.0, boxes=None):
    """-> dict of CPU tensors: proto, coef, box, gt, gt_idx, img_off, weight."""
    g = _g(seed)
    B, N = len(ns), sum(ns)
    proto = torch.relu(torch.randn(B, mh, mw, 32, generator=g)) * 0.5
    coef = torch.tanh(torch.randn(N, 32, generator=g))
    yy = (torch.arange(mh).float() + 0.5).view(1, mh, 1) / mh
    xx = (torch.arange(mw).float() + 0.5).view(1, 1, mw) / mw
    gts, gidx, bxs, wts, off = [], [], [], [], [0]
    row0 = 0
    for b, n in enumerate(ns):
        n_gt = 3 + b
        c = 0.2 + 0.6 * torch.rand(n_gt, 2, generator=g)
        half = 0.08 + 0.25 * torch.rand(n_gt, 2, generator=g)
        gbox = torch.cat([c - half, c + half], 1).clamp(0.01, 0.99)
        cx, cy = ((gbox[:, 0] + gbox[:, 2]) / 2).view(-1, 1, 1), ((gbox[:, 1] + gbox[:, 3]) / 2).view(-1, 1, 1)
        rx, ry = ((gbox[:, 2] - gbox[:, 0]) / 2).view(-1, 1, 1), ((gbox[:, 3] - gbox[:, 1]) / 2).view(-1, 1, 1)
        gts.append((((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2 <= 1.0).to(torch.uint8))
        idx = torch.randint(0, n_gt, (n,), generator=g)
        if n >= 2:
            idx[1] = idx[0]                           # two instances share one GT row
        gidx.append(idx.to(torch.int32) + row0)
        jit = gbox[idx] + 0.03 * torch.randn(n, 4, generator=g)
        bxs.append(torch.stack([off_grid(jit[:, 0], mw, g), off_grid(jit[:, 1], mh, g),
                                off_grid(jit[:, 2], mw, g), off_grid(jit[:, 3], mh, g)], 1))
        wts.append(torch.full((n,), 1.0 + 0.3 * b))
        off.append(off[-1] + n)
        row0 += n_gt
    box = torch.cat(bxs) if boxes is None else boxes
    img_off = torch.tensor(off, dtype=torch.int32)
    if N:
        coef, top = scale_logits(proto, coef, img_off, xmax)
        assert xmax > 12 or top <= 12
        assert_constructed(box, mh, mw)
    return dict(proto=proto, coef=coef, box=box, gt=torch.cat(gts), gt_idx=torch.cat(gidx), img_off=img_off, weight=torch.cat(wts))


ORDER = ('proto', 'coef', 'box', 'gt', 'gt_idx', 'img_off', 'weight')


def gpu_terms(case, crop=True, roi_norm=True):
    from yolact_amd.layers.mask_loss import mask_loss_terms
    out = mask_loss_terms(*[case[k].to(DEV) for k in ORDER], crop=crop, roi_norm=roi_norm, alpha=ALPHA)
    torch.cuda.synchronize()
    return [o.cpu() for o in out]


def refs(key, case, crop=True, roi_norm=True):
    """(fp64 oracle, fp32 yardstick), computed once per (case, switches)."""
    k = (key, crop, roi_norm)
    if k not in _REFS:
        args = [case[n] for n in ORDER]
        _REFS[k] = tuple(mask_loss_ref_grads(*args, crop, roi_norm, ALPHA, dtype=dt) for dt in (torch.float64, torch.float32))
    return _REFS[k]


def check(name, got, r64, r32):
    row = _MAX.setdefault(name, {})
    bad = []
    for n, a, b64, b32 in zip(NAMES, got, r64, r32):
        a, b64, b32 = a.double().reshape(-1), b64.double().reshape(-1), b32.double().reshape(-1)
        assert a.shape == b64.shape, n
        bar = max(4 * rel_err(b32, b64), EXACT_BAR)
        e = rel_err(a, b64)
        row[n] = (e, bar)
        print('%s %s: rel_err %.3e bar %.3e' % (name, n, e, bar))
        if not e <= bar:
            bad.append((n, e, bar))
    assert not bad, (name, bad)


CASES = {}


def case(key):
    if key not in CASES:
        CASES[key] = {'12x10': lambda: make_case(12, 10, (3,), 101),
                      '35x37': lambda: make_case(35, 37, (5, 0, 70), 102),
                      '138x138': lambda: make_case(138, 138, (100, 37), 103),
                      '12x10_n330': lambda: make_case(12, 10, (330, 9), 104)}[key]()
    return CASES[key]


def test_one_tile_narrower_than_a_wave_row():
    c = case('12x10')
    check('12x10 n3', gpu_terms(c), *refs('12x10', c))


@pytest.mark.parametrize('crop', [True, False])
@pytest.mark.parametrize('roi_norm', [True, False])
def test_ragged_tiles_and_an_image_without_positives(crop, roi_norm):
    c = case('35x37')
    assert c['gt_idx'][0] == c['gt_idx'][1]
    got = gpu_terms(c, crop, roi_norm)
    check('35x37 n5,0,70 crop%d roi%d' % (crop, roi_norm), got, *refs('35x37', c, crop, roi_norm))
    assert torch.equal(got[2][1], torch.zeros_like(got[2][1]))          # the image without positives


def test_shipped_geometry():
    c = case('138x138')
    check('138x138 n100,37', gpu_terms(c), *refs('138x138', c))


def test_more_instances_than_one_lds_round():
    """330 instances in one image: the coefficient rows are staged in two rounds (320 fit at once)."""
    c = case('12x10_n330')
    check('12x10 n330,9', gpu_terms(c), *refs('12x10_n330', c))


def edge_boxes():
    mw, mh = 37.0, 35.0
    return torch.tensor([
        [-0.5 / mw, -0.5 / mh, 37.5 / mw, 35.5 / mh],      # the full image: both clamps active on both axes
        [24.5 / mw, 5.75 / mh, 8.5 / mw, 20.25 / mh],      # reversed (b2 < b0)
        [0.5 / mw, 0.5 / mh, 36.5 / mw, 34.5 / mh],        # the padding crosses the border
        [10.3 / mw, 4.5 / mh, 10.7 / mw, 30.5 / mh],       # narrower than one pixel
        [1.5 / mw, 1.5 / mh, 6.5 / mw, 5.5 / mh],          # disjoint from its GT (placed bottom right below)
    ])


def edge_case():
    if 'edges' not in CASES:
        c = make_case(35, 37, (5,), 105, boxes=edge_boxes())
        gt = c['gt'].clone()
        gt[2] = 0
        gt[2, 25:33, 27:36] = 1
        gt_idx = c['gt_idx'].clone()
        gt_idx[4] = 2
        assert not (inside_masks(c['box'], 35, 37, torch.float64)[4] & gt[2].bool()).any()
        c.update(gt=gt, gt_idx=gt_idx)
        CASES['edges'] = c
    return CASES['edges']


def test_box_edges():
    c = edge_case()
    ins = inside_masks(c['box'], 35, 37, torch.float64)
    assert ins[0].all() and ins[3].sum().item() == 2 * 28 and ins[2].all()
    got = gpu_terms(c)
    check('35x37 box edges', got, *refs('edges', c))
    assert got[1][1].item() < 0                                         # the reversed box: its width, hence its L_j, is negative
    got = gpu_terms(c, True, False)
    check('35x37 box edges roi0', got, *refs('edges', c, True, False))


def test_closed_form_with_zero_prototypes():
    """proto = 0, so p = 1/2 everywhere: L_j = (#inside) ln 2 + 100 (#GT pixels outside), from integer counts."""
    for key, c in (('35x37', case('35x37')), ('edges', edge_case())):
        c = dict(c, proto=torch.zeros_like(c['proto']))
        mh, mw = c['proto'].shape[1:3]
        ins = inside_masks(c['box'], mh, mw, torch.float64)
        t = c['gt'][c['gt_idx'].long()].bool()
        want = ins.sum(dim=(1, 2)).double() * math.log(2.0) + 100.0 * (t & ~ins).sum(dim=(1, 2)).double()
        loss, inst, dproto, dcoef = gpu_terms(c, True, False)
        e = rel_err(inst.double(), want)
        _MAX.setdefault('closed form ' + key, {})['loss_inst'] = (e, EXACT_BAR)
        assert e <= EXACT_BAR, (key, e)
        total = (want * c['weight'].double()).sum().item() * ALPHA / mh / mw
        assert abs(loss.item() - total) <= EXACT_BAR * abs(total)
        assert torch.equal(dcoef, torch.zeros_like(dcoef))              # sum of g * proto[k] with proto = 0


def _golden(name):
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'mask_loss.npz'))
    meta = json.loads(bytes(z['meta']).decode())
    m = next(c for c in meta['cases'] if c['name'] == name)
    t = {k: torch.from_numpy(z['%s_%s' % (name, k)]) for k in ('proto', 'mask_data', 'pos', 'idx_t', 'gt_box_t')}
    t['masks'] = [torch.from_numpy(z['%s_masks_%d' % (name, b)]).float() for b in range(len(m['ns']))]
    t['select'] = {b: torch.from_numpy(z['%s_select_%d' % (name, b)]) for b in m['over_cap']}
    return meta, m, t


def test_wrapper_draws_the_reference_subset_over_the_cap(monkeypatch):
    import yolact_amd
    from yolact_amd.layers import mask_loss as ML
    meta, m, t = _golden('overcap12x10')
    assert m['ns'] == [130] and meta['masks_to_train'] == 100
    cfg = yolact_amd.CONFIGS['yolact_base_config'].copy()
    monkeypatch.setattr(ML, 'active_cfg', lambda: cfg)
    dev = lambda v: [u.to(DEV) for u in v] if isinstance(v, list) else v.to(DEV)
    # the same gathering on the CPU, seeded alike: the oracle's inputs on the drawn subset
    torch.manual_seed(meta['torch_seed'])
    coef, box, gt, gt_idx, img_off, weight, selects = ML.gather_instances(t['pos'], t['idx_t'], t['mask_data'], t['masks'],
                                                                          t['gt_box_t'], 12, 10, cfg.masks_to_train)
    assert torch.equal(selects[0], t['select'][0])                       # the golden's select is drawn
    assert coef.shape[0] == 100 and torch.equal(weight, torch.full((100,), np.float32(130 / 100)))
    assert logits(t['proto'], coef, img_off).abs().max().item() <= 12
    assert torch.equal(inside_masks(box, 12, 10, torch.float32), inside_masks(box, 12, 10, torch.float64))
    proto = t['proto'].to(DEV).requires_grad_(True)
    mask_data = t['mask_data'].to(DEV).requires_grad_(True)
    torch.manual_seed(meta['torch_seed'])
    out = ML.lincomb_mask_loss(dev(t['pos']), dev(t['idx_t']), mask_data, proto, dev(t['masks']), dev(t['gt_box_t']))
    assert set(out) == {'M'} and out['M'].dim() == 0
    out['M'].backward()
    torch.cuda.synchronize()
    rows = torch.nonzero(t['pos'][0]).squeeze(1)[selects[0]]             # prior of each gathered instance
    got_dcoef = mask_data.grad.cpu()[0, rows]
    untouched = torch.ones(t['pos'].shape[1], dtype=torch.bool)
    untouched[rows] = False
    assert torch.equal(mask_data.grad.cpu()[0, untouched], torch.zeros(int(untouched.sum()), 32))
    r64, r32 = (mask_loss_ref_grads(t['proto'], coef, box, gt, gt_idx, img_off, weight, True, True, float(cfg.mask_alpha), dtype=dt)
                for dt in (torch.float64, torch.float32))
    got = [out['M'].detach().cpu(), r64[1].float(), proto.grad.cpu(), got_dcoef]      # (loss_inst is not a wrapper output)
    check('wrapper 12x10 n130 -> 100', got, r64, r32)
    del _MAX['wrapper 12x10 n130 -> 100']['loss_inst']


def test_autograd_scaling_and_requires_grad_subsets():
    from yolact_amd.layers.mask_loss import mask_loss
    c = case('35x37')
    rest = [c[k].to(DEV) for k in ORDER[2:]]

    def run(scale, need_proto, need_coef=True):
        proto, coef = c['proto'].to(DEV).requires_grad_(need_proto), c['coef'].to(DEV).requires_grad_(need_coef)
        loss = mask_loss(proto, coef, *rest, alpha=ALPHA)
        (scale * loss).backward()
        return loss.detach(), proto.grad, coef.grad

    l1, p1, c1 = run(1.0, True)
    l2, p2, c2 = run(0.5, True)
    assert torch.equal(l1, l2) and torch.equal(p2 * 2, p1) and torch.equal(c2 * 2, c1)
    l3, p3, c3 = run(1.0, False)
    assert p3 is None and torch.equal(l3, l1) and torch.equal(c3, c1)
    l4, p4, c4 = run(1.0, True, False)
    assert c4 is None and torch.equal(l4, l1) and torch.equal(p4, p1)
    # the same launch as gpu_terms, which test_ragged_tiles_and_an_image_without_positives holds to the bar
    t = gpu_terms(c)
    assert torch.equal(l1.cpu().view(1), t[0]) and torch.equal(p1.cpu(), t[2]) and torch.equal(c1.cpu(), t[3])


def test_no_instances_at_all():
    from yolact_amd.layers.mask_loss import mask_loss
    c = make_case(12, 10, (0, 0), 106)
    proto, coef = c['proto'].to(DEV).requires_grad_(True), c['coef'].to(DEV).requires_grad_(True)
    loss = mask_loss(proto, coef, *[c[k].to(DEV) for k in ORDER[2:]], alpha=ALPHA)
    loss.backward()
    assert loss.item() == 0.0 and tuple(coef.grad.shape) == (0, 32)
    assert torch.equal(proto.grad, torch.zeros_like(proto))


def abi_call(c, fill=float('nan')):
    """ymi_mask_loss_f32 directly, every output pre-filled."""
    from yolact_amd import _lib as L
    d = L.MaskLossDesc()
    ins = {k: c[k].to(DEV).contiguous() for k in ORDER}
    B, mh, mw, K = c['proto'].shape
    N = c['coef'].shape[0]
    outs = [torch.full(s, fill, device=DEV) for s in ((1,), (N,), (B, mh, mw, K), (N, K))]
    for k in ORDER:
        setattr(d, k, ins[k].data_ptr())
    d.loss, d.loss_inst, d.d_proto, d.d_coef = [o.data_ptr() for o in outs]
    d.B, d.mh, d.mw, d.K, d.N, d.G, d.crop, d.roi_norm, d.alpha = B, mh, mw, K, N, c['gt'].shape[0], 1, 1, ALPHA
    nbytes = L.lib().ymi_workspace_bytes(L.WS_MASK_LOSS, C.byref(d))
    ws = torch.full((nbytes // 4,), fill, device=DEV)
    d.ws = ws.data_ptr()
    L.check(L.lib().ymi_mask_loss_f32(C.byref(d), L.stream_ptr()), 'ymi_mask_loss_f32')
    torch.cuda.synchronize()
    return [o.cpu() for o in outs]


def test_outputs_are_fully_overwritten_and_bit_reproducible():
    c = case('35x37')
    a = abi_call(c)
    for n, o in zip(NAMES, a):
        assert torch.isfinite(o).all(), n
    assert torch.equal(a[2][1], torch.zeros_like(a[2][1]))              # the image without positives
    b = abi_call(c, fill=float('inf'))
    t = gpu_terms(c)
    for n, x, y, z in zip(NAMES, a, b, t):
        assert torch.equal(x, y) and torch.equal(x, z), n


def test_shipped_geometry_is_bit_reproducible():
    c = case('138x138')
    a, b = gpu_terms(c), gpu_terms(c)
    for n, x, y in zip(NAMES, a, b):
        assert torch.isfinite(x).all(), n
        same_bits(x, y, n)


def test_saturated_logits_stay_finite():
    c = make_case(35, 37, (5, 0, 70), 107, xmax=40.0)
    assert logits(c['proto'], c['coef'], c['img_off']).abs().max().item() > 39
    for crop, roi in ((True, True), (False, False)):
        for n, o in zip(NAMES, gpu_terms(c, crop, roi)):
            assert torch.isfinite(o).all(), (n, crop, roi)
