"""The train path's deformable convolution on the GPU (csrc/dcn_train.hip: ymi_dcn_cols_fwd_f32, ymi_dcn_cols_entries_f32,
ymi_dcn_cols_bwd_f32; yolact_amd/layers/train_ops.py: deform_conv, dcn_bottleneck; train_net.backbone / forward; Trainer(forward=))
against the fp64 oracle of tests/dcn_train_ref.py, whose cases tests/test_dcn_train_host.py certifies on the CPU.

Bar, per tensor (y and the gradients in x, om, weight, bias): rel_err(gpu, g64) <= max(4 * rel_err(g32, g64), 8e-6), the bar of
tests/test_gpu_dcn_bwd.py; g32 is the CPU fp32 run of the same formulation.  Every gradient is also required to have the SAME BITS
on every run, which is what the op exists for.  The parent's atomic backward (dcn_v2.dcn_v2_conv) is held to the same oracle, so the
two agree within the sum of their bars.
"""
import itertools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dcn_train_ref as D  # noqa: E402
import heads_train_ref as H  # noqa: E402
import train_helpers  # noqa: E402
from gpu_utils import rel_err  # noqa: E402
from helpers import same_bits  # noqa: E402
from test_gpu_dcn_bwd import off_kink_offsets  # noqa: E402,F401  (the cases of dcn_train_ref are built with it)
from train_helpers import DEV, EXACT_BAR, twice  # noqa: E402
import yolact_amd  # noqa: E402
from yolact_amd import modules as M  # noqa: E402
from yolact_amd.layers import train_ops as TO  # noqa: E402

pytestmark = pytest.mark.gpu
_MAX = {}
compare = lambda name, got, w64, w32: train_helpers.compare(_MAX, name, got, w64, w32)
_ORACLES = {}


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    print('\ntrain-mode deformable convolution: rel_err against the fp64 oracle (bar)')
    for case in _MAX:
        print('  %-30s ' % case + '  '.join('%s %.2e (%.1e)' % (k, e, b) for k, (e, b) in _MAX[case].items()))


@pytest.fixture(autouse=True)
def _restore_cfg():
    saved = yolact_amd.config.cfg.copy()
    yield
    yolact_amd.config.cfg.replace(saved)


def oracles(name, case):
    """(g64, g32) of a case, computed once per module and never changed."""
    if name not in _ORACLES:
        _ORACLES[name] = (D.op_grads(case, torch.float64), D.op_grads(case, torch.float32))
    return _ORACLES[name]


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def gpu_op(case, needs=(True, True, True, True), grad=True):
    """deform_conv on the case -> dict of CPU tensors in the oracle's layout (NCHW), None for what `needs` leaves out."""
    x, om, w, b, gy, stride = case
    leaves = [nhwc(x).to(DEV), nhwc(om).to(DEV), w.to(DEV), None if b is None else b.to(DEV)]
    if not grad:
        with torch.no_grad():
            y = TO.deform_conv(*leaves, stride)
        torch.cuda.synchronize()
        return dict(y=y.permute(0, 3, 1, 2).cpu())
    for t, n in zip(leaves, needs):
        if t is not None:
            t.requires_grad_(n)
    y = TO.deform_conv(*leaves, stride)
    y.backward(nhwc(gy).to(DEV))
    torch.cuda.synchronize()
    g = [None if t is None or t.grad is None else t.grad for t in leaves]
    out = dict(y=y.detach().permute(0, 3, 1, 2).cpu(), x=None if g[0] is None else g[0].permute(0, 3, 1, 2).cpu(),
               om=None if g[1] is None else g[1].permute(0, 3, 1, 2).cpu(), weight=None if g[2] is None else g[2].cpu())
    if b is not None:
        out['bias'] = None if g[3] is None else g[3].cpu()
    return out


def parent_op(case):
    """The parent's route on the same data: dcn_v2.dcn_v2_conv (NCHW, the modulation passed in, fp32 atomics), the sigmoid and the
    channel split as torch operations on the om leaf."""
    from yolact_amd import dcn_v2
    x, om, w, b, gy, stride = case
    leaves = [t.to(DEV).requires_grad_(True) for t in (x, om, w)] + ([b.to(DEV).requires_grad_(True)] if b is not None else [])
    bias = leaves[3] if b is not None else torch.zeros(w.shape[0], device=DEV)
    y = dcn_v2.dcn_v2_conv(leaves[0], leaves[1][:, :18], torch.sigmoid(leaves[1][:, 18:]), leaves[2], bias, stride, 1, 1, 1)
    y.backward(gy.to(DEV))
    torch.cuda.synchronize()
    out = dict(y=y.detach().cpu(), x=leaves[0].grad.cpu(), om=leaves[1].grad.cpu(), weight=leaves[2].grad.cpu())
    if b is not None:
        out['bias'] = leaves[3].grad.cpu()
    return out


# ---- 1. against fp64, and the parent's atomic backward --------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(D.OP_CASES))
def test_gradients_against_fp64(name):
    case = D.op_case(name)
    g64, g32 = oracles(name, case)
    got = twice(lambda: gpu_op(case))
    compare(name, got, g64, g32)
    assert all(bool(t.ne(0).any()) for t in got.values())
    # the parent's atomic kernels meet the same oracle under the same bars, so the two agree within their sum
    old, bars = parent_op(case), D.bars(g64, g32)
    for k in g64:
        diff = (got[k].double() - old[k].double()).abs().max().item() / g64[k].abs().max().item()
        print('%s %s: new against the atomic backward %.3e (two bars: %.3e)' % (name, k, diff, 2 * bars[k]))
        assert diff <= 2 * bars[k], (k, diff, bars[k])


# ---- 2. reproducibility ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['adversarial', D.SMALL, 'c128_35_s2'])
def test_three_runs_give_the_same_bits(name):
    """The adversarial case aims every point of a 9 x 9 map at one cell: four pixels of gx hold lists of 729 entries each, which is
    where a sum in arrival order would differ from run to run."""
    case = D.adversarial_case() if name == 'adversarial' else D.op_case(name)
    a, b, c = gpu_op(case), gpu_op(case), gpu_op(case)
    assert sorted(a) == ['bias', 'om', 'weight', 'x', 'y']
    same_bits(a, b)
    same_bits(a, c)
    if name == 'adversarial':
        g64, g32 = oracles(name, case)
        compare(name, a, g64, g32)
        gx = a['x']
        hot = torch.zeros(9, 9, dtype=torch.bool)
        hot[4:6, 4:6] = True
        assert (gx[:, :, ~hot].view(torch.int32) == 0).all() and all(bool(gx[0, :, i, j].ne(0).all()) for i in (4, 5) for j in (4, 5))


# ---- 3. exact zeros ---------------------------------------------------------------------------------------------------------------------------
def test_every_point_outside_the_image():
    case = D.outside_case()
    got = gpu_op(case)
    b = case[3]
    assert (got['x'].view(torch.int32) == 0).all()                                  # +0.0, every bit
    assert bool((got['om'] == 0).all())
    same_bits(got['y'], b.view(1, -1, 1, 1).expand_as(got['y']).contiguous(), 'y is the bias')
    assert bool((got['weight'] == 0).all()) and bool(got['bias'].ne(0).any())


def test_unsampled_rows_get_exact_zeros():
    case = D.band_case()
    got = gpu_op(case)
    lo, hi = D.BAND
    gx = got['x']
    rows = torch.zeros(gx.shape[2], dtype=torch.bool)
    rows[lo:hi + 1] = True
    assert (gx[:, :, ~rows].view(torch.int32) == 0).all()
    assert all(bool(gx[:, :, r].ne(0).any()) for r in range(lo, hi + 1))
    g64, g32 = oracles('band', case)
    compare('band', got, g64, g32)


# ---- 4. the initial state of a DCN ----------------------------------------------------------------------------------------------------------
def test_zero_offsets_and_logits():
    """om = 0: every point on a pixel, every modulation 1/2.  y = conv2d_plain(x, w) / 2 + b, gx and gw half the plain convolution's,
    within 8e-6; d/d dh and d/d dw are the one-sided derivatives of the cells [h, h + 1], [w, w + 1], as the parent's kernel has them."""
    case = D.zero_om_case()
    x, om, w, b, gy, stride = case
    got = twice(lambda: gpu_op(case))
    leaves = [nhwc(x).to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)]
    yp = TO.conv2d_plain(leaves[0], leaves[1], stride)
    yp.backward(nhwc(gy).to(DEV))
    torch.cuda.synchronize()
    want_y = (0.5 * yp.detach() + b.to(DEV)).permute(0, 3, 1, 2).cpu()
    for k, a, r in (('y', got['y'], want_y), ('x', got['x'], 0.5 * leaves[0].grad.permute(0, 3, 1, 2).cpu()),
                    ('weight', got['weight'], 0.5 * leaves[1].grad.cpu())):
        e = rel_err(a.double(), r.double())
        print('zero om %s: rel_err %.3e against half the plain convolution' % (k, e))
        assert e <= EXACT_BAR, (k, e)
    g64, g32 = oracles('zero_om', case)
    # on a kink the CPU's grid_sample picks its cell by the rounding of its own coordinate arithmetic, so no CPU run is a yardstick for
    # the offset channels here: the bar is the one the parent's kernel is held to on the off-kink case of the same shape class
    small = oracles(D.SMALL, D.op_case(D.SMALL))
    bar = max(4 * rel_err(small[1]['om'][:, :18].double(), small[0]['om'][:, :18]), EXACT_BAR)
    old = parent_op(case)
    e = rel_err(got['om'][:, :18].double(), old['om'][:, :18].double())
    print('zero om offsets: rel_err %.3e against the atomic backward (bar %.3e)' % (e, bar))
    assert e <= bar and bool(got['om'][:, :18].ne(0).any())
    # the logits: mu (1 - mu) = 1/4 of d/d mu
    assert rel_err(got['om'][:, 18:].double(), g64['om'][:, 18:]) <= max(4 * rel_err(g32['om'][:, 18:].double(), g64['om'][:, 18:]), EXACT_BAR)


# ---- 5. needs_input_grad ------------------------------------------------------------------------------------------------------------------------
def test_every_requires_grad_subset():
    case = D.op_case(D.SMALL)
    full = gpu_op(case)
    same_bits(gpu_op(case, grad=False)['y'], full['y'], 'the no-grad forward')
    for needs in itertools.product((False, True), repeat=4):
        if not any(needs):
            continue
        got = gpu_op(case, needs)
        same_bits(got['y'], full['y'], 'y')
        for k, want in zip(('x', 'om', 'weight', 'bias'), needs):
            assert (got[k] is not None) == want, (needs, k)
            if want:
                same_bits(got[k], full[k], '%s of %s' % (k, needs))


# ---- 6. the DCN bottleneck ----------------------------------------------------------------------------------------------------------------------
def make_block(spec, params):
    inplanes, planes, stride, projection = spec
    import torch.nn as nn
    ds = nn.Sequential(nn.Conv2d(inplanes, 4 * planes, 1, stride=stride, bias=False), nn.BatchNorm2d(4 * planes)) if projection else None
    blk = M.Bottleneck(inplanes, planes, stride, ds, use_dcn=True)
    sd = blk.state_dict()
    assert sorted(n for n in sd if 'num_batches' not in n) == sorted(params)
    with torch.no_grad():
        for n in params:
            assert sd[n].shape == params[n].shape, n
            sd[n].copy_(params[n])
    return blk.to(DEV).eval()


def run_block(blk, params, x, up, batch_stats):
    with torch.no_grad():
        for n, t in blk.state_dict().items():
            if 'running' in n:
                t.copy_(params[n])
    leaf = nhwc(x).to(DEV).requires_grad_(True)
    out = TO.dcn_bottleneck(leaf, blk, batch_stats)
    named = list(blk.named_parameters())
    gr = torch.autograd.grad((out * nhwc(up).to(DEV)).sum(), [leaf] + [p for _, p in named])
    torch.cuda.synchronize()
    got = {'y': out.detach().permute(0, 3, 1, 2).cpu(), 'd_x': gr[0].permute(0, 3, 1, 2).cpu()}
    got.update({'d_' + n: t.cpu() for (n, _), t in zip(named, gr[1:])})
    got.update({'new_' + n: t.detach().cpu().clone() for n, t in blk.state_dict().items() if 'running' in n})
    return got


@pytest.mark.parametrize('batch_stats', [False, True], ids=['frozen', 'batch_stats'])
@pytest.mark.parametrize('variant', list(D.BLOCK_SPECS))
def test_dcn_bottleneck_through_autograd(variant, batch_stats):
    spec, x, params, up = D.block_case(variant, batch_stats)
    r64, r32 = (D.run_block_ref(x, params, spec[2], up, batch_stats, dt) for dt in (torch.float64, torch.float32))
    keys = [k for k in r64 if not k.startswith('_')]
    blk = make_block(spec, params)
    got = twice(lambda: run_block(blk, params, x, up, batch_stats))
    compare('%s_%s' % (variant, 'stats' if batch_stats else 'frozen'), got, {k: r64[k] for k in keys}, {k: r32[k] for k in keys})
    for n in D.DCN_NAMES + ('conv2.weight',):
        assert bool(got['d_' + n].ne(0).any()), n
    if not batch_stats:
        for n in params:
            if 'running' in n:
                same_bits(got['new_' + n], params[n], n)
    with pytest.raises(NotImplementedError, match='DCN block'):
        TO.bottleneck(nhwc(x).to(DEV), blk)


# ---- 7. end to end ------------------------------------------------------------------------------------------------------------------------------
def test_a_plus_config_trains_end_to_end():
    """yolact_plus_resnet50_config shrunk to 96 x 96 images and 32 features: train_net.forward -> MultiBoxLossPlus -> backward reaches
    every DCN parameter with the same bits twice; Trainer(net, forward=..) takes two steps; the Yolact methods keep refusing."""
    from yolact_amd import train_net as TN
    from yolact_amd.layers.modules.multibox_loss_plus import MultiBoxLossPlus
    from yolact_amd.training import Trainer
    from yolact_amd.yolact import Yolact
    yolact_amd.set_cfg('yolact_plus_resnet50_config')
    cfg = yolact_amd.config.cfg
    o = H.golden_cfg_overrides()
    cfg.fpn = cfg.fpn.copy({'num_features': o.pop('num_features')})
    cfg.update(o)
    # 96 x 96 images give 24 x 24 prototypes: the mask-IoU net keeps its first three stride-2 layers (24 -> 11 -> 5 -> 2; all five need 63)
    cfg.update(dict(lr=1e-3, lr_warmup_until=0, lr_steps=(), freeze_bn=False, maskiou_net=list(cfg.maskiou_net)[:3]))
    torch.manual_seed(5)
    net = Yolact()
    gen = torch.Generator().manual_seed(5)
    with torch.no_grad():      # a DCN away from its all-zero initial offsets, so that the offsets matter
        for n, p in net.backbone.named_parameters():
            if 'conv_offset_mask.weight' in n:
                p.copy_(torch.randn(p.shape, generator=gen) * 0.01)
            elif 'conv_offset_mask.bias' in n:
                p.copy_(torch.randn(p.shape, generator=gen) * 0.5)
    net.to(DEV)
    assert cfg.use_maskiou and net.maskiou_net is not None
    dcn = [('layers.%d.%d.conv2.%s' % (si, bi, n), p) for si, layer in enumerate(net.backbone.layers) for bi, blk in enumerate(layer)
           if blk.use_dcn for n, p in blk.conv2.named_parameters()]
    n_blocks = sum(blk.use_dcn for layer in net.backbone.layers for blk in layer)
    assert n_blocks == 13 and len(dcn) == 4 * n_blocks
    gen = torch.Generator().manual_seed(4)
    images = torch.randn(2, 3, 96, 96, generator=gen).to(DEV)
    targets = [torch.tensor([[0.11, 0.13, 0.42, 0.41, 2.0], [0.52, 0.31, 0.93, 0.79, 0.0], [0.21, 0.56, 0.44, 0.81, 4.0],
                             [0.03, 0.03, 0.97, 0.96, 1.0]]),
               torch.tensor([[0.31, 0.22, 0.79, 0.71, 1.0], [0.06, 0.61, 0.29, 0.84, 3.0]])]
    masks = []
    for t in targets:
        m = torch.zeros(t.size(0), 48, 48)
        for j, (x1, y1, x2, y2) in enumerate((t[:, :4] * 48).round().long().tolist()):
            m[j, y1:y2, x1:x2] = 1
        masks.append(m.to(DEV))
    targets = [t.to(DEV) for t in targets]
    state = {k: v.detach().clone() for k, v in net.state_dict().items()}
    crit = MultiBoxLossPlus(cfg.num_classes, cfg.positive_iou_threshold, cfg.negative_iou_threshold, cfg.ohem_negpos_ratio)

    def run():
        net.load_state_dict(state)
        net.zero_grad()
        cfg._tmp_img_h = cfg._tmp_img_w = None
        torch.manual_seed(3)
        losses = crit(net, TN.forward(net, images, True), targets, masks, [0, 0])
        assert (cfg._tmp_img_h, cfg._tmp_img_w) == (96, 96)
        sum(losses.values()).backward()
        torch.cuda.synchronize()
        got = {k: v.detach().cpu().view(1) for k, v in losses.items()}
        got.update({'d_' + n: p.grad.cpu() for n, p in net.named_parameters() if p.grad is not None})
        return got
    got = twice(run)
    print('losses:', {k: round(float(v), 4) for k, v in got.items() if len(k) == 1})
    assert set('BCMS') <= set(got) and all(bool(torch.isfinite(v).all()) for v in got.values())
    for n, _ in dcn:
        g = got['d_backbone.' + n]
        assert bool(torch.isfinite(g).all()) and bool(g.ne(0).any()), n

    net.load_state_dict(state)
    net.zero_grad()
    tr = Trainer(net, forward=lambda x, bs: TN.forward(net, x, bs))
    assert type(tr.criterion) is MultiBoxLossPlus and tr.batch_stats is True
    for it in range(2):
        torch.manual_seed(100 + it)
        losses = tr.step(images, targets, masks, [0, 0])
    torch.cuda.synchronize()
    assert tr.iteration == 2 and int(tr.optimizer.skipped.item()) == 0 and all(bool(torch.isfinite(v).all()) for v in losses.values())
    for n, p in dcn:
        assert not torch.equal(p.detach(), state['backbone.' + n]), n
    # what stays refused, on the same net
    with pytest.raises(NotImplementedError, match='is a DCN block'):
        net.forward_train(images)
    with pytest.raises(NotImplementedError, match='is a DCN block'):
        net.forward_backbone(torch.zeros(2, 64, 24, 24, device=DEV))
    with pytest.raises(NotImplementedError, match='is a DCN block'):
        Trainer(net).step(images, targets, masks, [0, 0])
