"""MultiBoxLoss on the GPU (yolact_amd/layers/modules/multibox_loss.py: B + M + C + S on the HIP kernels) against the composed
oracles of tests/multibox_ref.py, which tests/test_multibox_host.py pins to the reference's own forward().

Bars: every loss and the gradient of the losses' sum in loc, conf, mask, proto and segm: rel_err against the fp64 oracle <=
max(4 * rel_err(the same in fp32 on the CPU, fp64), EXACT_BAR = 8e-6), the project's bar (tests/test_gpu_match.py).  The rows of
d_conf that are non-zero - pos | neg - equal the oracle's exactly (the cut of every image is open by 1e-3, asserted on the fp64 oracle).
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import class_loss_ref as CR  # noqa: E402
import match_ref  # noqa: E402
import multibox_ref as R  # noqa: E402
import yolact_amd  # noqa: E402
from yolact_amd.layers import class_loss, mask_loss, match, segm_loss  # noqa: E402
from yolact_amd.layers.modules import MultiBoxLoss  # noqa: E402
import yolact_amd.layers.modules.multibox_loss as MB  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EXACT_BAR = 8e-6
META, G = CR.load_golden()
_MAX = {}


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    print('\nMultiBoxLoss: rel_err against the fp64 oracle (bar)')
    for case in _MAX:
        print('  %-10s ' % case + '  '.join('%s %.2e (%.1e)' % (n, e, b) for n, (e, b) in _MAX[case].items()))


@pytest.fixture(autouse=True)
def _cfg(monkeypatch):
    cfg = yolact_amd.CONFIGS['yolact_base_config'].copy()
    for mod in (MB, class_loss, mask_loss, match, segm_loss):
        monkeypatch.setattr(mod, 'active_cfg', lambda: cfg)
    return cfg


def run_gpu(preds, targets, masks, num_crowds, seed):
    leaves = {k: preds[k].to(DEV).requires_grad_(True) for k in R.NAMES}
    p = dict(leaves, priors=preds['priors'].to(DEV))
    tg, mk, nc = [t.to(DEV) for t in targets], [m.to(DEV) for m in masks], list(num_crowds)
    shapes = [tuple(t.shape) for t in tg], [tuple(m.shape) for m in mk]
    torch.manual_seed(seed)
    losses = MultiBoxLoss(81, 0.5, 0.4, 3)(None, p, tg, mk, nc)
    assert sorted(losses) == ['B', 'C', 'M', 'S'] and all(v.dim() == 0 for v in losses.values())
    assert ([tuple(t.shape) for t in tg], [tuple(m.shape) for m in mk]) == shapes and nc == list(num_crowds)   # the caller's lists
    grads = torch.autograd.grad(sum(losses.values()), [leaves[k] for k in R.NAMES])
    torch.cuda.synchronize()
    return {k: v.detach().cpu() for k, v in losses.items()}, {k: g.cpu() for k, g in zip(R.NAMES, grads)}


def check(name, preds, targets, masks, num_crowds, seed=11):
    torch.manual_seed(seed)
    l64, g64, ex = R.multibox_ref(preds, targets, masks, num_crowds, torch.float64)
    torch.manual_seed(seed)
    l32, g32, _ = R.multibox_ref(preds, targets, masks, num_crowds, torch.float32)
    assert min(CR.cut_gaps(ex['key'], ex['n'])) >= 1e-3
    losses, grads = run_gpu(preds, targets, masks, num_crowds, seed)
    errs = {}
    for k in 'BMCS':
        errs[k] = (CR.rel_err(losses[k].view(1), l64[k].view(1)), max(4 * CR.rel_err(l32[k].view(1), l64[k].view(1)), EXACT_BAR))
    for k in R.NAMES:
        errs['d_' + k] = (CR.rel_err(grads[k], g64[k]), max(4 * CR.rel_err(g32[k], g64[k]), EXACT_BAR))
    _MAX[name] = errs
    for k, (e, bar) in errs.items():
        print('%s %s: rel_err %.3e (bar %.3e)' % (name, k, e, bar))
    for k, (e, bar) in errs.items():
        assert e <= bar, (name, k, e, bar)
    sel = ex['neg'] | (ex['conf_t'] > 0)
    assert torch.equal(grads['conf'].ne(0).any(2), sel)
    assert (grads['conf'][~sel].view(torch.int32) == 0).all()
    return losses, grads


def test_the_golden_forward_case():
    preds, targets, masks, ncs = R.golden_forward(G, META)
    losses, grads = check('golden', preds, targets, masks, ncs)
    # the reference's own selection: the rows its gradient touches
    assert torch.equal(grads['conf'].ne(0).any(2), G['fwd_d_conf'].ne(0).any(2))


def test_a_seeded_batch_of_4_on_the_550_prior_set():
    from test_gpu_match import random_targets
    g = torch.Generator().manual_seed(70)
    priors = match_ref.make_priors((69, 35, 18, 9, 5), 550)
    P = priors.size(0)
    assert P == 19248
    ns, ncs = [3, 1, 6, 2], [0, 1, 2, 0]
    targets = [random_targets(g, n, c) for n, c in zip(ns, ncs)]
    masks = []
    for t in targets:
        m = torch.zeros(t.size(0), 64, 64)
        for j, (x1, y1, x2, y2) in enumerate((t[:, :4] * 64).round().long().tolist()):
            m[j, y1:max(y2, y1 + 2), x1:max(x2, x1 + 2)] = 1
        masks.append(m)
    conf_t = match_ref.match_batch_ref(priors, targets, ncs)['conf_t']
    conf = CR.open_the_cuts((torch.randn(4, P, 81, generator=g) * 2).clamp(-8, 8), conf_t, 3, 2e-3)
    preds = dict(priors=priors, loc=torch.randn(4, P, 4, generator=g) * 0.7, conf=conf,
                 mask=torch.tanh(torch.randn(4, P, 32, generator=g)), proto=torch.relu(torch.randn(4, 34, 34, 32, generator=g)) * 0.5,
                 segm=torch.randn(4, 80, 18, 18, generator=g) * 2)
    check('b4_19248', preds, targets, masks, ncs)
