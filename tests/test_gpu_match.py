"""MultiBoxLoss target assignment and the box loss on the GPU (csrc/match.hip, ymi_match_f32 / ymi_box_loss_f32,
yolact_amd/layers/match.py) against tests/match_ref.py, which tests/test_match_host.py pins to the reference's own results.

Bars.  conf_t, idx_t, pos, num_pos and gt_box_t: bit-equal to match_ref in fp32 on the CPU, for every prior.  loc_t, 'B' and
d_loc: rel_err against match_ref's encode / box loss in fp64 (on the fp32 matching) <= max(4 * rel_err(the same in fp32 on the
CPU, fp64), EXACT_BAR); the factor 4 allows for the device's logf and another summation order, EXACT_BAR = 8e-6 is the project's
exact-fp32 bar (tests/test_gpu_dcn_kat.py).  d_loc is bit-zero off the positives, and two runs give the same bits.

loc_data is CONSTRUCTED from the fp64 targets so that |loc_data - loc_t| stays 1e-3 away from the smooth-L1 kink at 1 (asserted on
the fp64 oracle).  Where loc_t is not finite (log 0 of a zero-area GT) loc_data is 0.  The largest rel_err per case and tensor is
printed at the end of the module (the table of DESIGN.md 5.3).
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_ref as R  # noqa: E402
from helpers import same_bits  # noqa: E402
import yolact_amd  # noqa: E402
import yolact_amd.layers.match as M  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EXACT_BAR = 8e-6
ALPHA = 1.5
META, CASES = R.load_golden()
NAMES = [c['name'] for c in META['cases']]
_MAX = {}
_ORACLES = {}


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    print('\nmatch / box loss: rel_err against the fp64 oracle (bar)')
    for case in _MAX:
        print('  %-14s ' % case + '  '.join('%s %.2e (%.1e)' % (n, e, b) for n, (e, b) in _MAX[case].items()))


@pytest.fixture(autouse=True)
def _cfg(monkeypatch):
    cfg = yolact_amd.CONFIGS['yolact_base_config'].copy()
    monkeypatch.setattr(M, 'active_cfg', lambda: cfg)
    monkeypatch.setattr(yolact_amd.config, 'active_cfg', lambda: cfg)
    return cfg


def build_loc_data(loc_t64, seed):
    """loc_t + a difference of magnitude in [0, 0.998] or [1.002, 2.5] and random sign; 0 where loc_t is not finite."""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(loc_t64.shape, generator=g, dtype=torch.float64)
    mag = torch.where(u < 0.6, u / 0.6 * 0.998, 1.002 + (u - 0.6) / 0.4 * 1.498)
    sign = torch.where(torch.rand(loc_t64.shape, generator=g) < 0.5, -1.0, 1.0).double()
    fin = torch.isfinite(loc_t64)
    return torch.where(fin, loc_t64 + sign * mag, torch.zeros_like(loc_t64)).float()


def oracle(name, priors, targets, num_crowds, seed):
    """Computed once per case: the fp32 CPU matching, the fp64 encode / loss on it, the constructed loc_data and the bars."""
    if name in _ORACLES:
        return _ORACLES[name]
    ref = R.match_batch_ref(priors, targets, num_crowds)
    p64 = priors.double()
    loc_t64 = torch.stack([R.encode_ref(g.double(), p64) for g in ref['gt_box_t']])
    loc_data = build_loc_data(loc_t64, seed)
    pos = ref['pos']
    d = (loc_data.double() - loc_t64)[pos]
    d = d[torch.isfinite(d)]
    assert ((d.abs() - 1).abs() >= 1e-3).all()                          # off the kink, on the fp64 oracle
    loss64, dloc64 = R.box_loss_ref(loc_data.double(), loc_t64, pos, ALPHA)
    loss32, dloc32 = R.box_loss_ref(loc_data, ref['loc_t'], pos, ALPHA)
    want = dict(loc_t=loc_t64, B=loss64.view(1), d_loc=dloc64)
    cpu = dict(loc_t=ref['loc_t'], B=loss32.view(1), d_loc=dloc32)
    bars = {k: max(4 * R.rel_err(cpu[k], want[k]), EXACT_BAR) for k in want}
    _ORACLES[name] = (ref, loc_data, want, bars)
    return _ORACLES[name]


def run_gpu(priors, targets, num_crowds, loc_data):
    out = M.match_targets(priors.to(DEV), [t.to(DEV) for t in targets], num_crowds, loc_data.to(DEV))
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def check(name, out, ref, want, bars):
    assert out['conf_t'].dtype == torch.long and out['idx_t'].dtype == torch.long and out['pos'].dtype == torch.bool
    for k in ('conf_t', 'idx_t', 'pos', 'num_pos'):
        assert torch.equal(out[k], ref[k]), k
    assert torch.equal(out['gt_box_t'].view(torch.int32), ref['gt_box_t'].view(torch.int32))
    errs = {}
    for k in ('loc_t', 'B', 'd_loc'):
        e = R.rel_err(out[k].view(-1), want[k].view(-1))
        errs[k] = (e, bars[k])
        print('%s %s: rel_err %.3e (bar %.3e)' % (name, k, e, bars[k]))
    _MAX[name] = errs
    for k, (e, bar) in errs.items():
        assert e <= bar, (name, k, e, bar)
    off = out['d_loc'][~out['pos']]
    assert off.numel() and (off.view(torch.int32) == 0).all()            # exactly +0.0f off the positives


@pytest.mark.parametrize('name', NAMES)
def test_golden_cases_through_match_targets(name):
    t = CASES[name]
    ref, loc_data, want, bars = oracle(name, t['priors'], t['targets'], t['num_crowds'], 5)
    out = run_gpu(t['priors'], t['targets'], t['num_crowds'], loc_data)
    for k in ('conf_t', 'idx_t', 'gt_box_t'):                            # the reference's own results
        assert torch.equal(out[k], t[k]), k
    assert R.rel_err(out['loc_t'], t['loc_t']) <= bars['loc_t']
    check(name, out, ref, want, bars)


@pytest.mark.parametrize('name', NAMES)
def test_golden_cases_through_the_one_image_match(name):
    from yolact_amd.layers.box_utils import match
    t = CASES[name]
    B, P = len(t['targets']), t['priors'].size(0)
    loc_t = torch.zeros(B, P, 4, device=DEV)
    conf_t = torch.zeros(B, P, dtype=torch.long, device=DEV)
    idx_t = torch.zeros(B, P, dtype=torch.long, device=DEV)
    priors = t['priors'].to(DEV)
    for b, (truths, labels, crowds) in enumerate(R.split_targets(t['targets'], t['num_crowds'])):
        match(0.5, 0.4, truths.to(DEV), priors, labels.to(DEV), None if crowds is None else crowds.to(DEV), loc_t, conf_t, idx_t, b,
              None)
    assert torch.equal(conf_t.cpu(), t['conf_t']) and torch.equal(idx_t.cpu(), t['idx_t'])
    assert R.rel_err(loc_t.cpu(), t['loc_t']) <= EXACT_BAR


def random_targets(g, n, n_crowd):
    """n GT boxes of about the sizes of the 550 prior set's anchors, + n_crowd crowd boxes, bundled as the reference does."""
    size = torch.tensor([24.0, 48.0, 96.0, 192.0, 384.0])[torch.randint(0, 5, (n,), generator=g)] / 550 * (0.7 + 0.7 * torch.rand(n, generator=g))
    ar = 0.6 + 0.9 * torch.rand(n, generator=g)
    w, h = size * ar, size / ar
    c = 0.05 + 0.9 * torch.rand(n, 2, generator=g)
    box = torch.stack([c[:, 0] - w / 2, c[:, 1] - h / 2, c[:, 0] + w / 2, c[:, 1] + h / 2], 1).clamp(0.0, 1.0)
    rows = [torch.cat([box, torch.randint(0, 80, (n, 1), generator=g).float()], 1)]
    for _ in range(n_crowd):
        c = 0.2 + 0.6 * torch.rand(2, generator=g)
        half = 0.05 + 0.25 * torch.rand(2, generator=g)
        rows.append(torch.cat([(c - half).clamp(0, 1), (c + half).clamp(0, 1), torch.tensor([-1.0])]).view(1, 5))
    return torch.cat(rows)


def batch32():
    g = torch.Generator().manual_seed(32)
    priors = R.make_priors((69, 35, 18, 9, 5), 550)
    assert priors.size(0) == 19248
    ns = torch.randint(1, 41, (32,), generator=g).tolist()
    ncs = torch.randint(0, 3, (32,), generator=g).tolist()
    ns[0], ns[1], ncs[0], ncs[1] = 1, 40, 0, 2
    return priors, [random_targets(g, n, c) for n, c in zip(ns, ncs)], ncs


def test_batch_of_32_on_the_550_prior_set_and_reproducibility():
    priors, targets, ncs = batch32()
    ref, loc_data, want, bars = oracle('batch32', priors, targets, ncs, 6)
    assert ref['num_pos'].min() >= 1 and (ref['conf_t'] == -1).any() and (ref['conf_t'] == 0).any()
    out = run_gpu(priors, targets, ncs, loc_data)
    check('batch32', out, ref, want, bars)
    again = run_gpu(priors, targets, ncs, loc_data)
    same_bits(out, again)


def test_more_gts_than_the_force_kernel_keeps_in_lds():
    """300 GTs in one image (the row state of more than 256 lives in the workspace), next to an image with 2."""
    g = torch.Generator().manual_seed(33)
    priors = CASES['many_gt']['priors']
    size = 0.1 + 0.6 * torch.rand(300, generator=g)
    c = 0.1 + 0.8 * torch.rand(300, 2, generator=g)
    box = torch.cat([c - size[:, None] / 2, c + size[:, None] / 2], 1).clamp(0, 1)
    targets = [torch.cat([box, torch.randint(0, 80, (300, 1), generator=g).float()], 1), CASES['plain3']['targets'][0][:2]]
    ref, loc_data, want, bars = oracle('gt300', priors, targets, [0, 0], 7)
    check('gt300', run_gpu(priors, targets, [0, 0], loc_data), ref, want, bars)


def test_thresholds_compare_in_fp32():
    """An overlap of exactly float32(0.4) and its two neighbours (tests/test_match_host.py threshold_case)."""
    priors = torch.tensor([[0.5, 0.5, 1.0, 1.0], [0.25, 0.5, 0.5, 1.0]])
    x = np.float32(0.4)
    ws = [np.nextafter(x, np.float32(0)), x, np.nextafter(x, np.float32(1))]
    targets = [torch.tensor([[0.0, 0.0, float(w), 1.0, 4.0]]) for w in ws]
    ref = R.match_batch_ref(priors, targets, [0, 0, 0])
    assert ref['conf_t'][:, 0].tolist() == [0, -1, -1]
    out = M.match_targets(priors.to(DEV), [t.to(DEV) for t in targets], [0, 0, 0])
    assert 'B' not in out and 'd_loc' not in out
    assert torch.equal(out['conf_t'].cpu(), ref['conf_t']) and torch.equal(out['idx_t'].cpu(), ref['idx_t'])


def test_autograd_through_box_loss_is_d_loc_times_the_upstream_scalar():
    t = CASES['crowds']
    ref, loc_data, want, bars = oracle('crowds', t['priors'], t['targets'], t['num_crowds'], 5)
    out = M.match_targets(t['priors'].to(DEV), [x.to(DEV) for x in t['targets']], t['num_crowds'], loc_data.to(DEV))
    x = loc_data.to(DEV).requires_grad_(True)
    loss = M.box_loss(x, out['loc_t'], out['pos'])['B']
    assert loss.dim() == 0 and torch.equal(loss.detach().view(1).view(torch.int32), out['B'].view(1).view(torch.int32))
    (g,) = torch.autograd.grad(loss * 3.0, [x])
    assert torch.equal(g, out['d_loc'] * 3.0)
    assert R.rel_err(loss.detach().cpu().view(1), want['B']) <= bars['B']


def test_lincomb_mask_loss_takes_the_outputs_unchanged(monkeypatch, _cfg):
    from yolact_amd.layers import mask_loss as ML
    monkeypatch.setattr(ML, 'active_cfg', lambda: _cfg)
    t = CASES['plain3']
    P = t['priors'].size(0)
    g = torch.Generator().manual_seed(9)
    out = M.match_targets(t['priors'].to(DEV), [x.to(DEV) for x in t['targets']], t['num_crowds'])
    assert out['pos'].sum().item() == 7
    mask_data = torch.tanh(torch.randn(1, P, 32, generator=g)).to(DEV)
    proto = (torch.relu(torch.randn(1, 12, 10, 32, generator=g)) * 0.5).to(DEV)
    masks = [(torch.rand(3, 24, 20, generator=g) > 0.5).float().to(DEV)]
    got = ML.lincomb_mask_loss(out['pos'], out['idx_t'], mask_data, proto, masks, out['gt_box_t'])['M']
    ref = R.match_batch_ref(t['priors'], t['targets'], t['num_crowds'])
    want = ML.lincomb_mask_loss(ref['pos'].to(DEV), ref['idx_t'].to(DEV), mask_data, proto, masks, ref['gt_box_t'].to(DEV))['M']
    assert torch.isfinite(got) and got.item() > 0 and torch.equal(got, want)
