"""The OHEM class loss 'C' on the GPU (csrc/class_loss.hip, ymi_class_loss_f32, yolact_amd/layers/class_loss.py) against
tests/class_loss_ref.py, which tests/test_class_loss_host.py pins to the reference's own results.

Bars.  neg and num_neg: equal to the fp64 oracle for every prior.  Inputs are BUILT with a gap of 1e-3 between the last selected
and the first unselected key of every image (class_loss_ref.open_the_cuts), asserted on the fp64 oracle: 1e-3 is ~500 ulp of a key,
the fp32 key is within 1e-6 of fp64.  'C' and d_conf: rel_err against the fp64 oracle <= max(4 * rel_err(the same in fp32 on the
CPU, fp64), EXACT_BAR); the factor 4 allows for the device's expf / logf and another summation order, EXACT_BAR = 8e-6 is the
project's exact-fp32 bar (tests/test_gpu_match.py).  d_conf is bit-zero off pos | neg, and two runs give the same bits.  The
largest rel_err per case is printed at the end of the module (the table of DESIGN.md 5.4).
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import class_loss_ref as R  # noqa: E402
import match_ref  # noqa: E402
from helpers import same_bits  # noqa: E402
import yolact_amd  # noqa: E402
import yolact_amd.layers.class_loss as CL  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EXACT_BAR = 8e-6
GAP = 1e-3
_MAX = {}


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    print('\nclass loss: rel_err against the fp64 oracle (bar)')
    for case in _MAX:
        print('  %-14s ' % case + '  '.join('%s %.2e (%.1e)' % (n, e, b) for n, (e, b) in _MAX[case].items()))


@pytest.fixture(autouse=True)
def _cfg(monkeypatch):
    cfg = yolact_amd.CONFIGS['yolact_base_config'].copy()
    monkeypatch.setattr(CL, 'active_cfg', lambda: cfg)
    return cfg


def logits(g, B, P, C):
    return (torch.randn(B, P, C, generator=g) * 2.0).clamp(-8, 8)


def labels(g, B, P, C, npos, nneutral=0):
    """npos[b] positives and nneutral neutrals per image at random priors."""
    ct = torch.zeros(B, P, dtype=torch.long)
    for b in range(B):
        perm = torch.randperm(P, generator=g)
        ct[b, perm[:npos[b]]] = torch.randint(1, C, (npos[b],), generator=g)
        ct[b, perm[npos[b]:npos[b] + nneutral]] = -1
    return ct


def run_gpu(conf, ct, ratio=3):
    out = CL.ohem_terms(conf.to(DEV), ct.to(DEV), ratio)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def check(name, conf, ct, ratio=3, gap=GAP):
    """One GPU call against the fp64 oracle; -> (out, oracle64)."""
    o64 = R.ohem_ref(conf.double(), ct, ratio)
    o32 = R.ohem_ref(conf, ct, ratio)
    if gap is not None:
        assert min(R.cut_gaps(o64['key'], o64['n'])) >= gap               # the cut of every image is open, on the fp64 oracle
    out = run_gpu(conf, ct, ratio)
    assert out['neg'].dtype == torch.bool and out['num_neg'].dtype == torch.long
    assert torch.equal(out['neg'], o64['neg']) and torch.equal(out['num_neg'], o64['num_neg'])
    errs = {}
    for k, got, want, cpu in (('C', out['C'], o64['loss'].view(1), o32['loss'].view(1)), ('d_conf', out['d_conf'], o64['d_conf'], o32['d_conf'])):
        bar = max(4 * R.rel_err(cpu, want), EXACT_BAR)
        errs[k] = (R.rel_err(got, want), bar)
        print('%s %s: rel_err %.3e (bar %.3e)' % (name, k, errs[k][0], bar))
    _MAX[name] = errs
    for k, (e, bar) in errs.items():
        assert e <= bar, (name, k, e, bar)
    off = out['d_conf'][~(out['neg'] | (ct > 0))]
    assert (off.view(torch.int32) == 0).all()                            # exactly +0.0f off pos | neg (no such row: the clamp case)
    return out, o64


def test_labels_of_the_match_golden_with_positives_neutrals_and_three_images():
    meta, cases = match_ref.load_golden()
    ct = cases['crowds']['conf_t']
    assert tuple(ct.shape) == (3, 345) and (ct > 0).any() and (ct < 0).any()
    g = torch.Generator().manual_seed(50)
    conf = R.open_the_cuts(logits(g, 3, 345, 81), ct, 3, 2 * GAP)
    out, o64 = check('crowds', conf, ct)
    assert out['num_neg'].sum() > 0
    same_bits(out, run_gpu(conf, ct))


def test_an_image_without_positives_selects_nothing_on_1290_priors():
    g = torch.Generator().manual_seed(51)
    ct = labels(g, 2, 1290, 81, [23, 0], 40)
    conf = R.open_the_cuts(logits(g, 2, 1290, 81), ct, 3, 2 * GAP)
    out, o64 = check('no_pos', conf, ct)
    assert out['num_neg'].tolist() == [69, 0] and not out['neg'][1].any()
    assert (out['d_conf'][1].view(torch.int32) == 0).all()


def test_the_clamp_to_p_minus_1_mines_every_negative():
    g = torch.Generator().manual_seed(52)
    ct = labels(g, 1, 345, 81, [200])
    out, o64 = check('clamp', logits(g, 1, 345, 81), ct)
    assert o64['n'].tolist() == [344] and out['num_neg'].tolist() == [145]


def test_exact_ties_at_the_cut_go_to_the_lowest_prior():
    """One row's logits copied to 16 other rows on both sides of the select kernel's 1024-prior chunk; the cut falls inside the group.
    Against the oracle only: the reference leaves ties to an unstable sort."""
    g = torch.Generator().manual_seed(53)
    P = 1290
    conf = logits(g, 1, P, 81)
    group = torch.sort(torch.randperm(P, generator=g)[:17])[0]
    assert group[0] < 1024 < group[-1]
    row = conf[0, group[3]].clone()
    row[0], row[5] = -20.0, 12.0                                        # a key of ~32: above every other row's
    conf[0, group] = row
    ct = torch.zeros(1, P, dtype=torch.long)
    free = torch.tensor([i for i in range(P) if i not in set(group.tolist())])
    ct[0, free[torch.randperm(free.numel(), generator=g)[:5]]] = 7      # 5 positives: 15 of the 17 equal keys are taken
    out, o64 = check('ties', conf, ct, gap=None)
    s = torch.sort(o64['key'], 1, descending=True)[0]
    assert s[0, 14] == s[0, 15] == s[0, 16] and s[0, 16] > s[0, 17]      # the cut is inside the tie group
    assert out['neg'][0].nonzero().view(-1).tolist() == group[:15].tolist()


def test_rows_far_from_the_batch_maximum_stay_finite():
    """A row of +-80 and a row 100 below the batch maximum: the reference's global-maximum log_sum_exp gives log 0 for the second."""
    g = torch.Generator().manual_seed(54)
    ct = labels(g, 2, 345, 81, [10, 12], 5)
    conf = logits(g, 2, 345, 81)
    negs = (ct[0] == 0).nonzero().view(-1)
    conf[0, negs[0]] = torch.tensor([80.0, -80.0]).repeat(41)[:81]
    conf[0, negs[1]] = conf[0, negs[1]] - 100.0
    pos = (ct[1] > 0).nonzero().view(-1)
    conf[1, pos[0]] = conf[1, pos[0]] - 100.0
    conf = R.open_the_cuts(conf, ct, 3, 2 * GAP)
    out, o64 = check('extremes', conf, ct)
    assert torch.isfinite(out['C']).all() and torch.isfinite(out['d_conf']).all()


def test_four_classes_take_the_even_stride_path():
    g = torch.Generator().manual_seed(55)
    ct = labels(g, 2, 345, 4, [30, 9], 11)
    conf = R.open_the_cuts(logits(g, 2, 345, 4), ct, 3, 2 * GAP)
    check('C4', conf, ct)


def test_a_label_out_of_range_gives_nan_and_reads_nothing():
    g = torch.Generator().manual_seed(56)
    ct = labels(g, 1, 345, 81, [10])
    ct[0, (ct[0] == 0).nonzero()[0]] = 200                              # compared with C before it indexes
    out = run_gpu(logits(g, 1, 345, 81), ct)
    assert torch.isnan(out['C']).all() and out['num_neg'].item() > 0


def test_backward_is_d_conf_times_the_upstream_scalar():
    g = torch.Generator().manual_seed(57)
    ct = labels(g, 2, 345, 81, [14, 3], 6)
    conf = R.open_the_cuts(logits(g, 2, 345, 81), ct, 3, 2 * GAP)
    terms = CL.ohem_terms(conf.to(DEV), ct.to(DEV))
    x = conf.to(DEV).requires_grad_(True)
    loss = CL.ohem_conf_loss(x, ct.to(DEV))
    assert loss.dim() == 0 and torch.equal(loss.detach().view(1).view(torch.int32), terms['C'].view(torch.int32))
    (gx,) = torch.autograd.grad(loss * 0.37, [x])
    assert torch.equal(gx, terms['d_conf'] * 0.37)
    assert CL.ohem_conf_loss(conf.to(DEV), ct.to(DEV)).requires_grad is False


def test_full_size_batch_of_8_and_reproducibility():
    g = torch.Generator().manual_seed(58)
    B, P = 8, 19248
    ct = labels(g, B, P, 81, torch.randint(80, 121, (B,), generator=g).tolist(), 300)
    conf = R.open_the_cuts(logits(g, B, P, 81), ct, 3, 2 * GAP)
    out, o64 = check('b8_19248', conf, ct)
    assert out['num_neg'].tolist() == [3 * int(n) for n in (ct > 0).sum(1)]
    same_bits(out, run_gpu(conf, ct))
