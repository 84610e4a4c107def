"""images -> forward_train -> MultiBoxLoss -> backward() on the GPU against the composed fp64 oracle (tests/train_net_ref.py, pinned to
the reference by tests/test_train_net_host.py), on the two cases of tests/train_step_ref.build_grads_case: 'stats' (batch statistics,
every parameter trains) and 'frozen' (the running statistics, BatchNorm affine parameters frozen).  Every pyramid level holds a
positive prior and every trained parameter has a non-zero gradient, so each wiring between the pieces carries signal.

The bars come from the two oracles alone (fp32 and fp64), never from the GPU's result:
  * the four losses, every running statistic after the step, and the gradients of the FPN, the protonet, the prediction head and
    semantic_seg_conv (whose ReLUs keep 16 times the fp32 deviation as margin in these cases): train_helpers.compare, max-norm,
    bar = max(4 * rel_err(fp32 oracle, fp64 oracle), EXACT_BAR) per tensor;
  * the gradients of the stem and of each stage: rel. L2 per tensor against the fp64 oracle,
    bar = max(4 * the largest rel. L2 between the two oracles over the section's tensors, EXACT_BAR).  About two million ReLU and
    max-pool decisions sit below the FPN and some differ between any two fp32 evaluations; a single flip lands on different tensors in
    different evaluations, hence the section's maximum.

Measured on the MI355X (largest error / its bar):
                          stats                    frozen
    losses                9.9e-07 / 8.0e-06 (S)    2.8e-07 / 8.0e-06 (B)
    running statistics    5.5e-06 / 8.0e-06        0 / 8.0e-06 (untouched)
    above the backbone    3.1e-06 / 8.3e-06        2.3e-05 / 6.0e-05 (fpn.downsample_layers.1.weight)
    stem                  1.3e-02 / 5.0e-02        8.6e-03 / 4.4e-02
    layers.0              1.5e-02 / 5.4e-02        9.0e-03 / 4.7e-02
    layers.1              1.4e-02 / 5.3e-02        8.5e-03 / 4.6e-02
    layers.2              1.7e-02 / 6.5e-02        1.1e-02 / 4.4e-02
    layers.3              1.6e-02 / 6.4e-02        5.9e-03 / 4.0e-02
The comparison found no disagreement: every term, factor and level of train_net.py is the oracle's.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_net_ref as N  # noqa: E402
import train_step_ref as T  # noqa: E402
import yolact_amd  # noqa: E402
from train_helpers import DEV, EXACT_BAR, compare, twice  # noqa: E402
from yolact_amd.layers.modules import MultiBoxLoss  # noqa: E402

pytestmark = pytest.mark.gpu
LOSS_SEED = 100                  # as tests/test_gpu_train_step.py seeds MultiBoxLoss
F64, F32 = torch.float64, torch.float32
RECORD = {}


@pytest.fixture(scope='module', autouse=True)
def _summary():
    saved = yolact_amd.config.cfg.copy()
    yield
    yolact_amd.config.cfg.replace(saved)
    for name, errs in RECORD.items():
        worst = max(errs.items(), key=lambda kv: kv[1][0] / kv[1][1])
        print('%-24s largest error / bar: %.3e / %.3e (%s)' % (name, worst[1][0], worst[1][1], worst[0]))


def run_gpu(net, state, inputs, batch_stats):
    images, targets, masks, num_crowds = inputs
    cfg = yolact_amd.config.cfg
    net.load_state_dict(state)
    for p in net.parameters():
        p.grad = None
    torch.manual_seed(LOSS_SEED)
    crit = MultiBoxLoss(cfg.num_classes, cfg.positive_iou_threshold, cfg.negative_iou_threshold, cfg.ohem_negpos_ratio)
    losses = crit(net, net.forward_train(images, batch_stats), targets, masks, num_crowds)
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    out = {'loss ' + k: v.detach().cpu().view(1) for k, v in losses.items()}
    out.update({'grad ' + n: p.grad.cpu() for n, p in net.named_parameters() if p.grad is not None})
    out.update({'stat ' + n: b.detach().cpu() for n, b in net.named_buffers() if N.is_stat(n)})
    return out


@pytest.mark.parametrize('name', T.GRADS_CASES)
def test_losses_statistics_and_gradients(name):
    res, _, inputs = T.grads_oracles(name)                           # the host's part: seconds
    o64, o32 = res[F64], res[F32]
    net, images, targets, masks, num_crowds, batch_stats = T.build_grads_case(DEV, name)
    assert batch_stats == inputs['batch_stats']
    state = {k: v.detach().clone() for k, v in net.state_dict().items()}
    for k, v in inputs['state'].items():
        assert torch.equal(v, state[k].cpu()), k
    got = twice(lambda: run_gpu(net, state, (images, targets, masks, num_crowds), batch_stats))
    pick = lambda prefix: {k[len(prefix):]: v for k, v in got.items() if k.startswith(prefix)}
    losses, grads, stats = pick('loss '), pick('grad '), pick('stat ')

    # structure: a gradient exactly where the oracle has one, of its shape, and not all zero
    no_grad = sorted(n for n, p in net.named_parameters() if p.grad is None)
    assert no_grad == sorted(n for n, _ in net.named_parameters() if n not in o64['grads'])
    assert len(no_grad) == (0 if name == 'stats' else 2 * 53) and all(N.is_bn_affine(n) for n in no_grad)
    assert sorted(grads) == sorted(o64['grads'])
    for n, g in grads.items():
        assert g.shape == o64['grads'][n].shape, n
        assert bool(o64['grads'][n].ne(0).any()) and bool(g.ne(0).any()), n
        assert bool(torch.isfinite(g).all()), n

    compare(RECORD, name + ' losses', losses, {k: v.view(1) for k, v in o64['losses'].items()},
            {k: v.view(1) for k, v in o32['losses'].items()})
    compare(RECORD, name + ' statistics', stats, o64['new_stats'], o32['new_stats'])
    above = lambda d: {n: g for n, g in d.items() if N.section_of(n) is None}
    compare(RECORD, name + ' above the backbone', above(grads), above(o64['grads']), above(o32['grads']))

    noise = N.section_noise(o32['grads'], o64['grads'])
    failed = []
    for s in N.SECTIONS:
        bar = max(4 * noise[s], EXACT_BAR)
        errs = {n: (N.rel_l2(g, o64['grads'][n]), bar) for n, g in grads.items() if N.section_of(n) == s}
        assert errs, s
        RECORD['%s %s' % (name, s)] = errs
        worst = max(errs, key=lambda n: errs[n][0])
        print('%s %s: %d tensors, largest rel. L2 %.3e (%s), bar %.3e' % (name, s, len(errs), errs[worst][0], worst, bar))
        failed += [(n, e, bar) for n, (e, bar) in errs.items() if not e <= bar]
    assert not failed, failed
