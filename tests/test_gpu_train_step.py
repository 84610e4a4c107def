"""Trainer on the GPU, on the model and inputs of tests/test_gpu_stem_train.py test_multibox_loss_from_the_images (seeded ResNet-50 stages,
32 features, two 96 x 96 images; tests/train_step_ref.build_case): a step is exactly forward_train, MultiBoxLoss, backward and the
once-rounded update; the schedule reaches the optimiser; the loss falls as the reference's does; the parameter stamp moves."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_step_ref as T  # noqa: E402
import yolact_amd  # noqa: E402
from helpers import same_bits  # noqa: E402
from yolact_amd.layers.modules import MultiBoxLoss  # noqa: E402
from yolact_amd.training import Trainer, lr_at  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSS_SEED = 100                  # tools/make_golden_train_step.py seeds every iteration with LOSS_SEED + iteration


@pytest.fixture(scope='module')
def case():
    """The net (built once), its initial state dict (never changed) and the inputs."""
    net, images, targets, masks, num_crowds = T.build_case(DEV)
    state = {k: v.detach().clone() for k, v in net.state_dict().items()}
    saved = yolact_amd.config.cfg.copy()
    yield net, state, (images, targets, masks, num_crowds)
    yolact_amd.config.cfg.replace(saved)


def reset(net, state, **cfg_fields):
    """The initial weights and statistics, no gradients, the case's config with `cfg_fields` replaced."""
    net.load_state_dict(state)
    for p in net.parameters():
        p.grad = None
    yolact_amd.config.cfg.update(dict(lr=1e-3, lr_warmup_init=1e-4, lr_warmup_until=500, lr_steps=(280000, 600000, 700000, 750000),
                                      gamma=0.1, momentum=0.9, decay=5e-4, freeze_bn=False))
    yolact_amd.config.cfg.update(cfg_fields)


def snapshot(net, momentum_of, losses):
    out = {'p ' + n: p.detach().cpu() for n, p in net.named_parameters()}
    out.update({'b ' + n: b.detach().cpu() for n, b in net.named_buffers()})
    out.update({'m ' + n: momentum_of(p).detach().cpu() for n, p in net.named_parameters()})
    for i, l in enumerate(losses):
        out.update({'loss %d %s' % (i, k): v.detach().cpu().view(1) for k, v in l.items()})
    return out


def run_trainer(net, inputs, steps):
    tr = Trainer(net)
    assert type(tr.criterion) is MultiBoxLoss and tr.batch_stats is True
    losses = []
    for it in range(steps):
        torch.manual_seed(LOSS_SEED + it)
        losses.append(tr.step(*inputs))
    torch.cuda.synchronize()
    assert tr.iteration == steps and tr.optimizer.uploads == 1 and tr.optimizer.launches == steps
    assert int(tr.optimizer.skipped.item()) == 0
    return snapshot(net, lambda p: tr.optimizer.state[p]['momentum_buffer'], losses)


def run_by_hand(net, inputs, steps):
    """The same loop from its parts; the update as separate once-rounded torch operations (no alpha=, nothing to contract)."""
    cfg = yolact_amd.config.cfg
    images, targets, masks, num_crowds = inputs
    crit = MultiBoxLoss(cfg.num_classes, cfg.positive_iou_threshold, cfg.negative_iou_threshold, cfg.ohem_negpos_ratio)
    f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=DEV)
    mom, wd = f32(cfg.momentum), f32(cfg.decay)
    bufs = {p: torch.zeros_like(p) for p in net.parameters()}
    losses = []
    for it in range(steps):
        torch.manual_seed(LOSS_SEED + it)
        lr = f32(lr_at(it, cfg))
        l = crit(net, net.forward_train(images, True), targets, masks, num_crowds)
        sum(l.values()).backward()
        with torch.no_grad():
            for p in net.parameters():
                assert p.grad is not None
                d = torch.add(p.grad, torch.mul(p, wd))
                m = torch.add(torch.mul(bufs[p], mom), d)
                bufs[p].copy_(m)
                p.copy_(torch.sub(p, torch.mul(m, lr)))
                p.grad.zero_()
        losses.append(l)
    torch.cuda.synchronize()
    return snapshot(net, lambda p: bufs[p], losses)


def test_a_step_is_its_parts(case):
    net, state, inputs = case
    reset(net, state)
    a = run_trainer(net, inputs, 3)
    reset(net, state)
    b = run_by_hand(net, inputs, 3)
    assert sorted(a) == sorted(b) and len([k for k in a if k.startswith('loss 2')]) == 4
    same_bits(a, b)
    reset(net, state)
    same_bits(a, run_trainer(net, inputs, 3))                      # and again: the same bits
    moved = [n for n, p in net.named_parameters() if not torch.equal(a['p ' + n], state[n].cpu())]
    # one step moves every parameter: weight decay alone does that, so this does NOT show that the backward reaches each (here the
    # gradients of fpn.downsample_layers.* are exactly zero); tests/test_gpu_train_grads.py shows it, on cases where every one is not
    assert len(moved) == len(list(net.parameters()))
    assert any(not torch.equal(a['b ' + n], state[n].cpu()) for n, _ in net.named_buffers() if 'running_mean' in n)
    for k in [k for k in a if k.startswith('loss')]:
        assert bool(torch.isfinite(a[k]).all()), k


def test_the_schedule_reaches_the_optimiser(case):
    net, state, inputs = case
    reset(net, state, lr_warmup_until=2, lr_steps=(3,))
    cfg = yolact_amd.config.cfg
    tr = Trainer(net)
    seen = []
    for it in range(5):
        torch.manual_seed(LOSS_SEED + it)
        tr.step(*inputs)
        seen.append(tr.optimizer.param_groups[0]['lr'])
        assert seen[-1] == lr_at(it, cfg)
    torch.cuda.synchronize()
    assert seen == [1e-4, (1e-3 - 1e-4) * 0.5 + 1e-4, (1e-3 - 1e-4) * 1.0 + 1e-4, 1e-3 * 0.1, 1e-3 * 0.1]


def test_it_trains(case):
    """Constant learning rate, as tools/make_golden_train_step.py ran the reference: our total loss falls from iteration 0 to N by at least
    half of the reference's relative drop (the half is the margin: OHEM's discrete picks may differ between the two trajectories)."""
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'train_step.npz'))
    lr, n = float(g['lr']), int(g['N'])
    ref_drop = 1.0 - float(g['total_N']) / float(g['total_0'])
    assert lr <= 1e-3 and n <= 12 and ref_drop >= 0.10
    net, state, inputs = case
    reset(net, state, lr=lr, lr_warmup_until=0, lr_steps=())
    tr = Trainer(net)
    totals = []
    for it in range(n + 1):
        torch.manual_seed(LOSS_SEED + it)
        totals.append(sum(tr.step(*inputs).values()).detach())
        assert tr.optimizer.param_groups[0]['lr'] == lr
    totals = [float(t) for t in totals]                            # read after the loop: no step waited for the host
    print('reference', [round(float(v), 4) for v in g['totals']])
    print('ours     ', [round(v, 4) for v in totals])
    drop = 1.0 - totals[n] / totals[0]
    print('relative drop: reference %.4f, ours %.4f' % (ref_drop, drop))
    assert abs(totals[0] - float(g['total_0'])) <= 1e-3 * float(g['total_0'])      # the same weights and inputs: the same start
    assert drop >= 0.5 * ref_drop, (drop, ref_drop)
    assert int(tr.optimizer.skipped.item()) == 0


def test_plans_see_the_step(case):
    net, state, inputs = case
    reset(net, state)
    tr = Trainer(net)
    before = net._param_stamp()
    torch.manual_seed(LOSS_SEED)
    tr.step(*inputs)
    assert net._param_stamp() != before
    from yolact_amd.yolact import Yolact
    other = Yolact()
    other.load_state_dict(net.state_dict())
    other.to(DEV)
    for (n, p), (n2, q) in zip(net.named_parameters(), other.named_parameters()):
        assert n == n2
        same_bits(p.detach().cpu(), q.detach().cpu(), n)
    assert any(not torch.equal(p.detach().cpu(), state[n].cpu()) for n, p in net.named_parameters())
